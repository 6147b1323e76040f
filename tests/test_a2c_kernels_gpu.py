"""The A2C step and update kernels (csrc/vn_a2c.hip, the fused A2C branch of env_kernel in
csrc/vn_env.hip, vn_policy_heads) against the float64 references of oracle/a2c.py and
against each other where the header promises bit-identical results.

Bounds are derived, not measured: exact (bitwise) wherever the arithmetic is exact — the env
step, the bookkeeping, dyadic reward sums, the schedule — and otherwise the number of fp32
roundings of the kernel times 2^-24 of the stated scale, or the project's 1e-5 bar
(tests/test_policy_gpu.py). Every test prints the error of the element closest to its bound
next to that bound ("A2CERR ..." lines, shown with pytest -s). Outputs are pre-filled with NaN / sentinels, so
an element the kernel should have written and did not, or wrote and should not have, fails.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import a2c as oa2c
from oracle import a2c_cases as cases
from oracle import envs as oe
from oracle import graph as og
from oracle.frames import synth_frames

pytestmark = pytest.mark.gpu

NAN = float("nan")
EPS24 = 2.0 ** -24
VN_EINVAL = -1
CF, CD, U64, I64 = ctypes.c_float, ctypes.c_double, ctypes.c_uint64, ctypes.c_int64


def _l():
    from vnav import _lib
    return _lib, _lib.load(), _lib.stream_ptr(torch.device("cuda", 0))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def full(shape, value, dtype=torch.float32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype, device="cuda")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def report(what, err, bound):
    print("A2CERR %-46s worst %.3e  bound %.3e" % (what, err, bound))


def within(what, got, ref, bound):
    """max |got - ref| <= bound (bound a scalar or per element), in float64."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: non-finite output" % what
    err = np.abs(got - ref).reshape(-1)
    b = np.broadcast_to(np.asarray(bound, dtype=np.float64), got.shape).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0.0, err / b, 0.0)  # the element closest to (or farthest past) its bound
    k = int(np.argmax(ratio))
    report(what, err[k], b[k])
    assert (err <= b).all(), "%s: err %.3g > bound %.3g at %d" % (what, err[k], b[k], k)


def within_scale(what, got, ref, rtol):
    """max |got - ref| <= rtol * max |ref| (the project's 'rtol of the tensor's scale')."""
    within(what, got, ref, rtol * np.abs(np.asarray(ref, dtype=np.float64)).max())


# ---- 1. vn_step_a2c against independent references ------------------------------------

def step_scenes():
    import vnav
    out = []
    for k, (X, Y, p) in enumerate([(6, 8, 0.3), (5, 5, 0.0), (7, 4, 0.25)]):
        maze = np.random.RandomState(40 + k).rand(X, Y) >= p
        graph, spd, _ = og.h5_tables(maze)
        frames = synth_frames(7 + k, np.arange(len(graph)), (6, 10, 3))
        out.append(vnav.scene_from_arrays(graph, spd, frames, rewards=cases.STEP_REWARDS))
    return out


def step_env(E):
    import vnav
    sc = step_scenes()
    return vnav.VectorEnv(sc, E, seed=cases.STEP_ENV_SEED, max_episode_steps=cases.STEP_MAX_EPISODE_STEPS), sc


class StepBuffers:
    """The caller-owned buffers of one env step; poison() fills every output with a value
    no step writes."""

    def __init__(self, E, A):
        self.E, self.A = E, A
        self.out = full((E, 8), NAN)
        self.actions = full(E, -7, torch.int32)
        self.prev_action = full(E, -7, torch.int64)
        self.prev_reward, self.prev_mask = full(E, NAN), full(E, NAN)
        self.lra, self.mask = full((E, A + 1), NAN), full(E, NAN)
        self.reward = full(E, NAN)
        self.done = full(E, True, torch.bool)
        self.state = full(E, -7, torch.int32)
        self.base = torch.tensor([cases.COUNTER_BASE], dtype=torch.int64, device="cuda")

    def poison(self):
        for t in (self.actions, self.prev_action, self.state):
            t.fill_(-7)
        for t in (self.prev_reward, self.prev_mask, self.lra, self.mask, self.reward):
            t.fill_(NAN)

    def a2c_step(self, seed, stats_env):
        _lib, _, _ = _l()
        s = _lib.A2CStep()
        s.policy_out = self.out.data_ptr()
        s.num_actions = self.A
        s.seed = seed
        s.counter_base_dev = self.base.data_ptr()
        s.counter = 0
        s.actions = self.actions.data_ptr()
        s.prev_action = self.prev_action.data_ptr()
        s.prev_reward = self.prev_reward.data_ptr()
        s.prev_mask = self.prev_mask.data_ptr()
        s.lra_next = self.lra.data_ptr()
        s.mask_next = self.mask.data_ptr()
        s.episode_stats_env = stats_env.data_ptr()
        return s

    def snapshot(self, env):
        d = dict(actions=self.actions, reward=self.reward, done=self.done, state=self.state,
                 prev_action=self.prev_action, prev_reward=self.prev_reward, prev_mask=self.prev_mask,
                 lra=self.lra, mask=self.mask)
        for k in ("ep_return", "ep_length", "img_row", "goal_row"):
            d[k] = env._info[k]
        return {k: host(v).copy() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def fused_run(E, A):
    """STEP_K fused steps on fresh random policy outputs: every output of every step, the
    per-env episode statistics, their reduction and the env's error flags. Run once per
    (E, A) and shared by the tests below (never modified)."""
    _lib, lib, st = _l()
    env, _ = step_env(E)
    b = StepBuffers(E, A)
    stats_env = torch.zeros((3, E), dtype=torch.float32, device="cuda")
    s = b.a2c_step(cases.STEP_SEED, stats_env)
    steps = []
    for t in range(cases.STEP_K):
        b.out.copy_(torch.as_tensor(cases.step_policy_out(E, A, t)))
        b.poison()
        s.counter = t
        env.step_a2c(s, b.reward, b.done, b.state)
        steps.append(b.snapshot(env))
    before = host(stats_env).copy()
    stats3 = full(3, NAN)
    _lib.check(lib.vn_a2c_episode_stats(_lib.ptr(stats_env), E, _lib.ptr(stats3), st), "episode_stats")
    res = dict(steps=steps, stats_env=before, stats3=host(stats3).copy(), stats_env_after=host(stats_env).copy(),
               flags=env.error_flags())
    env.close()
    return res


@pytest.mark.parametrize("E,A", cases.STEP_CASES)
def test_step_a2c_vs_references(E, A):
    """The trainer's rollout step: the sampled actions equal the fp64 inverse-CDF draw (but
    for draws within DRAW_MARGIN of a boundary), an env oracle stepped with those actions gives
    the same rewards (bits), dones, states, frame rows and episode returns / lengths, the
    bookkeeping equals step_post64 exactly, and the per-env episode statistics and their
    reduction equal the oracle's sums bitwise. E = 301 is no multiple of the 4 envs per
    workgroup, 2500 exceeds the 1024 threads of the statistics kernel; at A = 7 actions >= 4
    flag VN_FLAG_BAD_ACTION and act as blocked moves."""
    r = fused_run(E, A)
    sc = step_scenes()
    o = oe.VectorEnvOracle([dict(graph=s.graph, spd=s.spd, rewards=s.rewards, terminal_obs=s.terminal_obs)
                            for s in sc], E, cases.STEP_ENV_SEED, max_steps=cases.STEP_MAX_EPISODE_STEPS)
    acc = np.zeros((3, E), dtype=np.float32)
    excluded = n_done = 0
    for t, g in enumerate(r["steps"]):
        act, dist = oa2c.categorical_draw64(cases.step_policy_out(E, A, t), A, cases.STEP_SEED,
                                            cases.COUNTER_BASE + t, np.arange(E))
        keep = dist >= cases.DRAW_MARGIN
        excluded += int((~keep).sum())
        a = g["actions"]
        assert ((a >= 0) & (a < A)).all(), t
        assert np.array_equal(a[keep], act[keep]), (t, np.nonzero(a[keep] != act[keep])[0][:8])
        ref = o.step(a)
        assert same_bits(g["reward"], ref["reward"]), t
        assert np.array_equal(g["done"], ref["done"]), t
        assert np.array_equal(g["state"], ref["state"]), t
        assert np.array_equal(g["img_row"], ref["img_row"]), t
        assert np.array_equal(g["goal_row"], ref["goal_row"]), t
        assert same_bits(g["ep_return"], ref["ep_return"]), t
        assert np.array_equal(g["ep_length"], ref["ep_length"]), t
        lra, m, _ = oa2c.step_post64(a, ref["reward"], ref["done"], ref["ep_return"], ref["ep_length"], A)
        assert np.array_equal(g["lra"].astype(np.float64), lra), t
        assert np.array_equal(g["mask"].astype(np.float64), m), t
        assert g["prev_action"].dtype == np.int64 and np.array_equal(g["prev_action"], a), t
        assert same_bits(g["prev_reward"], ref["reward"]), t
        assert np.array_equal(g["prev_mask"].astype(np.float64), m), t
        d = ref["done"]
        acc[0, d] += np.float32(1.0)
        acc[1, d] += ref["ep_return"][d]
        acc[2, d] += ref["ep_length"][d].astype(np.float32)
        n_done += int(d.sum())
    total = E * cases.STEP_K
    report("step E=%d A=%d draws excluded / total" % (E, A), excluded, cases.MAX_EXCLUDED_SHARE * total)
    assert excluded <= cases.MAX_EXCLUDED_SHARE * total
    assert n_done >= total // (2 * cases.STEP_MAX_EPISODE_STEPS)  # many episodes ended
    assert same_bits(r["stats_env"], acc)
    assert np.array_equal(r["stats3"].astype(np.float64), acc.astype(np.float64).sum(1))
    assert not r["stats_env_after"].any()
    if A > 4:
        assert any((g["actions"] > 3).any() for g in r["steps"])
        assert r["flags"] == o.flags == oe.FLAG_BAD_ACTION
    else:
        assert r["flags"] == o.flags == 0


# ---- 2. promised equivalences, bitwise ------------------------------------------------

@pytest.mark.parametrize("E", [5, 301, 2500])
def test_fused_step_equals_unfused_chain(E):
    """vn_step_a2c against vn_policy_sample_dev -> index-only vn_step -> vn_a2c_step_post on a
    second env of the same seed: every output of every step is bit-identical, and the
    statistics vn_a2c_step_post accumulates equal the reduced per-env ones."""
    A = 4
    r = fused_run(E, A)
    _lib, lib, st = _l()
    P = _lib.ptr
    env, _ = step_env(E)
    b = StepBuffers(E, A)
    stats3 = torch.zeros(3, dtype=torch.float32, device="cuda")
    for t in range(cases.STEP_K):
        b.out.copy_(torch.as_tensor(cases.step_policy_out(E, A, t)))
        b.poison()
        _lib.check(lib.vn_policy_sample_dev(P(b.out), E, A, U64(cases.STEP_SEED), P(b.base), U64(t), P(b.actions),
                                            None, None, None, st), "sample_dev")
        _lib.check(lib.vn_step(env._ctx, P(b.actions), None, None, P(b.reward), P(b.done), P(b.state), st), "vn_step")
        _lib.check(lib.vn_a2c_step_post(P(b.actions), P(b.reward), P(b.done), P(env._info["ep_return"]),
                                        P(env._info["ep_length"]), E, A, P(b.prev_action), P(b.prev_reward),
                                        P(b.prev_mask), P(b.lra), P(b.mask), P(stats3), st), "step_post")
        snap = b.snapshot(env)
        for k, v in r["steps"][t].items():
            assert same_bits(snap[k], v), (t, k)
    assert same_bits(host(stats3), r["stats3"])
    assert env.error_flags() == 0
    env.close()


@pytest.mark.parametrize("A", [1, 4, 7])
@pytest.mark.parametrize("n", [1, 257, 5000])
def test_sample_dev_equals_sample(n, A):
    """vn_policy_sample_dev(base_dev, offset) against vn_policy_sample(counter = base +
    offset): identical actions, logp, entropy and value; value is column A bit for bit; logp
    and entropy within 1e-5 of their tensor's scale of softmax_stats64."""
    _lib, lib, st = _l()
    P = _lib.ptr
    rng = np.random.RandomState([77, n, A])
    out = np.full((n, 8), np.nan, dtype=np.float32)
    out[:, :A] = (rng.randn(n, A) * 3.0).astype(np.float32)
    out[:, A] = rng.randn(n).astype(np.float32)
    out_d = dev(out)
    base = torch.tensor([cases.COUNTER_BASE], dtype=torch.int64, device="cuda")
    seed, off = 0xC0FFEE0000000123, 11
    res = []
    for form in ("host", "dev"):
        a, lp, H, v = full(n, -7, torch.int32), full(n, NAN), full(n, NAN), full(n, NAN)
        if form == "host":
            _lib.check(lib.vn_policy_sample(P(out_d), n, A, U64(seed), U64(cases.COUNTER_BASE + off), P(a), P(lp),
                                            P(H), P(v), st), "sample")
        else:
            _lib.check(lib.vn_policy_sample_dev(P(out_d), n, A, U64(seed), P(base), U64(off), P(a), P(lp), P(H),
                                                P(v), st), "sample_dev")
        res.append([host(x) for x in (a, lp, H, v)])
    for x, y, name in zip(res[0], res[1], ("actions", "logp", "entropy", "value")):
        assert same_bits(x, y), name
    a, lp, H, v = res[0]
    assert ((a >= 0) & (a < A)).all()
    assert same_bits(v, out[:, A])
    _, lp64, H64 = oa2c.softmax_stats64(out[:, :A])
    within_scale("sample n=%d A=%d logp" % (n, A), lp, lp64[np.arange(n), a], 1e-5)
    within_scale("sample n=%d A=%d entropy" % (n, A), H, H64, 1e-5)


def _heads_policy(E):
    from vnav.policy import PolicyNet
    net = PolicyNet((84, 84), cases.HEADS_A, recurrent=True)
    params = net.init_params(3)
    w, b, h = cases.heads_inputs(E)
    w_off, b_off = net.offsets["head"]
    params[w_off:w_off + w.size] = dev(w.reshape(-1))
    params[b_off:b_off + b.size] = dev(b)
    return net, params, (w_off, b_off), w, b, h


def _heads64(w, b, h):
    ref = h.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
    mag = np.abs(h).astype(np.float64) @ np.abs(w).astype(np.float64).T
    return ref, mag


@pytest.mark.parametrize("E", cases.HEADS_CASES)
def test_in_step_heads(E):
    """The heads computed inside the env step (vn_a2c_step.head_weight): head_out is
    bit-equal to vn_policy_heads on the same rows, each output within 32 * 2^-24 * sum_k
    |w_k x_k| of the fp64 dot plus bias (16 fused steps per lane, 5 tree levels, the bias add:
    22 roundings, each at most 2^-24 of the partial sum's magnitude), and the action drawn from
    those logits is the fp64 draw's."""
    _lib, lib, st = _l()
    A = cases.HEADS_A
    net, params, (w_off, b_off), w, b, h = _heads_policy(E)
    h_d = dev(h)
    heads_out = full((E, 8), NAN)
    net.heads(params, h_d, E, heads_out)
    env, _ = step_env(E)
    bufs = StepBuffers(E, A)
    stats_env = torch.zeros((3, E), dtype=torch.float32, device="cuda")
    s = bufs.a2c_step(cases.HEADS_SEED, stats_env)
    s.head_weight = params.data_ptr() + 4 * w_off
    s.head_bias = params.data_ptr() + 4 * b_off
    s.head_input = h_d.data_ptr()
    s.head_out = bufs.out.data_ptr()
    bufs.poison()
    env.step_a2c(s, bufs.reward, bufs.done, bufs.state)
    got, want = host(bufs.out), host(heads_out)
    assert same_bits(got[:, :A + 1], want[:, :A + 1])
    assert np.isnan(got[:, A + 1:]).all()  # the step writes the A + 1 head outputs only
    ref, mag = _heads64(w, b, h)
    within("heads in step E=%d vs fp64" % E, got[:, :A + 1], ref, 32 * EPS24 * mag)
    a = host(bufs.actions)
    act, dist = oa2c.categorical_draw64(got, A, cases.HEADS_SEED, cases.COUNTER_BASE, np.arange(E))
    keep = dist >= cases.DRAW_MARGIN
    assert keep.all()  # tests/test_a2c_refs.py keeps these draws 1e-4 clear of the boundaries
    assert np.array_equal(a[keep], act[keep])
    assert env.error_flags() == 0
    env.close()


@pytest.mark.parametrize("n", [16, 17, 300])
def test_policy_heads_vs_fp64(n):
    """vn_policy_heads either side of kSkinnyRows (16) and on the wide path, at 1e-5 of scale."""
    net, params, _, w, b, h = _heads_policy(n)
    out = full((n, 8), NAN)
    net.heads(params, dev(h), n, out)
    ref, _ = _heads64(w, b, h)
    within_scale("vn_policy_heads n=%d" % n, host(out)[:, :cases.HEADS_A + 1], ref, 1e-5)


def test_step_a2c_refusals():
    """Arguments the fused step must refuse before any launch (VN_EINVAL, env untouched)."""
    _lib, lib, st = _l()
    E, A = 5, cases.HEADS_A
    net, params, (w_off, b_off), _, _, h = _heads_policy(E)
    h_d = torch.zeros(E * 512 + 4, dtype=torch.float32, device="cuda")
    env, _ = step_env(E)
    bufs = StepBuffers(E, A)
    bufs.out.zero_()
    other = torch.zeros((E, 8), dtype=torch.float32, device="cuda")
    stats_env = torch.zeros((3, E), dtype=torch.float32, device="cuda")
    before = host(env.get_state()).copy()

    def call(**kw):
        s = bufs.a2c_step(cases.HEADS_SEED, stats_env)
        s.head_weight = params.data_ptr() + 4 * w_off
        s.head_bias = params.data_ptr() + 4 * b_off
        s.head_input = h_d.data_ptr()
        s.head_out = bufs.out.data_ptr()
        for k, v in kw.items():
            setattr(s, k, v)
        return lib.vn_step_a2c(env._ctx, ctypes.byref(s), _lib.ptr(bufs.reward), _lib.ptr(bufs.done),
                               _lib.ptr(bufs.state), st)

    bufs.poison()
    assert call(head_out=other.data_ptr()) == VN_EINVAL
    assert call(head_input=h_d.data_ptr() + 4) == VN_EINVAL
    assert call(head_weight=params.data_ptr() + 4 * w_off + 4) == VN_EINVAL
    assert call(num_actions=0) == VN_EINVAL
    assert call(num_actions=8) == VN_EINVAL
    assert call(num_actions=0, head_weight=None) == VN_EINVAL
    assert call(num_actions=8, head_weight=None) == VN_EINVAL
    torch.cuda.synchronize()
    assert same_bits(host(env.get_state()), before)
    assert (host(bufs.actions) == -7).all() and np.isnan(host(bufs.reward)).all()
    env.close()


# ---- 3. the update-math kernels at the sizes and action counts never run ----------------

@pytest.mark.parametrize("A", [1, 4, 7])
@pytest.mark.parametrize("T,E", [(1, 1), (20, 257), (40, 1000)])
def test_returns_vs_fp64(T, E, A):
    """E > 256 runs returns_kernel's second workgroup; A selects the bootstrap column (the
    others hold NaN). Per element 4 T 2^-24 max|R|: two roundings per step, doubled."""
    _lib, lib, st = _l()
    P = _lib.ptr
    rng = np.random.RandomState([5, T, E, A])
    rewards = rng.randn(T, E).astype(np.float32)
    dones = (rng.rand(T, E) < 0.15).astype(np.uint8)
    boot = np.full((E, 8), np.nan, dtype=np.float32)
    boot[:, A] = rng.randn(E).astype(np.float32)
    rw, dn, bt = dev(rewards), dev(dones), dev(boot)
    R = full(T * E, NAN)
    _lib.check(lib.vn_a2c_returns(P(rw), P(dn), P(bt), T, E, A, CF(0.99), P(R), st), "returns")
    ref = oa2c.returns64(rewards, dones, boot, A, 0.99)
    within("returns T=%d E=%d A=%d" % (T, E, A), host(R).reshape(T, E), ref, 4 * T * EPS24 * np.abs(ref).max())


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("A", [1, 2, 4, 7])
@pytest.mark.parametrize("n", [1, 64, 257, 5000])
def test_loss_grad_vs_fp64(n, A, scale):
    """n > 256 adds several workgroups' sums with atomics; logit scale 30 saturates the
    softmax. dout within 1e-5 of its scale, the unused columns exactly 0, each statistic
    within 1e-5 of the sum of its terms' magnitudes; stats are zeroed by the call itself.
    The single saturated samples (n = 1, x30) are where logf(1 + s') lost the dominant
    action's log-probability and 3 % of the entropy (DESIGN.md "A2C contract")."""
    _lib, lib, st = _l()
    P = _lib.ptr
    rng = np.random.RandomState([6, n, A, int(scale)])
    out = np.full((n, 8), np.nan, dtype=np.float32)
    out[:, :A] = (rng.randn(n, A) * scale).astype(np.float32)
    out[:, A] = rng.randn(n).astype(np.float32)
    actions = rng.randint(0, A, size=n).astype(np.int32)
    rets = rng.randn(n).astype(np.float32)
    o_d, a_d, r_d = dev(out), dev(actions), dev(rets)
    dout, stats = full((n, 8), NAN), full(4, NAN)
    _lib.check(lib.vn_a2c_loss_grad(P(o_d), P(a_d), P(r_d), n, A, CF(0.5), CF(0.01), P(dout), P(stats), st), "loss_grad")
    first = host(stats).copy()
    ref, s64, mags = oa2c.loss_grad64(out, actions, rets, A, 0.5, 0.01)
    tag = "loss_grad n=%d A=%d x%d" % (n, A, int(scale))
    d = host(dout)
    within_scale(tag + " dout", d[:, :A + 1], ref[:, :A + 1], 1e-5)
    assert same_bits(d[:, A + 1:], np.zeros((n, 7 - A), dtype=np.float32))
    within(tag + " stats", first, s64, 1e-5 * mags)
    _lib.check(lib.vn_a2c_loss_grad(P(o_d), P(a_d), P(r_d), n, A, CF(0.5), CF(0.01), P(dout), P(stats), st), "loss_grad")
    within(tag + " stats, 2nd call", host(stats), s64, 1e-5 * mags)
    if n <= 256:  # one workgroup: no atomics between several, the sums repeat bit for bit
        assert same_bits(host(stats), first)


@pytest.mark.parametrize("n", [1, 255, 131079, 1500001])
def test_grad_norm_vs_fp64(n):
    """n > 131072 runs sumsq_partial_kernel's stride loop. Norm rtol 5e-7 (one fp32 rounding
    of g * scale, one of the result: 1.2e-7, times 4), clip coefficient rtol 1e-6; max_norm
    0.5 clips, 1e9 / 0 / -1 give exactly 1."""
    _lib, lib, st = _l()
    P = _lib.ptr
    g = np.random.RandomState([7, n]).randn(n).astype(np.float32)
    if n == 1:
        g[0] = -1.7  # norm > max_norm at every scale
    g_d = dev(g)
    worst_n = worst_c = 0.0
    for scale in (1.0, 0.5, 1.0 / 3.0):
        for max_norm in (0.5, 1e9, 0.0, -1.0):
            part, sc = full(512, NAN, torch.float64), full(2, NAN)
            _lib.check(lib.vn_grad_norm(P(g_d), I64(n), CF(scale), CF(max_norm), P(part), P(sc), st), "grad_norm")
            norm, coef = (float(x) for x in host(sc))
            rn, rc = oa2c.grad_norm64(g, scale, max_norm)
            worst_n = max(worst_n, abs(norm - rn) / rn)
            assert abs(norm - rn) <= 5e-7 * rn, (scale, max_norm, norm, rn)
            if max_norm == 0.5:
                assert rc < 1.0
                worst_c = max(worst_c, abs(coef - rc) / rc)
                assert abs(coef - rc) <= 1e-6 * rc, (scale, coef, rc)
            else:
                assert rc == 1.0 and coef == 1.0, (scale, max_norm, coef)
    report("grad_norm n=%d norm (relative)" % n, worst_n, 5e-7)
    report("grad_norm n=%d clip coefficient (relative)" % n, worst_c, 1e-6)


def test_grad_norm_square_overflows_fp32():
    """One 1e18 element: its square overflows fp32, not the double accumulator."""
    _lib, lib, st = _l()
    P = _lib.ptr
    n = 255
    g = np.random.RandomState(8).randn(n).astype(np.float32)
    g[7] = 1e18
    g_d = dev(g)
    part, sc = full(512, NAN, torch.float64), full(2, NAN)
    _lib.check(lib.vn_grad_norm(P(g_d), I64(n), CF(1.0), CF(0.5), P(part), P(sc), st), "grad_norm")
    norm, coef = (float(x) for x in host(sc))
    rn, rc = oa2c.grad_norm64(g, 1.0, 0.5)
    assert np.isfinite(norm) and abs(norm - rn) <= 5e-7 * rn
    assert abs(coef - rc) <= 1e-6 * rc
    report("grad_norm 1e18 element (relative)", abs(norm - rn) / rn, 5e-7)


@pytest.mark.parametrize("n", [1, 257, 524301])
def test_rmsprop_vs_fp64(n):
    """n > 524288 runs rmsprop_kernel's stride loop. Three steps, each from the kernel's own
    float32 state: the host-lr and device-lr forms are bit-equal, square_avg within 1e-6 of
    scale, the parameter step within 1e-5 max|step| + 2^-24 max|p| (the rounding of p +
    step), and parameters with zero gradient and zero square_avg do not change."""
    _lib, lib, st = _l()
    P = _lib.ptr
    rng = np.random.RandomState([9, n])
    p0 = rng.randn(n).astype(np.float32)
    zero = np.array(sorted({k for k in (3, 100, 256, 300000, n - 1) if 0 < k < n}), dtype=np.int64)
    pa, pb = dev(p0), dev(p0)
    sa, sb = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    scalars = dev(np.array([2.0, 0.75], dtype=np.float32))  # (norm, clip coefficient)
    scale, lr, alpha, eps = 0.5, 7e-4, 0.99, 1e-5
    lr_d = dev(np.array([lr], dtype=np.float32))
    worst_s = worst_p = 0.0
    for it in range(3):
        g = (rng.randn(n) * 0.01).astype(np.float32)
        g[zero] = 0.0
        g_d = dev(g)
        p_in, s_in = host(pa).copy(), host(sa).copy()
        _lib.check(lib.vn_rmsprop_step(P(pa), P(g_d), P(sa), I64(n), CF(scale), P(scalars), CF(lr), CF(alpha), CF(eps),
                                       st), "rmsprop")
        _lib.check(lib.vn_rmsprop_step_dev(P(pb), P(g_d), P(sb), I64(n), CF(scale), P(scalars), P(lr_d), CF(alpha),
                                           CF(eps), st), "rmsprop_dev")
        p_out, s_out = host(pa), host(sa)
        assert same_bits(p_out, host(pb)) and same_bits(s_out, host(sb)), it
        pr, sr = oa2c.rmsprop64(p_in, g, s_in, 0.75, scale, lr, alpha, eps)
        es = np.abs(s_out - sr).max() / np.abs(sr).max()
        assert es <= 1e-6, (it, es)
        step_ref = pr - p_in.astype(np.float64)
        bound = 1e-5 * np.abs(step_ref).max() + EPS24 * np.abs(p_in).max()
        ep = np.abs((p_out.astype(np.float64) - p_in.astype(np.float64)) - step_ref).max()
        assert ep <= bound, (it, ep, bound)
        worst_s, worst_p = max(worst_s, es), max(worst_p, ep / bound)
        assert same_bits(p_out[zero], p0[zero]) and not s_out[zero].any(), it
    report("rmsprop n=%d square_avg (of scale)" % n, worst_s, 1e-6)
    report("rmsprop n=%d parameter step (of its bound)" % n, worst_p, 1.0)


SCHEDULE_CASES = [  # (state3 before, max_time_steps, steps_per_update, T)
    ([0, 0, -9], 1e6, 80, 20),                          # total = 0
    ([cases.COUNTER_BASE, 400000, 3], 1e6, 2560, 20),   # mid-run
    ([100, 1000000, 0], 1e6, 80, 5),                    # total = max: lr exactly 0
    ([100, 5000000, 0], 1e6, 80, 5),                    # total > max
    ([7, 1234, 0], 0.0, 80, 20),                        # max_time_steps = 0: lr = lr0
    ([2 ** 40, 2 ** 31 + 12345, 0], 2.0 ** 33, 2 ** 31, 20),  # total above 2^31
]
LR0 = 7e-4


@pytest.mark.parametrize("case", range(len(SCHEDULE_CASES)))
def test_schedule_exact(case):
    _lib, lib, st = _l()
    P = _lib.ptr
    s0, mx, spu, T = SCHEDULE_CASES[case]
    state = dev(np.array(s0, dtype=np.int64))
    lr = full(1, NAN)
    _lib.check(lib.vn_a2c_schedule(P(state), P(lr), CD(LR0), CD(mx), I64(spu), T, st), "schedule")
    rs, rl = oa2c.schedule64(s0, LR0, mx, spu, T)
    total = s0[1]
    want = np.float32(LR0 * (1.0 - min(total / mx, 1.0))) if mx > 0 else np.float32(LR0)
    assert same_bits(rl, want)
    assert np.array_equal(host(state), rs)
    assert same_bits(host(lr)[0], rl)
    if total >= mx > 0:
        assert host(lr)[0] == 0.0


@pytest.mark.parametrize("E", [1, 256, 257, 1000])
def test_rollout_begin_exact(E):
    """Up to four workgroups launch and the schedule advances once; step 0's frame rows are
    copied, mask0 / lra0 are [one_hot(prev_action) | prev_reward] * prev_mask exactly; with
    mask0 = NULL the lra buffer is left alone. State and lr equal vn_a2c_schedule's."""
    _lib, lib, st = _l()
    P = _lib.ptr
    A = 4
    rng = np.random.RandomState([10, E])
    img = rng.randint(0, 2 ** 31 - 1, size=E).astype(np.int32)
    goal = rng.randint(0, 2 ** 31 - 1, size=E).astype(np.int32)
    pa = rng.randint(0, A, size=E).astype(np.int64)
    pr = rng.randn(E).astype(np.float32)
    pm = (rng.rand(E) < 0.7).astype(np.float32)
    img_d, goal_d, pa_d, pr_d, pm_d = dev(img), dev(goal), dev(pa), dev(pr), dev(pm)
    s0, mx, spu, T = SCHEDULE_CASES[1]
    rs, rl = oa2c.schedule64(s0, LR0, mx, spu, T)
    sched_state, sched_lr = dev(np.array(s0, dtype=np.int64)), full(1, NAN)
    _lib.check(lib.vn_a2c_schedule(P(sched_state), P(sched_lr), CD(LR0), CD(mx), I64(spu), T, st), "schedule")
    lra_ref, m_ref, _ = oa2c.step_post64(pa, pr, pm == 0, np.zeros(E), np.zeros(E), A)
    for with_mask in (True, False):
        state, lr = dev(np.array(s0, dtype=np.int64)), full(1, NAN)
        img_o, goal_o = full(E, -7, torch.int32), full(E, -7, torch.int32)
        mask0, lra0 = full(E, NAN), full((E, A + 1), NAN)
        _lib.check(lib.vn_a2c_rollout_begin(P(state), P(lr), CD(LR0), CD(mx), I64(spu), T, P(img_d), P(goal_d),
                                            P(img_o), P(goal_o), E, P(pa_d), P(pr_d), P(pm_d), A,
                                            P(mask0) if with_mask else None, P(lra0), st), "rollout_begin")
        assert np.array_equal(host(state), rs) and same_bits(host(state), host(sched_state)), with_mask
        assert same_bits(host(lr)[0], rl) and same_bits(host(lr), host(sched_lr)), with_mask
        assert same_bits(host(img_o), img) and same_bits(host(goal_o), goal), with_mask
        if with_mask:
            assert np.array_equal(host(mask0).astype(np.float64), m_ref)
            assert np.array_equal(host(lra0).astype(np.float64), lra_ref)
        else:
            assert np.isnan(host(mask0)).all() and np.isnan(host(lra0)).all()


def test_metrics_bit_equal():
    """vn_a2c_metrics[_ex] against its float32 restatement, the aux sum in (h0 + h2) + h1
    order; aux3 = NULL gives out[5] = 0; without unreal4 out[9..11] are not written."""
    _lib, lib, st = _l()
    P = _lib.ptr
    f = np.float32
    rng = np.random.RandomState(11)
    stats4 = (rng.randn(4) * 100).astype(f)
    inv_n = f(1.0) / f(2560)
    scalars2 = rng.rand(2).astype(f)
    aux3 = (rng.rand(3) * 1e4).astype(f)
    numel3 = np.array([2560 * 42 * 42, 2560 * 42 * 42 * 3, 2560 * 42 * 42 * 3 + 1], dtype=f)
    ep3 = np.array([17.0, -3.25, 211.0], dtype=f)
    un4 = (rng.rand(4) * 1e3).astype(f)
    norm3 = rng.rand(3).astype(f)
    d = [dev(x) for x in (stats4, scalars2, aux3, numel3, ep3, un4, norm3)]
    base = np.concatenate([(stats4 * inv_n).astype(f), scalars2[:1]])
    aux = f(f(aux3[0] / numel3[0]) + f(aux3[2] / numel3[2])) + f(aux3[1] / numel3[1])
    unreal = np.array([un4[0] * norm3[0], un4[1] * norm3[1], un4[3] * norm3[2]], dtype=f)
    sentinel = np.full(3, 777.0, dtype=f)
    for ex in (False, True):
        for with_aux in (True, False):
            for with_unreal in ((True, False) if ex else (False,)):
                out = full(12, 777.0)
                a3, n3 = (P(d[2]), P(d[3])) if with_aux else (None, None)
                if ex:
                    u4, un = (P(d[5]), P(d[6])) if with_unreal else (None, None)
                    _lib.check(lib.vn_a2c_metrics_ex(P(d[0]), CF(inv_n), P(d[1]), a3, n3, P(d[4]), u4, un, P(out), st),
                               "metrics_ex")
                else:
                    _lib.check(lib.vn_a2c_metrics(P(d[0]), CF(inv_n), P(d[1]), a3, n3, P(d[4]), P(out), st), "metrics")
                want = np.concatenate([base, [f(aux) if with_aux else f(0.0)], ep3,
                                       unreal if with_unreal else sentinel]).astype(f)
                assert same_bits(host(out), want), (ex, with_aux, with_unreal, host(out), want)


@pytest.mark.parametrize("A", [1, 4, 7])
@pytest.mark.parametrize("n", [1, 300])
def test_greedy_first_maximum(n, A):
    """np.argmax over the first A columns: the first maximum wins an exact tie, and larger
    values in the columns >= A are not looked at."""
    _lib, lib, st = _l()
    P = _lib.ptr
    rng = np.random.RandomState([12, n, A])
    out = np.full((n, 8), 100.0, dtype=np.float32)
    out[:, :A] = rng.randint(-2, 3, size=(n, A)).astype(np.float32)  # few values: many ties
    if A > 1:
        out[0, :A] = 1.0  # an all-way tie
    o_d = dev(out)
    a = full(n, -7, torch.int32)
    _lib.check(lib.vn_policy_greedy(P(o_d), n, A, P(a), st), "greedy")
    ref = np.argmax(out[:, :A], axis=1)
    assert np.array_equal(host(a), ref)
    if A > 1 and n > 1:
        srt = np.sort(out[:, :A], axis=1)
        assert (srt[:, -1] == srt[:, -2]).sum() > n // 10  # ties at the maximum did occur
