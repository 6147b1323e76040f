"""A2CTrainer(ppo_clip=..., ppo_epochs=..., optimizer=...): epoch 0 of a PPO update is the A2C
gradient; with learning_rate 0 every epoch's re-forward is the rollout's forward and every epoch's
gradient is epoch 0's; with a learning rate, epoch 1 runs on the stored rollout re-forwarded under
the parameters epoch 0 left, and its loss gradient is the fp64 restatement (tests/ppo_ref.py) on
exactly those head outputs; the captured hipGraph equals eager by bits, with RMSprop and with Adam;
a resume is exact, Adam's state included; the combinations out of scope are refused. 5 envs x 6
steps on the 5 x 6 maze of oracle.update_checks at 84 x 84, episodes of at most 4 steps so that
dones fall inside every rollout."""
import copy
import functools
import warnings

import numpy as np
import pytest
import torch

import ppo_ref as ref

pytestmark = pytest.mark.gpu

E, T, LIMIT = 5, 6, 4
CASES = {"goal-lstm": dict(arch="goal", recurrent=True), "goal-ff": dict(arch="goal", recurrent=False),
         "bighouse-lstm": dict(arch="bighouse", recurrent=True)}
PPO_KEYS = {"approx_kl", "clip_fraction", "ratio_mean", "value_clip_fraction"}


@functools.lru_cache(maxsize=None)
def _scene(aux=False):
    from oracle.update_checks import maze_scene
    return maze_scene((84, 84), aux)[0]


def make(case="goal-lstm", envs=E, steps=T, aux=False, **kw):
    import vnav
    env = vnav.VectorEnv([_scene(aux)], envs, seed=5, max_episode_steps=LIMIT)
    opts = dict(num_steps=steps, seed=9, max_time_steps=1e6, **CASES[case])
    opts.update(kw)
    return vnav.A2CTrainer(env, **opts)


def tensors(tr, flat):
    """{reference tensor name: float64 array} of a flat parameter-shaped buffer."""
    return {k: v.double().numpy() for k, v in tr.net.to_reference(flat).items()}


def worst_of_scale(got, want):
    """max over tensors of |got - want| / max |want| (tensors that are zero in both are skipped)."""
    worst = 0.0
    for k, w in want.items():
        s = np.abs(w).max()
        if s == 0:
            assert not got[k].any(), k
            continue
        worst = max(worst, float(np.abs(got[k] - w).max() / s))
    return worst


def bits_equal(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return torch.equal(a, b)


@pytest.mark.parametrize("case", list(CASES))
def test_epoch0_is_the_a2c_gradient(case):
    """Same seeds, one full step each; the PPO trainer then takes the A2C trainer's parameters (its
    own epochs moved them elsewhere), so the second rollouts agree bitwise, and the PPO update's
    epoch-0 gradient on that rollout is the A2C update's."""
    a = make(case)
    b = make(case, ppo_clip=0.2, ppo_epochs=2, ppo_normalize_advantage=False)
    a.step()
    b.step()
    b.params.copy_(a.params)
    if a.recurrent:
        assert torch.equal(a._hc0, b._hc0)  # the first rollouts were one rollout
    a.rollout()
    b.rollout()
    torch.cuda.synchronize()
    for name in ("out", "actions", "rewards", "dones", "rows_img", "rows_goal", "boot_out"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert int(a.dones.sum()) > 0
    seen = {}
    b.on_ppo_epoch = lambda k: seen.setdefault(k, b.grads.clone())
    a.update()
    b.update()
    torch.cuda.synchronize()
    assert sorted(seen) == [0, 1]
    err = worst_of_scale(tensors(b, seen[0]), tensors(a, a.grads))
    print("PPOERR %s epoch-0 grads vs A2C: %.3e of scale" % (case, err))
    assert err <= 1e-5, err
    assert torch.equal(a.returns, b.returns)


def _lr0_epochs(tr, K):
    """One step, then rollout + update with learning_rate 0 and the epoch checks of the issue."""
    tr.step()
    p0 = tr.params.clone()
    tr.rollout()
    torch.cuda.synchronize()
    N = tr.num_steps * tr.env.num_envs
    A = tr.A
    last = tr._hc_all.view(2, tr.num_steps, tr.env.num_envs, 512)[:, -1].clone() if tr.recurrent else None
    out_rollout = tr.out.clone()
    seen = []

    def hook(k):
        seen.append((k, tr.out.clone(), tr.grads.clone(), tr.ppo_stats.clone(), tr.out_old.clone()))

    tr.on_ppo_epoch = hook
    tr.update()
    torch.cuda.synchronize()
    assert [s[0] for s in seen] == list(range(K))
    g0 = tensors(tr, seen[0][2])
    actions = tr.actions.cpu().numpy()
    idx = np.arange(N)
    for k, out, grads, pstats, out_old in seen:
        assert torch.equal(out_old, out_rollout)
        o, oo = out.cpu().double().numpy()[:, :A + 1], out_old.cpu().double().numpy()[:, :A + 1]
        e_out = np.abs(o - oo).max() / np.abs(oo).max()
        e_g = worst_of_scale(tensors(tr, grads), g0)
        print("PPOERR lr=0 epoch %d: out %.3e of scale, grads %.3e of scale" % (k, e_out, e_g))
        assert e_out <= 1e-5 and e_g <= 1e-5, (k, e_out, e_g)
        kl, clipped, ratio, _ = pstats.cpu().double().numpy()
        assert clipped == 0.0
        d = ref.softmax_stats(o[:, :A])[1][idx, actions] - ref.softmax_stats(oo[:, :A])[1][idx, actions]
        mags = (np.abs(np.expm1(d)) + np.abs(d)).sum()
        assert abs(kl) <= 1e-5 * mags and abs(kl - (np.expm1(d) - d).sum()) <= 1e-5 * mags, (k, kl, mags)
        assert abs(ratio - N) <= 1e-5 * N
        if k == 0:
            assert kl == 0.0 and ratio == float(N)
    assert torch.equal(tr.params.view(torch.int32), p0.view(torch.int32))
    if tr.recurrent:
        assert torch.equal(tr._hc0, last)


@pytest.mark.parametrize("case", list(CASES))
def test_lr0_reforward_is_the_rollouts_forward(case):
    _lr0_epochs(make(case, ppo_clip=0.2, ppo_epochs=3, learning_rate=0.0), 3)


def test_lr0_with_aux_heads_and_with_goal_runs():
    tr = make("goal-lstm", aux=True, aux_weight=0.1, ppo_clip=0.2, ppo_epochs=3, learning_rate=0.0)
    assert tr.aux_source == "rollout"
    _lr0_epochs(tr, 3)
    assert float(tr.aux_stats.abs().sum()) > 0
    tr = make("goal-lstm", envs=18, steps=3, dedup_goals=True, ppo_clip=0.2, ppo_epochs=3, learning_rate=0.0)
    assert tr.dedup_goals
    _lr0_epochs(tr, 3)
    assert 0 < int(tr.goal_count[3]) < 3 * 18  # fewer goal frames than samples went through shared_base


@pytest.mark.parametrize("case", list(CASES))
def test_epoch1_runs_on_the_parameters_epoch0_left(case):
    tr = make(case, ppo_clip=0.2, ppo_epochs=2)
    tr.step()
    tr.rollout()
    torch.cuda.synchronize()
    net, N, A = tr.net, T * E, tr.A
    hc0 = tr._hc0.clone() if tr.recurrent else None
    seen = {}

    def hook(k):
        if k == 0:
            seen["params"] = tr.params.clone()
        else:
            seen.update(out=tr.out.clone(), dout=tr.dout.clone(), stats=tr.stats.clone(), pstats=tr.ppo_stats.clone())

    tr.on_ppo_epoch = hook
    tr.update()
    torch.cuda.synchronize()
    p1 = seen["params"]
    assert not torch.equal(p1, tr.params)
    # the stored rollout under the snapshot, with the test's own buffers
    acts = net.new_acts(N)
    out = torch.zeros((N, 8), device="cuda")
    frames = tr._frames(tr.rows_img, tr.rows_goal)
    if tr.recurrent:
        net.forward(p1, frames, N, acts, N, 0, None)
        x5 = net.x5(acts, N)
        f32 = dict(dtype=torch.float32, device="cuda")
        xcat, lacts = torch.zeros((N, net.lstm["xcat"]), **f32), torch.zeros((N, 2048), **f32)
        h, c, gates = torch.zeros((N, 512), **f32), torch.zeros((N, 512), **f32), torch.zeros((E, 2048), **f32)
        for t in range(T):
            sl = slice(t * E, (t + 1) * E)
            hp = hc0[0] if t == 0 else h[(t - 1) * E:t * E]
            cp = hc0[1] if t == 0 else c[(t - 1) * E:t * E]
            net.lstm_step(p1, E, x5[sl], tr.lra[t], tr.masks[t], hp, cp, xcat[sl], gates, lacts[sl], c[sl], h[sl])
        net.heads(p1, h, N, out)
    else:
        net.forward(p1, frames, N, acts, N, 0, out)
    torch.cuda.synchronize()
    got, want = seen["out"].cpu().double().numpy()[:, :A + 1], out.cpu().double().numpy()[:, :A + 1]
    e_out = np.abs(got - want).max() / np.abs(want).max()
    moved = np.abs(got - tr.out_old.cpu().double().numpy()[:, :A + 1]).max() / np.abs(want).max()
    print("PPOERR %s epoch-1 out vs the test's re-forward: %.3e of scale (moved %.3e from the rollout's)"
          % (case, e_out, moved))
    assert e_out <= 1e-5, e_out
    assert moved > 1e-4  # epoch 1 did not run on the rollout's parameters
    # the carried state is the behaviour policy's, and c0 stayed the start state during the update
    if tr.recurrent:
        assert not torch.equal(tr._hc0, hc0)
    r = ref.loss_grad(seen["out"].cpu().numpy(), tr.out_old.cpu().numpy(), tr.actions.cpu().numpy(),
                      tr.returns.cpu().numpy(), tr.adv_stats.cpu().numpy(), A, clip=0.2, value_clip=0.0,
                      vc=tr.value_coefficient, ec=tr.entropy_coefficient)
    assert min(float(m.min()) for m in r["margins"].values()) >= ref.MARGIN  # no sample near a branch
    dout = seen["dout"].cpu().double().numpy()
    e_d = np.abs(dout[:, :A + 1] - r["dout"][:, :A + 1]).max() / np.abs(r["dout"]).max()
    print("PPOERR %s epoch-1 dout vs fp64: %.3e of scale" % (case, e_d))
    assert e_d <= 1e-5, e_d
    assert not dout[:, A + 1:].any()
    # the advantage statistics are the rollout's, formed once
    want2 = ref.adv_stats(tr.returns.cpu().numpy() - tr.out_old.cpu().numpy()[:, A], np.zeros((N, 8)), A, 1e-8)
    assert (np.abs(tr.adv_stats.cpu().double().numpy() - want2) <= 1e-5 * np.abs(want2)).all()
    # and the metrics are the final epoch's
    m = tr._metric_layout
    assert list(m)[-1] == "ppo" and m["ppo"][1] == 4
    assert torch.equal(seen["pstats"], tr.ppo_stats) and torch.equal(seen["stats"], tr.stats)


@pytest.mark.parametrize("optimizer", ["rmsprop", "adam"])
def test_graph_is_bit_identical_to_eager(optimizer):
    runs = {}
    for graph in (False, True):
        tr = make("goal-lstm", ppo_clip=0.2, ppo_epochs=2, ppo_value_clip=0.2, optimizer=optimizer, cuda_graph=graph)
        raws = [tr.step(sync=False)["raw"].clone() for _ in range(3)]
        torch.cuda.synchronize()
        state = [tr.params.clone(), tr.square_avg.clone(), tr._hc0.clone(), tr.out.clone(), tr.ppo_stats.clone()]
        if optimizer == "adam":
            state += [tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.adam_step.clone()]
            assert int(tr.adam_step) == 6 and not tr.square_avg.any()  # one step per epoch
        runs[graph] = (state, raws)
        m = tr.step()
        assert PPO_KEYS <= set(m) and 0.0 <= m["clip_fraction"] <= 1.0 and m["ratio_mean"] > 0
    for x, y in zip(runs[True][0], runs[False][0]):
        assert bits_equal(x, y)
    for x, y in zip(runs[True][1], runs[False][1]):
        assert bits_equal(x, y)
    with pytest.raises(ValueError, match="on_ppo_epoch"):
        tr.on_ppo_epoch = lambda k: None


def test_resume_is_exact_with_adam_state():
    kw = dict(ppo_clip=0.2, ppo_epochs=2, optimizer="adam")
    a = make("goal-lstm", **kw)
    a.step()
    a.step()
    sd = copy.deepcopy(a.state_dict())
    assert int(sd["adam_step"]) == 4 and sd["exp_avg"].abs().sum() > 0 and sd["exp_avg_sq"].abs().sum() > 0
    a.step()
    b = make("goal-lstm", **kw)
    b.step()  # somewhere else: the load must replace it
    b.load_state_dict(sd)
    b.step()
    torch.cuda.synchronize()
    for name in ("params", "exp_avg", "exp_avg_sq", "adam_step", "returns", "out", "_hc0"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    # an RMSprop-era checkpoint into an Adam trainer: a warning, the moments start at zero
    old = {k: v for k, v in sd.items() if k not in ("exp_avg", "exp_avg_sq", "adam_step")}
    c = make("goal-lstm", **kw)
    c.step()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        c.load_state_dict(old)
    assert any("Adam" in str(x.message) for x in caught)
    assert int(c.adam_step) == 0 and not c.exp_avg.any() and not c.exp_avg_sq.any()
    m = c.step()
    assert np.isfinite(m["loss"]) and int(c.adam_step) == 2
    # the parameters-only form carries the state too
    d = make("goal-lstm", **kw)
    d.load_params_state_dict(a.params_state_dict())
    assert torch.equal(d.exp_avg, a.exp_avg) and torch.equal(d.adam_step, a.adam_step)


def test_adam_with_plain_a2c():
    """optimizer='adam' needs no PPO: one Adam step per update on the A2C gradient, which is the
    RMSprop trainer's gradient on the same first rollout."""
    a, b = make("goal-lstm"), make("goal-lstm", optimizer="adam")
    p0 = b.params.clone()
    a.step()
    m = b.step()
    torch.cuda.synchronize()
    assert not PPO_KEYS & set(m) and int(b.adam_step) == 1
    assert torch.equal(a.grads, b.grads)
    # the first Adam step: the bias corrections cancel, so it is lr g / (|g| + eps) of the clipped gradient
    g = (b.grads * b.scalars[1]).double()
    want = 7e-4 * g / (g.abs() + 1e-5)
    err = ((p0.double() - b.params.double()) - want).abs()
    assert bool((err <= 1e-3 * 7e-4 + 2.0 ** -23 * p0.abs().double()).all()), float(err.max())
    assert float(want.abs().max()) > 0.5 * 7e-4


def test_refusals():
    import vnav
    for bad in (dict(ppo_clip=0.0), dict(ppo_clip=-0.2), dict(ppo_clip=0.2, ppo_epochs=0), dict(ppo_epochs=0),
                dict(optimizer="sgd"), dict(ppo_clip=0.2, expert_weight=0.3)):
        with pytest.raises(ValueError):
            make("goal-lstm", **bad)
    with pytest.raises(ValueError, match="replay"):
        make("goal-lstm", aux=True, aux_weight=0.1, aux_source="replay", ppo_clip=0.2)
    with pytest.raises(ValueError, match="unreal"):
        make("bighouse-lstm", unreal=True, ppo_clip=0.2)

    class Group:  # a stand-in process group of two ranks
        pass

    from vnav import dist as vdist
    world_of = vdist.world_of
    vdist.world_of = lambda group=None: (2, 0) if isinstance(group, Group) else world_of(group)
    try:
        with pytest.raises(ValueError, match="world"):
            make("goal-lstm", ppo_clip=0.2, process_group=Group())
    finally:
        vdist.world_of = world_of

    class Custom(vnav.A2CTrainer):
        def compute_auxiliary_loss(self, model, batch, device):
            return None, {}

    env = vnav.VectorEnv([_scene()], E, seed=5, max_episode_steps=LIMIT)
    with pytest.raises(ValueError, match="compute_auxiliary_loss"):
        Custom(env, num_steps=T, recurrent=True, ppo_clip=0.2)
