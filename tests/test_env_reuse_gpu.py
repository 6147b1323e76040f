"""Output reuse of vn_step / vn_observe (vn_set_output_reuse, VectorEnv(reuse_outputs=...)):
a frame is not copied when its output row already holds it from this env's previous step.

Bit-exact against the oracle on the 16-, 4- and 1-byte copy paths at a ragged env count
(37 = 9 full workgroups + 1 env), with episodes short enough (TimeLimit 3 and 11) that resets,
goal changes, blocked moves and terminal steps all occur within the 50 steps.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import envs as oe
from test_env_gpu import compare_step, oracle_of, small_scenes

pytestmark = pytest.mark.gpu

N, STEPS, SEED = 37, 50, 4242
# frame bytes 96 (16-B path), 180 (4-B), 105 (1-B), and 96 into buffers offset by 1 and 4 bytes
PATHS = [((4, 8, 3), 0), ((6, 10, 3), 0), ((5, 7, 3), 0), ((4, 8, 3), 1), ((4, 8, 3), 4)]
LIMITS = [3, 11]


def _vnav():
    import vnav
    return vnav


def mixed_actions(steps=STEPS, seed=5):
    rng = np.random.RandomState(seed)
    acts = []
    for t in range(steps):
        a = rng.randint(0, 4, size=N).astype(np.int32)
        if t % 7 == 3:  # invalid actions count as blocked moves
            a[::5] = -1
            a[1::6] = 4
        acts.append(a)
    return acts


@functools.lru_cache(maxsize=None)
def reference(max_steps):
    """(rows after the constructor's reset, actions, the oracle's 50 steps): computed once per
    TimeLimit, shared by every test and shape (the graphs do not depend on the frame shape)."""
    o = oracle_of(small_scenes(), N, SEED, max_steps=max_steps)
    first = o.observe()
    acts = mixed_actions()
    return first, acts, [o.step(a) for a in acts]


def row_changes(max_steps):
    """Per step: (image row unchanged [N], goal row unchanged [N]) against the previous step."""
    first, _, steps = reference(max_steps)
    prev = first
    out = []
    for r in steps:
        out.append((r["img_row"] == prev["img_row"], r["goal_row"] == prev["goal_row"]))
        prev = r
    return out


def make_out(shape, offset=0):
    """Caller-owned outputs inside one zeroed buffer (test_frame_copy_paths_ragged's layout)."""
    F = int(np.prod(shape))
    buf = torch.zeros(2 * (N * F + 16), dtype=torch.uint8, device="cuda")
    g0 = N * F + 16 + offset
    out = dict(image=buf[offset:offset + N * F].view((N,) + shape), goal=buf[g0:g0 + N * F].view((N,) + shape),
               reward=torch.empty(N, dtype=torch.float32, device="cuda"),
               done=torch.empty(N, dtype=torch.bool, device="cuda"),
               state=torch.empty(N, dtype=torch.int32, device="cuda"))
    return buf, out, (offset, offset + N * F, g0, g0 + N * F)


def outside_is_zero(buf, span):
    b = buf.cpu().numpy()
    i0, i1, g0, g1 = span
    return not b[:i0].any() and not b[i1:g0].any() and not b[g1:].any()


def arena_of(scenes):
    return np.concatenate([s.observations for s in scenes])


def dev(a):
    return torch.as_tensor(a, device="cuda")


def assert_all_row_cases(max_steps, start=0):
    """Steps start.. of the shared trajectory hold each of image same / changed x goal same /
    changed (from the oracle's rows; a seed that misses one is replaced, not the assertion)."""
    seen = set()
    for same_i, same_g in row_changes(max_steps)[start:]:
        seen |= set(zip(same_i.tolist(), same_g.tolist()))
    assert seen == {(True, True), (True, False), (False, True), (False, False)}, seen


@pytest.mark.parametrize("max_steps", LIMITS)
@pytest.mark.parametrize("shape,offset", PATHS)
def test_parity_with_reuse(shape, offset, max_steps):
    vnav = _vnav()
    sc = small_scenes(shape)
    arena = arena_of(sc)
    _, acts, steps = reference(max_steps)
    assert_all_row_cases(max_steps)
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=max_steps)
    buf, out, span = make_out(shape, offset)
    for t in range(STEPS):
        compare_step(env.step(dev(acts[t]), out=out), steps[t], arena, (shape, offset, t))
    assert env._reuse_on
    assert outside_is_zero(buf, span)
    assert env.error_flags() == oe.FLAG_BAD_ACTION


def poisoned_steps(step_fn, out, arena, max_steps, expect_skips, tag):
    """Fill both outputs with 0xAA before each of steps 1..STEPS-1 (the contract's violation,
    on purpose: it shows which rows a step wrote). A row whose oracle row did not change keeps
    0xAA when skips are expected; every other row holds its arena row."""
    _, acts, steps = reference(max_steps)
    changes = row_changes(max_steps)
    step_fn(acts[0])
    assert np.array_equal(out["image"].cpu().numpy(), arena[steps[0]["img_row"]])
    assert np.array_equal(out["goal"].cpu().numpy(), arena[steps[0]["goal_row"]])
    poison = np.full(arena.shape[1:], 0xAA, dtype=np.uint8)
    kept = 0
    for t in range(1, STEPS):
        out["image"].fill_(0xAA)
        out["goal"].fill_(0xAA)
        step_fn(acts[t])
        for name, rows, same in (("image", steps[t]["img_row"], changes[t][0]),
                                 ("goal", steps[t]["goal_row"], changes[t][1])):
            got = out[name].cpu().numpy()
            want = arena[rows].copy()
            if expect_skips:
                want[same] = poison
                kept += int(same.sum())
            assert np.array_equal(got, want), (tag, name, t)
    return kept


@pytest.mark.parametrize("max_steps", LIMITS)
@pytest.mark.parametrize("shape,offset", PATHS)
def test_skips_happen_only_where_allowed(shape, offset, max_steps):
    vnav = _vnav()
    sc = small_scenes(shape)
    arena = arena_of(sc)
    assert not (arena.reshape(len(arena), -1) == 0xAA).all(axis=1).any()
    assert_all_row_cases(max_steps, start=1)
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=max_steps)
    buf, out, span = make_out(shape, offset)
    kept = poisoned_steps(lambda a: env.step(dev(a), out=out), out, arena, max_steps, True, (shape, offset))
    assert kept > 0
    assert outside_is_zero(buf, span)


@pytest.mark.parametrize("max_steps", LIMITS)
@pytest.mark.parametrize("shape,offset", [PATHS[0], PATHS[2]])
def test_every_row_rewritten_without_reuse(shape, offset, max_steps):
    """reuse_outputs=False, and raw vn_step on a context whose setter was never called (the C
    default), rewrite every row."""
    vnav = _vnav()
    sc = small_scenes(shape)
    arena = arena_of(sc)
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=max_steps, reuse_outputs=False)
    _, out, _ = make_out(shape, offset)
    poisoned_steps(lambda a: env.step(dev(a), out=out), out, arena, max_steps, False, "reuse_outputs=False")
    assert not env._reuse_on

    raw = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=max_steps, reuse_outputs=False)
    _, out, _ = make_out(shape, offset)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def raw_step(a):
        a = dev(a)
        assert raw.lib.vn_step(raw._ctx, p(a), p(out["image"]), p(out["goal"]), p(out["reward"]), p(out["done"]),
                               p(out["state"]), raw._stream()) == 0
        torch.cuda.synchronize()

    poisoned_steps(raw_step, out, arena, max_steps, False, "raw vn_step")


def test_buffer_changes():
    vnav = _vnav()
    shape, max_steps = (4, 8, 3), 11
    sc = small_scenes(shape)
    arena = arena_of(sc)
    _, acts, steps = reference(max_steps)
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=max_steps)
    _, A, _ = make_out(shape)
    t = 0
    for _ in range(4):
        compare_step(env.step(dev(acts[t]), out=A), steps[t], arena, ("A", t))
        t += 1
    # a fresh zeroed B with a new out dict: complete
    _, B, _ = make_out(shape)
    compare_step(env.step(dev(acts[t]), out=B), steps[t], arena, ("B", t))
    t += 1
    # back into A, poisoned meanwhile: complete
    A["image"].fill_(0xAA)
    A["goal"].fill_(0xAA)
    compare_step(env.step(dev(acts[t]), out=A), steps[t], arena, ("A again", t))
    t += 1
    compare_step(env.step(dev(acts[t]), out=A), steps[t], arena, ("A again", t))
    t += 1
    # plain tensors, dropped by the caller and allocated again, 0xAA-filled. The env's buffer cache
    # still holds the first pair, so the new pair lands at other addresses (the recycled-address
    # case is test_recycled_address_gets_full_write)
    rest = {k: A[k] for k in ("reward", "done", "state")}
    C = dict(rest, image=torch.zeros((N,) + shape, dtype=torch.uint8, device="cuda"),
             goal=torch.zeros((N,) + shape, dtype=torch.uint8, device="cuda"))
    for _ in range(3):
        compare_step(env.step(dev(acts[t]), out=C), steps[t], arena, ("C", t))
        t += 1
    del C
    C = dict(rest, image=torch.full((N,) + shape, 0xAA, dtype=torch.uint8, device="cuda"),
             goal=torch.full((N,) + shape, 0xAA, dtype=torch.uint8, device="cuda"))
    compare_step(env.step(dev(acts[t]), out=C), steps[t], arena, ("C again", t))


def poison(out):
    out["image"].fill_(0xAA)
    out["goal"].fill_(0xAA)


def assert_rows(out, arena, ref, kept, tag):
    """Both outputs hold the oracle's arena rows, except 0xAA where kept = (image rows, goal
    rows) says the step left the poisoned row alone; returns how many rows that was."""
    n = 0
    for name, rows, same in (("image", ref["img_row"], kept and kept[0]), ("goal", ref["goal_row"], kept and kept[1])):
        want = arena[rows].copy()
        if kept:
            want[same] = 0xAA
            n += int(same.sum())
        assert np.array_equal(out[name].cpu().numpy(), want), (tag, name)
    return n


def test_armed_full_write_into_matching_rows():
    """The rows' addresses and arena rows match the records, so only the armed full write makes
    observe(out=...) into poisoned buffers complete; the step after it skips again."""
    vnav = _vnav()
    shape, max_steps = (4, 8, 3), 11
    sc = small_scenes(shape)
    arena = arena_of(sc)
    _, acts, steps = reference(max_steps)
    changes = row_changes(max_steps)
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=max_steps)
    _, out, _ = make_out(shape)
    for t in range(2):
        compare_step(env.step(dev(acts[t]), out=out), steps[t], arena, t)
    poison(out)
    env.observe(out=(out["image"], out["goal"]))
    assert_rows(out, arena, steps[1], None, "observe after poison")
    poison(out)
    env.step(dev(acts[2]), out=out)
    assert assert_rows(out, arena, steps[2], changes[2], "step after observe") > 0


def test_raw_setter_arms_and_rearms():
    """vn_set_output_reuse through ctypes: the first launch after on = 1 writes every row, later
    ones skip, calling it again re-arms one full write, on = 0 writes every row."""
    vnav = _vnav()
    shape, max_steps = (4, 8, 3), 11
    sc = small_scenes(shape)
    arena = arena_of(sc)
    _, acts, steps = reference(max_steps)
    changes = row_changes(max_steps)
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=max_steps, reuse_outputs=False)
    _, out, _ = make_out(shape)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def raw_step(t):
        a = dev(acts[t])
        assert env.lib.vn_step(env._ctx, p(a), p(out["image"]), p(out["goal"]), p(out["reward"]), p(out["done"]),
                               p(out["state"]), env._stream()) == 0
        torch.cuda.synchronize()

    assert env.lib.vn_set_output_reuse(env._ctx, 1) == 0
    poison(out)
    raw_step(0)
    assert_rows(out, arena, steps[0], None, "first launch after on = 1")
    raw_step(1)
    poison(out)
    raw_step(2)
    assert assert_rows(out, arena, steps[2], changes[2], "skips") > 0
    poison(out)
    assert env.lib.vn_set_output_reuse(env._ctx, 1) == 0
    raw_step(3)
    assert_rows(out, arena, steps[3], None, "re-armed")
    poison(out)
    raw_step(4)
    assert assert_rows(out, arena, steps[4], changes[4], "skips return") > 0
    poison(out)
    assert env.lib.vn_set_output_reuse(env._ctx, 0) == 0
    raw_step(5)
    assert_rows(out, arena, steps[5], None, "on = 0")


def test_recycled_address_gets_full_write():
    """step(a) returns fresh frames, the caller drops them, and new 0xAA-filled tensors come to lie
    at the same addresses. So that this does not hang on the caching allocator's mood, the env
    draws its fresh frames from a buffer the test owns and the new tensors are new views of it
    (data_ptr checked). The records still name those addresses and, for most envs, the rows to
    emit: only the armed full write makes step(out=those) complete."""
    vnav = _vnav()
    shape, max_steps = (4, 8, 3), 11
    sc = small_scenes(shape)
    arena = arena_of(sc)
    _, acts, steps = reference(max_steps)
    changes = row_changes(max_steps)
    assert changes[1][0].any() and changes[1][1].any()  # rows a stale record would wrongly keep
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=max_steps)
    F = int(np.prod(shape))
    pool = torch.zeros(2 * N * F, dtype=torch.uint8, device="cuda")
    views = lambda: (pool[:N * F].view((N,) + shape), pool[N * F:].view((N,) + shape))  # noqa: E731
    env._frames = views
    ret = env.step(dev(acts[0]))
    compare_step(ret, steps[0], arena, "fresh")
    old = (ret[0][0].data_ptr(), ret[0][1].data_ptr())
    del ret
    pool.fill_(0xAA)  # the bytes now belong to someone else
    img, goal = views()
    assert (img.data_ptr(), goal.data_ptr()) == old
    out = dict(image=img, goal=goal, reward=torch.empty(N, dtype=torch.float32, device="cuda"),
               done=torch.empty(N, dtype=torch.bool, device="cuda"),
               state=torch.empty(N, dtype=torch.int32, device="cuda"))
    compare_step(env.step(dev(acts[1]), out=out), steps[1], arena, "recycled")
    poison(out)
    env.step(dev(acts[2]), out=out)
    assert assert_rows(out, arena, steps[2], changes[2], "skips after the full write") > 0


def test_capture_leaves_the_arm():
    """A launch that is captured while the full write is armed, and never replayed, does not use
    the arm up: the next eager step still writes every row."""
    vnav = _vnav()
    shape, max_steps = (4, 8, 3), 11
    sc = small_scenes(shape)
    arena = arena_of(sc)
    _, acts, steps = reference(max_steps)
    changes = row_changes(max_steps)
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=max_steps)
    _, out, _ = make_out(shape)
    for t in range(2):
        compare_step(env.step(dev(acts[t]), out=out), steps[t], arena, t)
    a2 = dev(acts[2])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.observe(out=(out["image"], out["goal"]))  # arms; recorded, not run
    poison(out)
    env.step(a2, out=out)
    assert_rows(out, arena, steps[2], None, "eager step after a capture")
    poison(out)
    env.step(dev(acts[3]), out=out)
    assert assert_rows(out, arena, steps[3], changes[3], "skips return") > 0
    del g


def test_fresh_tensor_path():
    """step(a) without out after stepping in place: fresh tensors at recycled addresses get
    every row, and the next in-place step arms again."""
    vnav = _vnav()
    shape, max_steps = (4, 8, 3), 3
    sc = small_scenes(shape)
    arena = arena_of(sc)
    _, acts, steps = reference(max_steps)
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=max_steps)
    _, out, _ = make_out(shape)
    t = 0
    for _ in range(3):
        compare_step(env.step(dev(acts[t]), out=out), steps[t], arena, ("in place", t))
        t += 1
    assert env._reuse_on
    for _ in range(30):
        ret = env.step(dev(acts[t]))
        assert not env._reuse_on
        compare_step(ret, steps[t], arena, ("fresh", t))
        del ret
        junk = [torch.full((N,) + shape, 0xAA, dtype=torch.uint8, device="cuda") for _ in range(2)]
        del junk
        t += 1
    for _ in range(5):
        compare_step(env.step(dev(acts[t]), out=out), steps[t], arena, ("in place again", t))
        assert env._reuse_on
        t += 1


def test_reset_and_observe_between_steps():
    vnav = _vnav()
    shape, max_steps = (5, 7, 3), 11
    sc = small_scenes(shape)
    arena = arena_of(sc)
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=max_steps)
    o = oracle_of(sc, N, SEED, max_steps=max_steps)
    acts = mixed_actions(30, seed=9)
    _, out, _ = make_out(shape)
    for t in range(30):
        compare_step(env.step(dev(acts[t]), out=out), o.step(acts[t]), arena, t)
        if t % 6 == 2:  # masked reset (its fresh observation is dropped), then step in place
            mask = np.zeros(N, dtype=bool)
            mask[t % 3::3] = True
            env.reset(dev(mask))
            o.reset(mask)
        if t % 6 == 4:  # observe into the same buffers, then step on the cached buffers
            mask = np.zeros(N, dtype=bool)
            mask[1::4] = True
            _lib_reset(env, mask)
            o.reset(mask)
            img, goal = env.observe(out=(out["image"], out["goal"]))
            ob = o.observe()
            assert np.array_equal(img.cpu().numpy(), arena[ob["img_row"]]), t
            assert np.array_equal(goal.cpu().numpy(), arena[ob["goal_row"]]), t


def _lib_reset(env, mask):
    """vn_reset alone (VectorEnv.reset also observes into fresh tensors)."""
    from vnav import _lib
    m = dev(mask).to(torch.int32).contiguous()
    _lib.check(env.lib.vn_reset(env._ctx, _lib.ptr(m), env._stream()), "vn_reset")
    torch.cuda.synchronize()


def test_set_state_between_steps():
    """set_state to an earlier snapshot, then step in place: the same frames as a second env
    driven the same way with reuse_outputs=False."""
    vnav = _vnav()
    shape, max_steps = (4, 8, 3), 11
    sc = small_scenes(shape)
    arena = arena_of(sc)
    acts = mixed_actions(20, seed=3)
    envs = [vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=max_steps, reuse_outputs=r) for r in (True, False)]
    outs = [make_out(shape)[1] for _ in envs]
    snap = [None, None]

    def both(t):
        for env, out in zip(envs, outs):
            env.step(dev(acts[t]), out=out)
        for k in ("image", "goal", "reward", "done", "state"):
            assert torch.equal(outs[0][k], outs[1][k]), (k, t)
        rows = envs[1]._info["img_row"].cpu().numpy(), envs[1]._info["goal_row"].cpu().numpy()
        assert np.array_equal(outs[0]["image"].cpu().numpy(), arena[rows[0]]), t
        assert np.array_equal(outs[0]["goal"].cpu().numpy(), arena[rows[1]]), t

    for t in range(5):
        both(t)
    for i, env in enumerate(envs):
        snap[i] = (env.get_state().clone(), env.get_episode_returns().clone())
    for t in range(5, 12):
        both(t)
    for i, env in enumerate(envs):
        env.set_state(snap[i][0])
        env.set_episode_returns(snap[i][1])
    for t in range(12, 20):
        both(t)


def test_graph_replay():
    """A captured step(out=out) replays correctly: the records live on the device, so a step
    into other buffers between two replays makes the next replay write every row."""
    vnav = _vnav()
    shape, max_steps = (4, 8, 3), 3
    sc = small_scenes(shape)
    arena = arena_of(sc)
    _, acts, steps = reference(max_steps)
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=max_steps)
    _, out, _ = make_out(shape)
    _, other, _ = make_out(shape)
    static = torch.zeros(N, dtype=torch.int32, device="cuda")
    t = 0
    for _ in range(4):
        static.copy_(dev(acts[t]))
        compare_step(env.step(static, out=out), steps[t], arena, ("eager", t))
        t += 1
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = env.step(static, out=out)
    for k in range(30):
        static.copy_(dev(acts[t]))
        g.replay()
        compare_step(captured, steps[t], arena, ("replay", k))
        t += 1
        if k == 14:  # one eager step into other buffers between two replays
            compare_step(env.step(dev(acts[t]), out=other), steps[t], arena, ("other", k))
            t += 1
    assert env.error_flags() == oe.FLAG_BAD_ACTION
