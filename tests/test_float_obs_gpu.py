"""Float observations on the GPU: VectorEnv(obs_format="f32_chw") / vn_step_f32 / vn_observe_f32.

Every frame value is compared bitwise with ScaledFloatFrame's arithmetic on the oracle's rows,
``arena[row].transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)``; scalars and info as
test_env_gpu.compare_step does. The trajectory (37 envs = 9 full workgroups + 1, TimeLimit 11,
50 steps with invalid actions mixed in) is test_env_reuse_gpu's, computed once and shared.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import envs as oe
from oracle.frames import synth_frames
from oracle.trunk_checks import _err
from test_env_gpu import oracle_of, small_scenes
from test_env_reuse_gpu import N, SEED, STEPS, arena_of, assert_all_row_cases, dev, reference, row_changes

pytestmark = pytest.mark.gpu

LIMIT = 11
POISON = -1.0  # no observation value: they lie in [0, 1]


def _vnav():
    import vnav
    return vnav


def chw(shape):
    return (shape[2], shape[0], shape[1])


def unit(arena, rows):
    """The expected float frames of arena rows: TransposeImage + ScaledFloatFrame."""
    return arena[rows].transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want):
    return got.dtype == torch.float32 and tuple(got.shape) == want.shape and np.array_equal(bits(got), bits(want))


def compare_step_f32(env_out, o, arena, tag, second=None):
    (img, goal), reward, done, info = env_out
    assert np.array_equal(reward.cpu().numpy().view(np.uint32), o["reward"].view(np.uint32)), tag
    assert np.array_equal(done.cpu().numpy(), o["done"]), tag
    assert np.array_equal(info["state"].cpu().numpy(), o["state"]), tag
    assert np.array_equal(info["img_row"].cpu().numpy(), o["img_row"]), tag
    assert np.array_equal(info["goal_row"].cpu().numpy(), o["goal_row"]), tag
    assert np.array_equal(info["ep_length"].cpu().numpy(), o["ep_length"]), tag
    assert np.array_equal(info["terminal_state"].cpu().numpy(), o["terminal_state"]), tag
    assert np.array_equal(info["truncated"].cpu().numpy().astype(bool), o["truncated"]), tag
    assert np.array_equal(info["ep_return"].cpu().numpy().view(np.uint32), o["ep_return"].view(np.uint32)), tag
    assert same_bits(img, unit(arena, o["img_row"])), tag
    assert same_bits(goal, unit(arena, o["goal_row"])), tag


def make_out(shape, offset=0, n=N):
    """Caller-owned float outputs inside one zeroed buffer, `offset` floats in (the guard
    layout of test_frame_copy_paths_ragged, in floats)."""
    F = int(np.prod(shape))
    buf = torch.zeros(2 * (n * F + 16), dtype=torch.float32, device="cuda")
    g0 = n * F + 16 + offset
    out = dict(image=buf[offset:offset + n * F].view((n,) + chw(shape)),
               goal=buf[g0:g0 + n * F].view((n,) + chw(shape)),
               reward=torch.empty(n, dtype=torch.float32, device="cuda"),
               done=torch.empty(n, dtype=torch.bool, device="cuda"),
               state=torch.empty(n, dtype=torch.int32, device="cuda"))
    return buf, out, (offset, offset + n * F, g0, g0 + n * F)


def outside_is_zero(buf, span):
    b = bits(buf)
    i0, i1, g0, g1 = span
    return not b[:i0].any() and not b[i1:g0].any() and not b[g1:].any()


# Pixels per frame 32 (4-pixel lanes, 8 groups: less than one trip), 60 (15 groups), 35 (not a
# multiple of 4: the scalar path, planes only 4-B aligned), 32 into buffers offset by one float
# (the 4-B-aligned fallback), and 4680 = 1170 groups. As built, a trip of the two-frame form is
# 64 lanes x 4 loads = 256 groups and of the one-frame form 64 x 8 = 512 groups, so 1170 groups
# are 4 full trips + 146 (two-frame) and 2 full trips + 146 (one-frame), and the remainder of 146
# is two full 64-lane loads and a ragged third of 18 lanes.
PATHS = [((4, 8, 3), 0), ((6, 10, 3), 0), ((5, 7, 3), 0), ((4, 8, 3), 1), ((60, 78, 3), 0)]


@pytest.mark.parametrize("shape,offset", PATHS)
def test_parity_over_paths(shape, offset):
    vnav = _vnav()
    sc = small_scenes(shape)
    arena = arena_of(sc)
    _, acts, steps = reference(LIMIT)
    assert_all_row_cases(LIMIT)  # both frames / one frame / none to convert all occur
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=LIMIT, obs_format="f32_chw")
    assert env.obs_shape == chw(shape) and env.obs_format == "f32_chw"
    buf, out, span = make_out(shape, offset)
    for t in range(STEPS):
        compare_step_f32(env.step(dev(acts[t]), out=out), steps[t], arena, (shape, offset, t))
    assert env._reuse_on
    assert outside_is_zero(buf, span)
    assert env.error_flags() == oe.FLAG_BAD_ACTION


def test_fresh_tensors_reset_and_observe():
    """Without out=: reset / observe / step return fresh contiguous float32 [E,C,H,W] tensors."""
    vnav = _vnav()
    shape = (6, 10, 3)
    sc = small_scenes(shape)
    arena = arena_of(sc)
    first, acts, steps = reference(LIMIT)
    env = vnav.make("CachedThor-v0", sc, N, seed=SEED, max_episode_steps=LIMIT, obs_format="f32_chw")
    img, goal = env.observe()
    assert img.is_contiguous() and goal.is_contiguous() and img.device.type == "cuda"
    assert same_bits(img, unit(arena, first["img_row"])) and same_bits(goal, unit(arena, first["goal_row"]))
    for t in range(12):
        compare_step_f32(env.step(dev(acts[t])), steps[t], arena, ("fresh", t))
        assert not env._reuse_on
    (img, goal), _, _, info = env.step(dev(acts[12]), gather=False)
    assert img is None and goal is None
    assert np.array_equal(info["img_row"].cpu().numpy(), steps[12]["img_row"])
    img, goal = env.reset()
    rows = env._info["img_row"].cpu().numpy(), env._info["goal_row"].cpu().numpy()
    assert same_bits(img, unit(arena, rows[0])) and same_bits(goal, unit(arena, rows[1]))


def test_one_frame_pointer_null():
    """vn_step_f32 / vn_observe_f32 with one frame pointer NULL: that frame is left alone, the other
    one is converted whatever the record says, and the next two-frame call is still right."""
    vnav = _vnav()
    shape = (4, 8, 3)
    sc = small_scenes(shape)
    arena = arena_of(sc)
    _, acts, steps = reference(LIMIT)
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=LIMIT, obs_format="f32_chw")
    _, out, _ = make_out(shape)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for t in range(3):
        compare_step_f32(env.step(dev(acts[t]), out=out), steps[t], arena, t)
    for t, k in ((3, "image"), (4, "goal")):
        out["image"].fill_(POISON)
        out["goal"].fill_(POISON)
        a = dev(acts[t])
        ptrs = [p(out["image"]) if k == "image" else None, p(out["goal"]) if k == "goal" else None]
        assert env.lib.vn_step_f32(env._ctx, p(a), ptrs[0], ptrs[1], p(out["reward"]), p(out["done"]), p(out["state"]),
                                   env._stream()) == 0
        torch.cuda.synchronize()
        row = steps[t]["img_row" if k == "image" else "goal_row"]
        other = "goal" if k == "image" else "image"
        assert same_bits(out[k], unit(arena, row)), (t, k)
        assert (out[other] == POISON).all().item(), (t, k)
        assert np.array_equal(out["state"].cpu().numpy(), steps[t]["state"])
    # the untouched frame's rows are poison now and their records still match: arm a full write
    assert env.lib.vn_set_output_reuse(env._ctx, 1) == 0
    assert env.lib.vn_observe_f32(env._ctx, p(out["image"]), p(out["goal"]), None, env._stream()) == 0
    torch.cuda.synchronize()
    assert same_bits(out["image"], unit(arena, steps[4]["img_row"]))
    assert same_bits(out["goal"], unit(arena, steps[4]["goal_row"]))
    compare_step_f32(env.step(dev(acts[5]), out=out), steps[5], arena, 5)


def test_full_frame_size():
    """84 x 84 (1764 groups = 6 two-frame trips + 228 = 3 one-frame trips + 228), 2 synthetic
    scenes, 8 envs, 30 steps."""
    vnav = _vnav()
    sc = [vnav.synthetic_scene(k) for k in range(2)]
    for s in sc:  # host copies of the frames, so the expected floats can be gathered
        s.observations = synth_frames(s.synth_id, np.arange(s.n_states), s.frame_shape)
    arena = arena_of(sc)
    n = 8
    env = vnav.VectorEnv(sc, n, seed=314, max_episode_steps=7, obs_format="f32_chw")
    o = oracle_of(sc, n, 314, max_steps=7)
    _, out, _ = make_out((84, 84, 3), n=n)
    rng = np.random.RandomState(2)
    for t in range(30):
        a = rng.randint(0, 4, size=n).astype(np.int32)
        compare_step_f32(env.step(dev(a), out=out), o.step(a), arena, t)
    assert env.error_flags() == 0


def poisoned_steps(step_fn, out, arena, expect_skips, tag):
    """test_env_reuse_gpu.poisoned_steps for float rows: both outputs are filled with POISON
    before each of steps 1..STEPS-1. A row whose oracle row did not change keeps the poison when
    skips are expected; every other row holds its frame, bit for bit."""
    _, acts, steps = reference(LIMIT)
    changes = row_changes(LIMIT)
    step_fn(acts[0])
    assert same_bits(out["image"], unit(arena, steps[0]["img_row"]))
    assert same_bits(out["goal"], unit(arena, steps[0]["goal_row"]))
    kept = 0
    for t in range(1, STEPS):
        out["image"].fill_(POISON)
        out["goal"].fill_(POISON)
        step_fn(acts[t])
        for name, rows, same in (("image", steps[t]["img_row"], changes[t][0]),
                                 ("goal", steps[t]["goal_row"], changes[t][1])):
            want = unit(arena, rows)
            if expect_skips:
                want[same] = np.float32(POISON)
                kept += int(same.sum())
            assert same_bits(out[name], want), (tag, name, t)
    return kept


@pytest.mark.parametrize("shape,offset", [PATHS[0], PATHS[2], PATHS[4]])
def test_reuse_skips_only_unchanged_rows(shape, offset):
    """(i) Rows the oracle says change are poisoned before the step, and only those: the outputs are
    bit-exact all the same (every changed row is rewritten). Then every row is poisoned: the rows
    the oracle says are unchanged keep the poison written into them (the skips happen)."""
    vnav = _vnav()
    sc = small_scenes(shape)
    arena = arena_of(sc)
    _, acts, steps = reference(LIMIT)
    changes = row_changes(LIMIT)
    assert_all_row_cases(LIMIT, start=1)
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=LIMIT, obs_format="f32_chw")
    buf, out, span = make_out(shape, offset)
    compare_step_f32(env.step(dev(acts[0]), out=out), steps[0], arena, 0)
    for t in range(1, STEPS):
        out["image"][dev(~changes[t][0])] = POISON
        out["goal"][dev(~changes[t][1])] = POISON
        compare_step_f32(env.step(dev(acts[t]), out=out), steps[t], arena, ("changed rows poisoned", t))
    assert outside_is_zero(buf, span)

    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=LIMIT, obs_format="f32_chw")
    buf, out, span = make_out(shape, offset)
    assert poisoned_steps(lambda a: env.step(dev(a), out=out), out, arena, True, (shape, offset)) > 0
    assert outside_is_zero(buf, span)


@pytest.mark.parametrize("shape,offset", [PATHS[0], PATHS[2]])
def test_every_row_rewritten_without_reuse(shape, offset):
    """(ii) reuse_outputs=False rewrites every row of every step."""
    vnav = _vnav()
    sc = small_scenes(shape)
    arena = arena_of(sc)
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=LIMIT, reuse_outputs=False, obs_format="f32_chw")
    _, out, _ = make_out(shape, offset)
    poisoned_steps(lambda a: env.step(dev(a), out=out), out, arena, False, "reuse_outputs=False")
    assert not env._reuse_on


def test_new_and_rebound_buffers_get_a_full_write():
    """(iii) A new out dict, the old one again after it was overwritten, and observe(out=...) into
    poisoned rows whose records match: each is a complete write."""
    vnav = _vnav()
    shape = (4, 8, 3)
    sc = small_scenes(shape)
    arena = arena_of(sc)
    _, acts, steps = reference(LIMIT)
    changes = row_changes(LIMIT)
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=LIMIT, obs_format="f32_chw")
    _, A, _ = make_out(shape)
    t = 0
    for _ in range(4):
        compare_step_f32(env.step(dev(acts[t]), out=A), steps[t], arena, ("A", t))
        t += 1
    _, B, _ = make_out(shape)
    B["image"].fill_(POISON)
    B["goal"].fill_(POISON)
    compare_step_f32(env.step(dev(acts[t]), out=B), steps[t], arena, ("B", t))
    t += 1
    A["image"].fill_(POISON)
    A["goal"].fill_(POISON)
    compare_step_f32(env.step(dev(acts[t]), out=A), steps[t], arena, ("A again", t))
    t += 1
    A["image"].fill_(POISON)
    A["goal"].fill_(POISON)
    img, goal = env.observe(out=(A["image"], A["goal"]))
    assert same_bits(img, unit(arena, steps[t - 1]["img_row"])) and same_bits(goal, unit(arena, steps[t - 1]["goal_row"]))
    # and the step after the full writes skips again
    A["image"].fill_(POISON)
    A["goal"].fill_(POISON)
    env.step(dev(acts[t]), out=A)
    want = unit(arena, steps[t]["goal_row"])
    want[changes[t][1]] = np.float32(POISON)
    assert changes[t][1].any() and same_bits(A["goal"], want)


def test_format_aliasing():
    """One float buffer and a uint8 view of the same storage (same data_ptr), reuse on, armed
    once, no reset: vn_step into the u8 view and vn_step_f32 into the float tensor in turn, with
    an invalid action (a blocked move: the emitted rows never change). Env 0's rows have the same
    address and arena row in both formats, so only the record's format bit makes each call write
    them; after each call the buffers hold that call's format in full."""
    vnav = _vnav()
    shape = (4, 8, 3)
    F = int(np.prod(shape))
    n = 5
    sc = small_scenes(shape)
    arena = arena_of(sc)
    env = vnav.VectorEnv(sc, n, seed=SEED, max_episode_steps=900, reuse_outputs=False)
    o = oracle_of(sc, n, SEED, max_steps=900)
    rows = o.observe()
    f_img = torch.zeros((n,) + chw(shape), dtype=torch.float32, device="cuda")
    f_goal = torch.zeros((n,) + chw(shape), dtype=torch.float32, device="cuda")
    u_img = f_img.view(-1).view(torch.uint8)[:n * F].view((n,) + shape)
    u_goal = f_goal.view(-1).view(torch.uint8)[:n * F].view((n,) + shape)
    assert u_img.data_ptr() == f_img.data_ptr() and u_goal.data_ptr() == f_goal.data_ptr()
    reward = torch.empty(n, dtype=torch.float32, device="cuda")
    done = torch.empty(n, dtype=torch.uint8, device="cuda")
    state = torch.empty(n, dtype=torch.int32, device="cuda")
    blocked = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    want_f = unit(arena, rows["img_row"]), unit(arena, rows["goal_row"])
    want_u = arena[rows["img_row"]], arena[rows["goal_row"]]

    def call(fmt):
        fn, img, goal = (env.lib.vn_step_f32, f_img, f_goal) if fmt == "f32" else (env.lib.vn_step, u_img, u_goal)
        assert fn(env._ctx, p(blocked), p(img), p(goal), p(reward), p(done), p(state), env._stream()) == 0
        torch.cuda.synchronize()
        assert not done.any().item()
        if fmt == "f32":
            assert same_bits(f_img, want_f[0]) and same_bits(f_goal, want_f[1]), fmt
        else:
            assert np.array_equal(u_img.cpu().numpy(), want_u[0]) and np.array_equal(u_goal.cpu().numpy(), want_u[1]), fmt

    assert env.lib.vn_set_output_reuse(env._ctx, 1) == 0
    for fmt in ("u8", "f32", "u8", "f32", "f32", "u8", "u8", "f32"):
        call(fmt)
    # the float records are in place again: a second float call skips every (unchanged) row
    f_img.fill_(POISON)
    f_goal.fill_(POISON)
    assert env.lib.vn_step_f32(env._ctx, p(blocked), p(f_img), p(f_goal), p(reward), p(done), p(state),
                               env._stream()) == 0
    torch.cuda.synchronize()
    assert (f_img == POISON).all().item() and (f_goal == POISON).all().item()
    assert env.error_flags() == oe.FLAG_BAD_ACTION


def test_graph_replay():
    """One captured step(out=float buffers), replayed 20 times against the oracle."""
    vnav = _vnav()
    shape = (4, 8, 3)
    sc = small_scenes(shape)
    arena = arena_of(sc)
    _, acts, steps = reference(LIMIT)
    env = vnav.VectorEnv(sc, N, seed=SEED, max_episode_steps=LIMIT, obs_format="f32_chw")
    buf, out, span = make_out(shape)
    static = torch.zeros(N, dtype=torch.int32, device="cuda")
    t = 0
    for _ in range(4):
        static.copy_(dev(acts[t]))
        compare_step_f32(env.step(static, out=out), steps[t], arena, ("eager", t))
        t += 1
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = env.step(static, out=out)
    for k in range(20):
        static.copy_(dev(acts[t]))
        g.replay()
        compare_step_f32(captured, steps[t], arena, ("replay", k))
        t += 1
    assert outside_is_zero(buf, span)
    del g


def test_companion_frames():
    """A small oriented scene with third-person frames: the second output is the companion frame
    of the observed state, converted."""
    vnav = _vnav()
    rng = np.random.RandomState(3)
    maze = np.ones((3, 3), dtype=bool)
    obs = rng.randint(0, 256, size=(3, 3, 4, 4, 8, 3)).astype(np.uint8)
    tp = rng.randint(0, 256, size=(3, 3, 4, 4, 8, 3)).astype(np.uint8)
    scene = vnav.oriented_scene(maze, obs, tp_observations=tp)
    E = 5
    env = vnav.VectorEnv([scene], E, seed=21, max_episode_steps=6, obs_format="f32_chw")
    o = oracle_of([scene], E, 21, max_steps=6)
    _, out, _ = make_out((4, 8, 3), n=E)
    for t in range(30):
        a = rng.randint(0, 4, size=E).astype(np.int32)
        (img, second), reward, done, info = env.step(dev(a), out=out)
        ref = o.step(a)
        assert np.array_equal(info["state"].cpu().numpy(), ref["state"]), t
        assert np.array_equal(done.cpu().numpy(), ref["done"]), t
        assert np.array_equal(reward.cpu().numpy().view(np.uint32), ref["reward"].view(np.uint32)), t
        assert np.array_equal(info["goal_row"].cpu().numpy(), scene.n_states + o.obs_state), t
        assert same_bits(img, unit(scene.observations, o.obs_state)), t
        assert same_bits(second, unit(scene.companion, o.obs_state)), t


def test_policy_on_float_observations_matches_u8():
    """GoalNavPolicy (84 x 84, 4 envs) on the float observations of an f32_chw env against the same
    policy on the u8 observations of an identically seeded u8_hwc env: logits and value within
    1e-5 of their scale (the bar of test_float_frames_of_u8_match_u8_run for these two paths)."""
    vnav = _vnav()
    from vnav.policy import GoalNavPolicy
    sc = [vnav.synthetic_scene(1)]
    n = 4
    envs = [vnav.VectorEnv(sc, n, seed=11, max_episode_steps=5, obs_format=f) for f in ("f32_chw", "u8_hwc")]
    torch.manual_seed(5)
    pol = GoalNavPolicy(3, 4, (84, 84))
    with torch.no_grad():
        pol.params.add_(torch.randn_like(pol.params) * 0.01)
    rng = np.random.RandomState(1)
    for t in range(3):
        a = dev(rng.randint(0, 4, size=n).astype(np.int32))
        (fi, fg), fr, fd, _ = envs[0].step(a)
        (ui, ug), ur, ud, _ = envs[1].step(a)
        assert torch.equal(fr, ur) and torch.equal(fd, ud)
        assert fi.dtype == torch.float32 and tuple(fi.shape) == (n, 3, 84, 84)
        assert same_bits(fi, unit(ui.cpu().numpy(), slice(None))) and same_bits(fg, unit(ug.cpu().numpy(), slice(None)))
        with torch.no_grad():
            fl, fv, _ = pol(((fi[:, None], fg[:, None]), None), None, None)
            ul, uv, _ = pol(((ui[:, None], ug[:, None]), None), None, None)
        torch.cuda.synchronize()
        e = {"logits": _err(fl.cpu().numpy(), ul.cpu().numpy()), "value": _err(fv.cpu().numpy(), uv.cpu().numpy())}
        print("float-obs policy cross-check step %d: %s" % (t, e))
        assert all(x <= 1e-5 for x in e.values()), (t, e)


def test_trainer_is_unaffected_by_the_format():
    """A2CTrainer is index-only: 4 envs, 84 x 84, 2 updates on an f32_chw env and on a u8_hwc env
    of the same seed give bitwise equal parameters."""
    vnav = _vnav()
    sc = [vnav.synthetic_scene(k) for k in range(2)]
    params = []
    for fmt in ("f32_chw", "u8_hwc"):
        env = vnav.VectorEnv(sc, 4, seed=21, max_episode_steps=6, obs_format=fmt)
        tr = vnav.A2CTrainer(env, num_steps=5, seed=3, max_time_steps=1e6)
        for _ in range(2):
            tr.step(sync=True)
        params.append(tr.params.detach().clone())
    assert torch.equal(params[0], params[1])
    assert params[0].abs().max().item() > 0


def test_bad_buffers_are_refused():
    """u8 buffers for an f32 env, float buffers of the wrong size, non-contiguous float buffers and
    float buffers for a u8 env raise before anything is launched."""
    vnav = _vnav()
    sc = small_scenes()
    n = 8
    env = vnav.VectorEnv(sc, n, seed=1, obs_format="f32_chw")
    F = int(np.prod(env.frame_shape))
    assert env.obs_shape == chw(env.frame_shape)
    mk = lambda dtype=torch.float32: torch.zeros((n,) + env.obs_shape, dtype=dtype, device="cuda")  # noqa: E731
    ok = dict(image=mk(), goal=mk(), reward=torch.empty(n, dtype=torch.float32, device="cuda"),
              done=torch.empty(n, dtype=torch.bool, device="cuda"),
              state=torch.empty(n, dtype=torch.int32, device="cuda"))
    a = torch.zeros(n, dtype=torch.int32, device="cuda")
    env.step(a, out=ok)
    bad = [("image", torch.zeros((n,) + env.frame_shape, dtype=torch.uint8, device="cuda")),
           ("goal", mk(torch.uint8)),
           ("goal", mk(torch.float16)),
           ("image", torch.zeros(n * F - 1, dtype=torch.float32, device="cuda")),
           ("goal", torch.zeros(n * F + 4, dtype=torch.float32, device="cuda")),
           ("image", torch.zeros((n, 2 * F), dtype=torch.float32, device="cuda")[:, ::2]),
           ("image", torch.zeros((n,) + env.obs_shape, dtype=torch.float32))]
    for k, t in bad:
        with pytest.raises(ValueError):
            env.step(a, out=dict(ok, **{k: t}))
        before = ok[k].clone()
        with pytest.raises(ValueError):
            env.observe(out=(t, ok["goal"]) if k == "image" else (ok["image"], t))
        assert torch.equal(ok[k], before)
    u8env = vnav.VectorEnv(sc, n, seed=1)
    assert u8env.obs_shape == u8env.frame_shape and u8env.obs_format == "u8_hwc"
    with pytest.raises(ValueError):
        u8env.step(a, out=ok)
    assert env.error_flags() == 0


def test_aux_observations_stay_u8():
    """aux_observations=True with f32_chw: image and goal are float CHW, the depth / segmentation
    frames stay uint8 HWC."""
    vnav = _vnav()
    rng = np.random.RandomState(5)
    maze = np.ones((3, 3), dtype=bool)
    obs = rng.randint(0, 256, size=(3, 3, 4, 4, 8, 3)).astype(np.uint8)
    dep = rng.randint(0, 256, size=(3, 3, 4, 4, 8, 1)).astype(np.uint8)
    seg = rng.randint(0, 256, size=(3, 3, 4, 4, 8, 3)).astype(np.uint8)
    scene = vnav.oriented_scene(maze, obs, depths=dep, segmentations=seg)
    E = 5
    env = vnav.VectorEnv([scene], E, seed=2, max_episode_steps=6, aux_observations=True, obs_format="f32_chw")
    frames = env.step(torch.zeros(E, dtype=torch.int32, device="cuda"))[0]
    rows = env._info["img_row"].cpu().numpy(), env._info["goal_row"].cpu().numpy()
    assert len(frames) == 5
    assert same_bits(frames[0], unit(scene.observations, rows[0])) and same_bits(frames[1], unit(scene.observations, rows[1]))
    assert np.array_equal(frames[2].cpu().numpy(), scene.depth[rows[0]])
    assert np.array_equal(frames[3].cpu().numpy(), scene.segmentation[rows[0]])
    assert np.array_equal(frames[4].cpu().numpy(), scene.segmentation[rows[1]])
