"""The five-frame observation of AuxiliaryGraph-v0 in the step's own launch: vn_set_aux_arena,
vn_step_aux / vn_observe_aux, VectorEnv(aux_observations=True, aux_format=...).

Expected frames come straight from the scene arrays at the oracle's rows: depth and segmentation
at img_row, goal segmentation at goal_row; float frames are compared bitwise with
``x.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)``. The trajectory (37 envs = 9 full
workgroups + 1, TimeLimit 11, 50 steps with invalid actions mixed in) is test_env_reuse_gpu's,
computed once and shared.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch

from oracle import envs as oe
from oracle.frames import synth_frames
from test_env_gpu import oracle_of, small_scenes
from test_env_reuse_gpu import N, SEED, STEPS, assert_all_row_cases, dev, reference, row_changes
from test_float_obs_gpu import bits, same_bits, unit

pytestmark = pytest.mark.gpu

LIMIT = 11
KEYS = ("image", "goal", "depth", "segmentation", "goal_segmentation")
FORMATS = ("u8_hwc", "f32_chw")
# HW = 32: 16-B lanes for both row sizes (u8), 4-pixel lanes (f32); HW = 60: 4-B lanes (u8),
# 4-pixel lanes; HW = 35: bytes / the scalar float form; HW = 32 with every output offset by 1 and
# by 4 elements inside the guard buffer (u8: bytes, then 4-B lanes; f32: the scalar form on 4-B
# aligned planes, then 4-pixel lanes on a shifted base)
PATHS = [((4, 8, 3), 0), ((6, 10, 3), 0), ((5, 7, 3), 0), ((4, 8, 3), 1), ((4, 8, 3), 4)]


def _vnav():
    import vnav
    return vnav


def with_aux(scenes, seed=900):
    """The scenes with seeded random depth [n,H,W,1] / segmentation [n,H,W,3] attached."""
    out = []
    for k, s in enumerate(scenes):
        rng = np.random.RandomState(seed + k)
        H, W = s.frame_shape[:2]
        out.append(dataclasses.replace(
            s, depth=rng.randint(0, 256, size=(s.n_states, H, W, 1)).astype(np.uint8),
            segmentation=rng.randint(0, 256, size=(s.n_states, H, W, 3)).astype(np.uint8)))
    return out


@functools.lru_cache(maxsize=None)
def aux_scenes(shape):
    return with_aux(small_scenes(shape))


def arenas(scenes):
    return dict(image=np.concatenate([s.observations for s in scenes]),
                depth=np.concatenate([s.depth for s in scenes]),
                seg=np.concatenate([s.segmentation for s in scenes]))


def expected(ar, ref, fmt):
    """The five frames of the oracle's rows, in the env's format."""
    rows = (("image", "img_row"), ("image", "goal_row"), ("depth", "img_row"), ("seg", "img_row"), ("seg", "goal_row"))
    if fmt == "f32_chw":
        return [unit(ar[a], ref[r]) for a, r in rows]
    return [ar[a][ref[r]] for a, r in rows]


def same(got, want):
    if want.dtype == np.float32:
        return same_bits(got, want)
    return got.dtype == torch.uint8 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want)


def assert_frames(frames, ar, ref, fmt, tag):
    assert len(frames) == 5, tag
    for k, got, want in zip(KEYS, frames, expected(ar, ref, fmt)):
        assert same(got, want), (tag, k)


def compare_five(env_out, o, ar, fmt, tag):
    frames, reward, done, info = env_out
    assert np.array_equal(reward.cpu().numpy().view(np.uint32), o["reward"].view(np.uint32)), tag
    assert np.array_equal(done.cpu().numpy(), o["done"]), tag
    assert np.array_equal(info["state"].cpu().numpy(), o["state"]), tag
    assert np.array_equal(info["img_row"].cpu().numpy(), o["img_row"]), tag
    assert np.array_equal(info["goal_row"].cpu().numpy(), o["goal_row"]), tag
    assert np.array_equal(info["ep_length"].cpu().numpy(), o["ep_length"]), tag
    assert np.array_equal(info["terminal_state"].cpu().numpy(), o["terminal_state"]), tag
    assert np.array_equal(info["truncated"].cpu().numpy().astype(bool), o["truncated"]), tag
    assert np.array_equal(info["ep_return"].cpu().numpy().view(np.uint32), o["ep_return"].view(np.uint32)), tag
    assert_frames(frames, ar, o, fmt, tag)


def frame_shapes(shape, fmt):
    H, W, C = shape
    if fmt == "f32_chw":
        return [(C, H, W), (C, H, W), (1, H, W), (3, H, W), (3, H, W)]
    return [(H, W, C), (H, W, C), (H, W, 1), (H, W, 3), (H, W, 3)]


def make_out(shape, fmt, offset=0, n=N):
    """Caller-owned outputs: the five frames inside one zeroed guard buffer, each `offset`
    elements past a 16-element boundary with at least 16 untouched elements on either side."""
    dtype = torch.float32 if fmt == "f32_chw" else torch.uint8
    shapes = frame_shapes(shape, fmt)
    starts, pos = [], 16
    for s in shapes:
        starts.append(pos + offset)
        pos = (pos + offset + n * int(np.prod(s)) + 15) // 16 * 16 + 16
    buf = torch.zeros(pos, dtype=dtype, device="cuda")
    out = dict(reward=torch.empty(n, dtype=torch.float32, device="cuda"),
               done=torch.empty(n, dtype=torch.bool, device="cuda"),
               state=torch.empty(n, dtype=torch.int32, device="cuda"))
    spans = []
    for k, s, st in zip(KEYS, shapes, starts):
        m = n * int(np.prod(s))
        out[k] = buf[st:st + m].view((n,) + s)
        spans.append((st, st + m))
    return buf, out, spans


def outside_is_zero(buf, spans):
    b = bits(buf) if buf.dtype == torch.float32 else buf.cpu().numpy()
    mask = np.ones(b.shape, dtype=bool)
    for s, e in spans:
        mask[s:e] = False
    return not b[mask].any()


def five(out):
    return tuple(out[k] for k in KEYS)


def poison_of(fmt):
    return -1.0 if fmt == "f32_chw" else 0xAA  # no float observation value: they lie in [0, 1]


def make_env(sc, fmt, n=N, **kw):
    kw.setdefault("max_episode_steps", LIMIT)
    return _vnav().VectorEnv(sc, n, seed=SEED, aux_observations=True, obs_format=fmt, aux_format=fmt, **kw)


# ---- 1. parity over the copy / convert paths ------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape,offset", PATHS)
def test_parity_over_paths(shape, offset, fmt):
    sc = aux_scenes(shape)
    ar = arenas(sc)
    _, acts, steps = reference(LIMIT)
    assert_all_row_cases(LIMIT)
    env = make_env(sc, fmt)
    assert env.aux_format == fmt and env.aux_shapes == tuple(frame_shapes(shape, fmt)[2:])
    buf, out, spans = make_out(shape, fmt, offset)
    for t in range(STEPS):
        ret = env.step(dev(acts[t]), out=out)
        assert all(x is y for x, y in zip(ret[0], five(out)))
        compare_five(ret, steps[t], ar, fmt, (shape, offset, t))
    assert env._reuse_on
    assert outside_is_zero(buf, spans)
    assert env.error_flags() == oe.FLAG_BAD_ACTION


# ---- 2. full-size rows ----------------------------------------------------------------------

# u8 16-B lanes, one-frame trip 512 uint4: 84 x 84 depth 441 (shorter than a trip), image 1323
# (2 trips + 299); 96 x 96 depth 576 (1 trip + 64), image 1728 (3 trips + 192); 64 x 64 depth 256,
# image 768 (1 trip + 256). f32 4-pixel groups, trip 512 groups for 3-channel frames and for the
# one-channel depth plane alike: 84 x 84 = 1764 groups (3 trips + 228), 96 x 96 = 2304 (4 trips +
# 256), 64 x 64 = 1024 (2 trips exactly: the size added for "exact trips"); "shorter than a trip"
# is every shape of PATHS.
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", [84, 96, 64])
def test_full_size_rows(size, fmt):
    vnav = _vnav()
    shape = (size, size, 3)
    sc = [vnav.synthetic_scene(k, grid=8, frame_shape=shape) for k in range(2)]
    for s in sc:  # host copies of the frames, so the expected rows can be gathered
        s.observations = synth_frames(s.synth_id, np.arange(s.n_states), s.frame_shape)
    sc = with_aux(sc)
    ar = arenas(sc)
    n = 8
    env = vnav.VectorEnv(sc, n, seed=314, max_episode_steps=7, aux_observations=True, obs_format=fmt, aux_format=fmt)
    o = oracle_of(sc, n, 314, max_steps=7)
    buf, out, spans = make_out(shape, fmt, n=n)
    rng = np.random.RandomState(2)
    for t in range(30):
        a = rng.randint(0, 4, size=n).astype(np.int32)
        compare_five(env.step(dev(a), out=out), o.step(a), ar, fmt, (size, t))
    assert outside_is_zero(buf, spans)
    assert env.error_flags() == 0


# ---- 3. skips happen, and only where allowed ------------------------------------------------

def same_rows(t):
    """Per output of KEYS: the envs whose arena row at step t is the one of step t - 1 (depth and
    segmentation follow the image row, goal segmentation the goal row)."""
    si, sg = row_changes(LIMIT)[t]
    return (si, sg, si, si, sg)


def poisoned_steps(step_fn, out, ar, fmt, expect_skips, tag):
    """All five outputs are filled with the poison before each of steps 1..STEPS-1 (the contract's
    violation, on purpose: it shows which rows a step wrote). A row whose arena row did not change
    keeps the poison when skips are expected; every other row holds its frame."""
    _, acts, steps = reference(LIMIT)
    p = poison_of(fmt)
    step_fn(acts[0])
    assert_frames(five(out), ar, steps[0], fmt, (tag, 0))
    kept = [0] * 5
    for t in range(1, STEPS):
        for k in KEYS:
            out[k].fill_(p)
        step_fn(acts[t])
        for i, (k, want, same_r) in enumerate(zip(KEYS, expected(ar, steps[t], fmt), same_rows(t))):
            if expect_skips:
                want = want.copy()
                want[same_r] = p
                kept[i] += int(same_r.sum())
            assert same(out[k], want), (tag, k, t)
    return kept


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape,offset", [PATHS[0], PATHS[2]])
def test_skips_happen_only_where_allowed(shape, offset, fmt):
    sc = aux_scenes(shape)
    ar = arenas(sc)
    if fmt == "u8_hwc":
        for a in ar.values():
            assert not (a.reshape(len(a), -1) == 0xAA).all(axis=1).any()
    _, acts, steps = reference(LIMIT)
    assert_all_row_cases(LIMIT, start=1)
    p = poison_of(fmt)
    # only the rows the oracle says change are poisoned: still exact (every changed row is written)
    env = make_env(sc, fmt)
    buf, out, spans = make_out(shape, fmt, offset)
    compare_five(env.step(dev(acts[0]), out=out), steps[0], ar, fmt, 0)
    for t in range(1, STEPS):
        for k, same_r in zip(KEYS, same_rows(t)):
            out[k][dev(~same_r)] = p
        compare_five(env.step(dev(acts[t]), out=out), steps[t], ar, fmt, ("changed rows poisoned", t))
    assert outside_is_zero(buf, spans)
    # everything is poisoned: exactly the rows whose arena row did not change keep the poison
    env = make_env(sc, fmt)
    buf, out, spans = make_out(shape, fmt, offset)
    kept = poisoned_steps(lambda a: env.step(dev(a), out=out), out, ar, fmt, True, (shape, offset))
    assert all(k > 0 for k in kept), kept
    assert outside_is_zero(buf, spans)
    # reuse_outputs=False: every row of all five is rewritten on every step
    env = make_env(sc, fmt, reuse_outputs=False)
    _, out, _ = make_out(shape, fmt, offset)
    poisoned_steps(lambda a: env.step(dev(a), out=out), out, ar, fmt, False, "reuse_outputs=False")
    assert not env._reuse_on


# ---- 4. full writes where due ---------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_new_rebound_and_swapped_buffers_get_a_full_write(fmt):
    shape = (4, 8, 3)
    sc = aux_scenes(shape)
    ar = arenas(sc)
    _, acts, steps = reference(LIMIT)
    p = poison_of(fmt)
    env = make_env(sc, fmt)
    _, A, _ = make_out(shape, fmt)

    def fill(out):
        for k in KEYS:
            out[k].fill_(p)

    t = 0
    for _ in range(4):
        compare_five(env.step(dev(acts[t]), out=A), steps[t], ar, fmt, ("A", t))
        t += 1
    _, B, _ = make_out(shape, fmt)  # a new out dict
    fill(B)
    compare_five(env.step(dev(acts[t]), out=B), steps[t], ar, fmt, ("B", t))
    t += 1
    fill(A)  # the old one again, overwritten meanwhile
    compare_five(env.step(dev(acts[t]), out=A), steps[t], ar, fmt, ("A again", t))
    t += 1
    compare_five(env.step(dev(acts[t]), out=A), steps[t], ar, fmt, ("A again", t))
    t += 1
    # segmentation and goal segmentation swap roles: the same five tensors, other keys
    S = dict(A, segmentation=A["goal_segmentation"], goal_segmentation=A["segmentation"])
    ret = env.step(dev(acts[t]), out=S)
    assert ret[0][3] is A["goal_segmentation"] and ret[0][4] is A["segmentation"]
    compare_five(ret, steps[t], ar, fmt, ("swapped", t))
    t += 1
    compare_five(env.step(dev(acts[t]), out=S), steps[t], ar, fmt, ("swapped", t))
    t += 1
    compare_five(env.step(dev(acts[t]), out=A), steps[t], ar, fmt, ("swapped back", t))
    # observe(out=5-tuple) into poisoned rows whose records match: only the armed write fills them
    fill(A)
    frames = env.observe(out=five(A))
    assert all(x is y for x, y in zip(frames, five(A)))
    assert_frames(frames, ar, steps[t], fmt, "observe after poison")
    t += 1
    # and the step after the full writes skips again
    fill(A)
    env.step(dev(acts[t]), out=A)
    kept = 0
    for k, want, same_r in zip(KEYS, expected(ar, steps[t], fmt), same_rows(t)):
        want = want.copy()
        want[same_r] = p
        kept += int(same_r.sum())
        assert same(A[k], want), k
    assert kept > 0


# ---- 5. the C level: a NULL aux pointer, no aux arena -----------------------------------------

def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def obs_set(out, fmt, null=()):
    from vnav import _lib
    return _lib.ObsSet(*[None if k in null else out[k].data_ptr() for k in KEYS],
                       _lib.OBS_F32_CHW if fmt == "f32_chw" else _lib.OBS_U8_HWC)


def raw_step_aux(env, a, out, fmt, null=()):
    o = obs_set(out, fmt, null)
    rc = env.lib.vn_step_aux(env._ctx, ptr(a), ctypes.byref(o), ptr(out["reward"]), ptr(out["done"]), ptr(out["state"]),
                             env._stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("fmt", FORMATS)
def test_null_aux_pointer(fmt):
    shape = (4, 8, 3)
    sc = aux_scenes(shape)
    ar = arenas(sc)
    _, acts, steps = reference(LIMIT)
    p = poison_of(fmt)
    env = make_env(sc, fmt)
    _, out, _ = make_out(shape, fmt)
    t = 0
    for _ in range(3):
        compare_five(env.step(dev(acts[t]), out=out), steps[t], ar, fmt, t)
        t += 1
    # goal rows change where episodes end: the shared trajectory truncates 34 envs at step 10
    for null, t0 in (("depth", 3), ("segmentation", 5), ("goal_segmentation", 9)):
        while t < t0:
            compare_five(env.step(dev(acts[t]), out=out), steps[t], ar, fmt, t)
            t += 1
        # the rows the NULL frame's record and buffer still describe are two steps old at the
        # five-pointer call below: some env must need a rewrite there, some must not
        r = "goal_row" if null == "goal_segmentation" else "img_row"
        moved = steps[t + 1][r] != steps[t - 1][r]
        assert moved.any() and not moved.all()
        assert env.lib.vn_set_output_reuse(env._ctx, 1) == 0  # the four others were poisoned: full write
        before = out[null].clone()
        for k in KEYS:
            if k != null:
                out[k].fill_(p)
        assert raw_step_aux(env, dev(acts[t]), out, fmt, null=(null,)) == 0
        assert np.array_equal(bits(out[null]) if fmt == "f32_chw" else out[null].cpu().numpy(),
                              bits(before) if fmt == "f32_chw" else before.cpu().numpy()), null
        for k, want in zip(KEYS, expected(ar, steps[t], fmt)):
            if k != null:
                assert same(out[k], want), (null, k)
        assert np.array_equal(out["state"].cpu().numpy(), steps[t]["state"])
        t += 1
        # all five again, reuse on and not re-armed: the frame left out is brought up to date
        assert raw_step_aux(env, dev(acts[t]), out, fmt) == 0
        assert_frames(five(out), ar, steps[t], fmt, ("after NULL", null))
        t += 1
    # image or goal NULL is refused
    for null in KEYS[:2]:
        before = [out[k].clone() for k in KEYS]
        assert raw_step_aux(env, dev(acts[t]), out, fmt, null=(null,)) == -1
        assert all(torch.equal(x, out[k]) for x, k in zip(before, KEYS))
    compare_five(env.step(dev(acts[t]), out=out), steps[t], ar, fmt, "step after the refusals")


def test_no_aux_arena_is_einval_and_launches_nothing():
    from vnav import _lib
    vnav = _vnav()
    shape = (4, 8, 3)
    env = vnav.VectorEnv(small_scenes(shape), N, seed=SEED, max_episode_steps=LIMIT)  # no depth / segmentation
    assert env.aux_arena is None
    _, out, _ = make_out(shape, "u8_hwc")
    for k in KEYS:
        out[k].fill_(0xAA)
    out["state"].fill_(-7)
    state = env.get_state().clone()
    a = dev(reference(LIMIT)[1][0])
    assert raw_step_aux(env, a, out, "u8_hwc") == -1
    assert "aux arena" in _lib.last_error()
    o = obs_set(out, "u8_hwc")
    assert env.lib.vn_observe_aux(env._ctx, ctypes.byref(o), None, env._stream()) == -1
    torch.cuda.synchronize()
    assert all((out[k] == 0xAA).all().item() for k in KEYS) and (out["state"] == -7).all().item()
    assert torch.equal(env.get_state(), state)
    # cleared arenas answer the same
    env2 = make_env(aux_scenes(shape), "u8_hwc")
    assert env2.lib.vn_set_aux_arena(env2._ctx, None, 0, None, 0) == 0
    assert raw_step_aux(env2, a, out, "u8_hwc") == -1
    assert all((out[k] == 0xAA).all().item() for k in KEYS)


# ---- 6. two-frame and five-frame calls in turn ------------------------------------------------

def test_interleaved_with_two_frame_steps():
    """vn_step (even steps) and vn_step_aux (odd steps) into the same image / goal buffers, reuse
    on. The aux buffers are poisoned before every five-frame call after the first: the rows whose
    arena row is the one of the previous five-frame call keep the poison, so the aux records
    survived the two-frame call in between; every other row is exact."""
    shape = (4, 8, 3)
    fmt = "u8_hwc"
    sc = aux_scenes(shape)
    ar = arenas(sc)
    _, acts, steps = reference(LIMIT)
    env = make_env(sc, fmt, reuse_outputs=False)
    _, out, _ = make_out(shape, fmt)
    assert env.lib.vn_set_output_reuse(env._ctx, 1) == 0
    kept = 0
    for t in range(30):
        a = dev(acts[t])
        want = expected(ar, steps[t], fmt)
        if t % 2 == 0:
            aux_before = [out[k].clone() for k in KEYS[2:]]
            assert env.lib.vn_step(env._ctx, ptr(a), ptr(out["image"]), ptr(out["goal"]), ptr(out["reward"]),
                                   ptr(out["done"]), ptr(out["state"]), env._stream()) == 0
            torch.cuda.synchronize()
            assert all(torch.equal(x, out[k]) for x, k in zip(aux_before, KEYS[2:])), t
        else:
            if t > 1:
                for k in KEYS[2:]:
                    out[k].fill_(0xAA)
                si = steps[t]["img_row"] == steps[t - 2]["img_row"]
                sg = steps[t]["goal_row"] == steps[t - 2]["goal_row"]
                for i, same_r in ((2, si), (3, si), (4, sg)):
                    want[i] = want[i].copy()
                    want[i][same_r] = 0xAA
                    kept += int(same_r.sum())
            assert raw_step_aux(env, a, out, fmt) == 0
            for k, w in zip(KEYS[2:], want[2:]):
                assert same(out[k], w), (t, k)
        assert same(out["image"], want[0]) and same(out["goal"], want[1]), t
        assert np.array_equal(out["state"].cpu().numpy(), steps[t]["state"]), t
    assert kept > 0


# ---- 7. one storage, two formats, on the aux rows ---------------------------------------------

def test_format_aliasing_on_aux_rows():
    """Float buffers and uint8 views of the same storage (same data_ptr) for all five outputs,
    reuse on, armed once, no reset: the u8 and the f32 form of vn_step_aux in turn, with an invalid
    action (a blocked move: the emitted rows never change). Env 0's rows have the same address and
    arena row in both formats, so only the records' format bit makes each call write them."""
    shape = (4, 8, 3)
    n = 5
    sc = aux_scenes(shape)
    ar = arenas(sc)
    env = make_env(sc, "u8_hwc", n=n, max_episode_steps=900, reuse_outputs=False)
    o = oracle_of(sc, n, SEED, max_steps=900)
    rows = o.observe()
    f = {k: torch.zeros((n,) + s, dtype=torch.float32, device="cuda")
         for k, s in zip(KEYS, frame_shapes(shape, "f32_chw"))}
    u = {k: f[k].view(-1).view(torch.uint8)[:n * int(np.prod(s))].view((n,) + s)
         for k, s in zip(KEYS, frame_shapes(shape, "u8_hwc"))}
    assert all(u[k].data_ptr() == f[k].data_ptr() for k in KEYS)
    scal = dict(reward=torch.empty(n, dtype=torch.float32, device="cuda"),
                done=torch.empty(n, dtype=torch.uint8, device="cuda"),
                state=torch.empty(n, dtype=torch.int32, device="cuda"))
    blocked = torch.full((n,), -1, dtype=torch.int32, device="cuda")

    def call(fmt):
        out = dict(scal, **(f if fmt == "f32_chw" else u))
        assert raw_step_aux(env, blocked, out, fmt) == 0
        assert not scal["done"].any().item()
        assert_frames(five(out), ar, rows, fmt, fmt)

    assert env.lib.vn_set_output_reuse(env._ctx, 1) == 0
    for fmt in ("u8_hwc", "f32_chw", "u8_hwc", "f32_chw", "f32_chw", "u8_hwc", "u8_hwc", "f32_chw"):
        call(fmt)
    # the float records are in place again: a second float call skips every (unchanged) row
    for k in KEYS:
        f[k].fill_(-1.0)
    assert raw_step_aux(env, blocked, dict(scal, **f), "f32_chw") == 0
    assert all((f[k] == -1.0).all().item() for k in KEYS)
    assert env.error_flags() == oe.FLAG_BAD_ACTION


# ---- 8. graph replay --------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_graph_replay(fmt):
    """One captured step(out=five buffers), replayed 20 times against the oracle: nothing is
    allocated by the step, and the records that decide the skips live on the device."""
    shape = (4, 8, 3)
    sc = aux_scenes(shape)
    ar = arenas(sc)
    _, acts, steps = reference(LIMIT)
    env = make_env(sc, fmt)
    buf, out, spans = make_out(shape, fmt)
    static = torch.zeros(N, dtype=torch.int32, device="cuda")
    t = 0
    for _ in range(4):
        static.copy_(dev(acts[t]))
        compare_five(env.step(static, out=out), steps[t], ar, fmt, ("eager", t))
        t += 1
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = env.step(static, out=out)
    assert all(x is y for x, y in zip(captured[0], five(out)))
    for k in range(20):
        static.copy_(dev(acts[t]))
        g.replay()
        compare_five(captured, steps[t], ar, fmt, ("replay", k))
        t += 1
    assert outside_is_zero(buf, spans)
    del g


# ---- 9. A/B against the former form -----------------------------------------------------------

def ab_steps(monkeypatch, scenes, n, steps, actions, **kw):
    """Route a: VN_AUX_OBS_GATHER=1 (step + three vn_gather_rows, fresh tensors); route b: the
    fused step into five caller-owned buffers. The same seed and actions; all five frames, reward
    and done bitwise equal at every step."""
    vnav = _vnav()
    envs = [vnav.VectorEnv(scenes, n, seed=77, aux_observations=True, **kw) for _ in range(2)]
    _, out, _ = make_out(tuple(scenes[0].frame_shape), "u8_hwc", n=n)
    for t in range(steps):
        a = dev(actions(t))
        monkeypatch.setenv("VN_AUX_OBS_GATHER", "1")
        fa, ra, da, ia = envs[0].step(a)
        monkeypatch.delenv("VN_AUX_OBS_GATHER")
        fb, rb, db, ib = envs[1].step(a, out=out)
        assert all(x is y for x, y in zip(fb, five(out)))
        assert not any(x is y for x, y in zip(fa, five(out)))
        assert len(fa) == 5 and all(torch.equal(x, y) for x, y in zip(fa, fb)), t
        assert torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(ia["state"], ib["state"]), t
    return envs


def test_ab_against_step_plus_gathers(monkeypatch):
    _, acts, _ = reference(LIMIT)
    envs = ab_steps(monkeypatch, aux_scenes((6, 10, 3)), N, STEPS, lambda t: acts[t], max_episode_steps=LIMIT)
    assert all(e.error_flags() == oe.FLAG_BAD_ACTION for e in envs)


def test_ab_on_an_oriented_scene_with_companion_frames(monkeypatch):
    """Companion frames as the second output and depth / segmentation on one scene: goal_row is the
    companion row there, and both routes read the aux arenas at it."""
    vnav = _vnav()
    rng = np.random.RandomState(3)
    maze = np.ones((3, 3), dtype=bool)
    mk = lambda c: rng.randint(0, 256, size=(3, 3, 4, 4, 8, c)).astype(np.uint8)  # noqa: E731
    scene = vnav.oriented_scene(maze, mk(3), tp_observations=mk(3), depths=mk(1), segmentations=mk(3))
    assert scene.companion is not None and scene.depth is not None
    ab_steps(monkeypatch, [scene], 5, 30, lambda t: rng.randint(0, 4, size=5).astype(np.int32), max_episode_steps=6)


# ---- 10. refusals, each before any launch -----------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_bad_buffers_are_refused(fmt):
    vnav = _vnav()
    shape = (4, 8, 3)
    sc = aux_scenes(shape)
    n = 8
    env = make_env(sc, fmt, n=n)
    _, ok, _ = make_out(shape, fmt, n=n)
    a = torch.zeros(n, dtype=torch.int32, device="cuda")
    env.step(a, out=ok)
    state = env.get_state().clone()
    snapshot = [ok[k].clone() for k in KEYS]
    dtype = torch.float32 if fmt == "f32_chw" else torch.uint8
    wrong = torch.uint8 if fmt == "f32_chw" else torch.float32
    shapes = dict(zip(KEYS, frame_shapes(shape, fmt)))
    numel = {k: n * int(np.prod(s)) for k, s in shapes.items()}
    bad = []
    for k in KEYS[2:]:
        bad += [{k: torch.zeros((n,) + shapes[k], dtype=wrong, device="cuda")},            # wrong dtype
                {k: torch.zeros(numel[k] - 1, dtype=dtype, device="cuda")},                # wrong element count
                {k: torch.zeros(numel[k] + 4, dtype=dtype, device="cuda")},
                {k: torch.zeros((n, 2 * numel[k] // n), dtype=dtype, device="cuda")[:, ::2]},  # non-contiguous
                {k: torch.zeros((n,) + shapes[k], dtype=dtype)}]                           # wrong device
    # two overlapping buffers: the same tensor twice, and two windows of one buffer
    big = torch.zeros(2 * numel["segmentation"], dtype=dtype, device="cuda")
    bad += [dict(goal_segmentation=ok["segmentation"]),
            dict(segmentation=big[:numel["segmentation"]].view((n,) + shapes["segmentation"]),
                 goal_segmentation=big[8:8 + numel["segmentation"]].view((n,) + shapes["segmentation"])),
            dict(depth=ok["image"].view(-1)[:numel["depth"]].view((n,) + shapes["depth"]))]
    # one or two of the three aux keys
    bad += [dict(depth=None), dict(segmentation=None, goal_segmentation=None), dict(depth=None, segmentation=None)]
    for repl in bad:
        out = dict(ok, **repl)
        with pytest.raises(ValueError):
            env.step(a, out=out)
        with pytest.raises(ValueError):
            env.observe(out=five(out))
    one_key = {k: v for k, v in ok.items() if k not in ("segmentation", "goal_segmentation")}
    with pytest.raises(ValueError):
        env.step(a, out=one_key)
    with pytest.raises(ValueError):
        env.observe(out=five(ok)[:3])
    torch.cuda.synchronize()
    assert torch.equal(env.get_state(), state)
    assert all(torch.equal(x, ok[k]) for x, k in zip(snapshot, KEYS))
    # the formats: float aux frames only next to float image frames, in the constructor
    with pytest.raises(ValueError):
        vnav.VectorEnv(sc, n, aux_observations=True, obs_format="u8_hwc", aux_format="f32_chw")
    with pytest.raises(ValueError):
        vnav.make("AuxiliaryGraph-v0", sc, n, aux_format="f32_chw")
    assert env.error_flags() == 0
    # and the env still steps into the good buffers
    env.step(a, out=ok)


# ---- 11. API shape ----------------------------------------------------------------------------

def test_step_returns_the_callers_tensors():
    shape = (4, 8, 3)
    sc = aux_scenes(shape)
    env = _vnav().make("AuxiliaryGraph-v0", sc, N, seed=SEED, max_episode_steps=LIMIT)
    _, out, _ = make_out(shape, "u8_hwc")
    a = dev(reference(LIMIT)[1][0])
    for _ in range(2):  # the validating call and the cached-pointer call
        frames, reward, done, info = env.step(a, out=out)
        assert frames[2] is out["depth"]
        assert all(x is y for x, y in zip(frames, five(out)))
        assert reward is out["reward"] and done is out["done"] and info["state"] is out["state"]


def test_float_aux_frames_from_reset_observe_and_step():
    shape = (6, 10, 3)
    H, W, _ = shape
    sc = aux_scenes(shape)
    ar = arenas(sc)
    first, acts, steps = reference(LIMIT)
    env = _vnav().make("AuxiliaryGraph-v0", sc, N, seed=SEED, max_episode_steps=LIMIT, obs_format="f32_chw",
                       aux_format="f32_chw")

    def check(frames, ref, tag):
        assert [tuple(x.shape) for x in frames] == [(N, 3, H, W), (N, 3, H, W), (N, 1, H, W), (N, 3, H, W), (N, 3, H, W)]
        assert all(x.dtype == torch.float32 and x.is_contiguous() and x.device.type == "cuda" for x in frames)
        assert_frames(frames, ar, ref, "f32_chw", tag)

    check(env.observe(), first, "observe")
    for t in range(6):  # fresh tensors, reuse disarmed
        ret = env.step(dev(acts[t]))
        assert not env._reuse_on
        compare_five(ret, steps[t], ar, "f32_chw", ("fresh", t))
        check(ret[0], steps[t], t)
    # image / goal buffers without aux buffers: the three are fresh float tensors, all five exact
    _, out, _ = make_out(shape, "f32_chw")
    two = {k: v for k, v in out.items() if k not in KEYS[2:]}
    for t in range(6, 12):
        ret = env.step(dev(acts[t]), out=two)
        assert ret[0][0] is out["image"] and ret[0][2] is not out["depth"]
        compare_five(ret, steps[t], ar, "f32_chw", ("two buffers", t))
    frames = env.reset()
    rows = dict(img_row=env._info["img_row"].cpu().numpy(), goal_row=env._info["goal_row"].cpu().numpy())
    check(frames, rows, "reset")
    # the u8 default of the registry id, through the fused path too
    u8 = _vnav().make("AuxiliaryGraph-v0", sc, N, seed=SEED, max_episode_steps=LIMIT)
    assert u8.aux_format == "u8_hwc" and u8._aux_fused
    assert_frames(u8.observe(), ar, first, "u8_hwc", "u8 observe")
    compare_five(u8.step(dev(acts[0])), steps[0], ar, "u8_hwc", "u8 fresh")
