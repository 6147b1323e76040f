"""The episode sampler (vn_nav_sample_episodes) bit for bit against tests/episodes_ref.py, and the
per-episode log of the nav step (vn_nav_set_episode_log) against the steps' own outputs, on the
GPU."""
import ctypes

import numpy as np
import pytest
import torch

import episodes_ref as er
import nav_ref as nr

pytestmark = pytest.mark.gpu

BUCKETS = ((1, 3), (4, 8), (9, None))
COUNTS = (1, 63, 64, 65, 257, 1000)
SENT = 0x5A


def _vnav():
    import vnav
    return vnav


def dev(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int32), device="cuda")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def scenes():
    return nr.shared_scenes()


@pytest.fixture(scope="module")
def env3(scenes):
    env = _vnav().VectorEnv(scenes, 4, seed=1, nav_info=True)
    yield env
    env.close()


@pytest.fixture(scope="module")
def env12():
    env = _vnav().VectorEnv([_vnav().synthetic_scene(0, grid=12, frame_shape=nr.FRAME)], 4, seed=1, nav_info=True)
    yield env
    env.close()


@pytest.fixture(scope="module")
def geos(scenes):
    return [nr.geodesic(s.graph) for s in scenes], nr.geodesic(_vnav().synthetic_scene(0, grid=12).graph)


def check_draws(env, k, geo, lo, hi, seed, salt, counts=COUNTS):
    total = None
    for count in counts:
        pairs, dist, total = env.sample_episodes(k, count, lo, hi, seed=seed, salt=salt)
        want = er.sample_episodes(geo, lo, hi, count, seed, salt)
        assert pairs.dtype == torch.int32 and dist.dtype == torch.int32 and pairs.shape == (count, 2)
        assert total == want[2], (count, total)
        assert same_bits(pairs.cpu().numpy(), want[0]), count
        assert same_bits(dist.cpu().numpy(), want[1]), count
    return total


# ---- sampler ----------------------------------------------------------------------------------
CASES3 = [(0, 0, 224), (0, 1, 238), (1, 0, 1640), (1, 1, 3972), (1, 2, 2760), (2, 0, 17), (2, 1, 1)]


@pytest.mark.parametrize("k,b,total", CASES3)
def test_sampler_bitwise_shared_scenes(env3, geos, k, b, total):
    """n = 22, 92 and 7: rows of 44, 184 and 14 bytes (2-byte aligned only), ragged last chunks."""
    lo, hi = BUCKETS[b]
    assert check_draws(env3, k, geos[0][k], lo, hi, seed=7, salt=k * 65536 + b) == total


@pytest.mark.parametrize("b,total", [(0, 7648), (1, 27768), (2, None)])
def test_sampler_bitwise_376_states(env12, geos, b, total):
    """376 states = 5 chunks of 64 and one of 56, more than one state per counting thread."""
    lo, hi = BUCKETS[b]
    got = check_draws(env12, 0, geos[1], lo, hi, seed=2**40 + 5, salt=b)
    assert total is None or got == total


def test_sampler_whole_table_range(env3, geos):
    """dist_hi beyond the clamp, and a one-distance range."""
    check_draws(env3, 1, geos[0][1], 1, 10**6, seed=1, salt=1, counts=(65,))
    check_draws(env3, 1, geos[0][1], 5, 5, seed=1, salt=1, counts=(65,))


def test_single_pair_bucket(env3):
    pairs, dist, total = env3.sample_episodes(2, 257, 4, 8, seed=3, salt=9)
    assert total == 1
    assert (pairs.cpu().numpy() == np.array([0, 4])).all() and (dist.cpu().numpy() == 4).all()


def test_no_unreachable_pair(env3, geos):
    pairs, dist, total = env3.sample_episodes(2, 1000, 1, 3, seed=4, salt=0)
    p = pairs.cpu().numpy()
    d = geos[0][2][p[:, 1], p[:, 0]]
    assert total == 17 and (d >= 1).all() and (d <= 3).all() and same_bits(dist.cpu().numpy(), d.astype(np.int32))
    assert len(np.unique(p[:, 1] * 7 + p[:, 0])) == 17  # 1000 draws reach all 17 pairs


def raw_sample(env, scene, lo, hi, count, out, dist, total, seed=1, salt=0):
    from vnav import _lib
    return env.lib.vn_nav_sample_episodes(env._ctx, scene, lo, hi, count, ctypes.c_uint64(seed), ctypes.c_uint32(salt),
                                          _lib.ptr(out), _lib.ptr(dist),
                                          ctypes.byref(total) if total is not None else None, env._stream())


def test_empty_bucket_keeps_the_sentinel(env3):
    out = torch.full((64, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dist = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    total = ctypes.c_int64(-7)
    assert raw_sample(env3, 0, 9, 32767, 64, out, dist, total) == 0
    torch.cuda.synchronize()
    assert total.value == 0 and (out == 0x5A5A5A5A).all() and (dist == 0x5A5A5A5A).all()


def test_seed_salt_and_repeat(env3):
    base = env3.sample_episodes(1, 64, 1, 3, seed=3, salt=7)[0]
    assert torch.equal(env3.sample_episodes(1, 64, 1, 3, seed=3, salt=7)[0], base)
    assert not torch.equal(env3.sample_episodes(1, 64, 1, 3, seed=3, salt=8)[0], base)
    assert not torch.equal(env3.sample_episodes(1, 64, 1, 3, seed=4, salt=7)[0], base)
    assert not torch.equal(env3.sample_episodes(1, 64, 1, 3, seed=3 + 2**32, salt=7)[0], base)


def test_dist_output_is_optional(env3, geos):
    out = torch.full((65, 2), -1, dtype=torch.int32, device="cuda")
    total = ctypes.c_int64(0)
    assert raw_sample(env3, 1, 9, 32767, 65, out, None, total, seed=7, salt=65538) == 0
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), er.sample_episodes(geos[0][1], 9, None, 65, 7, 65538)[0])


def test_sampler_refusals(env3, scenes):
    out = torch.full((8, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dist = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    total = ctypes.c_int64(-7)
    bad = [dict(scene=-1), dict(scene=3), dict(lo=0), dict(lo=-1), dict(lo=5, hi=4), dict(count=0), dict(count=-3),
           dict(out=None), dict(total=None)]
    for kw in bad:
        a = dict(scene=1, lo=1, hi=3, count=8, out=out, dist=dist, total=total)
        a.update(kw)
        assert raw_sample(env3, a["scene"], a["lo"], a["hi"], a["count"], a["out"], a["dist"], a["total"]) == -1, kw
    torch.cuda.synchronize()
    assert total.value == -7 and (out == 0x5A5A5A5A).all() and (dist == 0x5A5A5A5A).all()
    for kw in (dict(min_distance=0), dict(min_distance=4, max_distance=3)):
        with pytest.raises(_vnav().VnavError):
            env3.sample_episodes(1, 8, **kw)
    with pytest.raises(_vnav().VnavError):
        env3.sample_episodes(1, 0)
    off = _vnav().VectorEnv(scenes, 4, seed=1)
    assert raw_sample(off, 1, 1, 3, 8, out, dist, total) == -4  # VN_ESTATE before vn_nav_enable
    log = _lib_log(3, *[out] * 7)
    assert off.lib.vn_nav_set_episode_log(off._ctx, ctypes.byref(log)) == -4
    with pytest.raises(_vnav().VnavError):
        off.sample_episodes(1, 8)
    with pytest.raises(_vnav().VnavError):
        off.set_episode_log(3, torch.zeros(4, dtype=torch.int32))
    off.close()


def _lib_log(capacity, *tensors):
    from vnav import _lib
    return _lib.EpisodeLog(capacity, *[t.data_ptr() if t is not None else None for t in tensors])


def test_log_refusals(env3):
    E = env3.num_envs
    t = [torch.zeros(3 * E, dtype=torch.int32, device="cuda") for _ in range(7)]
    assert env3.lib.vn_nav_set_episode_log(env3._ctx, ctypes.byref(_lib_log(0, *t))) == -1
    assert env3.lib.vn_nav_set_episode_log(env3._ctx, ctypes.byref(_lib_log(-2, *t))) == -1
    for i in range(7):
        u = list(t)
        u[i] = None
        assert env3.lib.vn_nav_set_episode_log(env3._ctx, ctypes.byref(_lib_log(3, *u))) == -1, i
    for cap, want in ((0, [0] * E), (3, [0] * (E - 1)), (3, [4] + [0] * (E - 1)), (3, [-1] + [0] * (E - 1))):
        with pytest.raises(ValueError):
            env3.set_episode_log(cap, want)
    assert env3.episode_log is None
    assert env3.set_episode_log(None) is None


# ---- log --------------------------------------------------------------------------------------
E, LIMIT, STEPS, CAP = 37, 6, 200, 3
NAV = ("distance_to_goal", "optimal_action", "optimal_mask", "success", "spl", "start_distance")
INFO = ("ep_return", "ep_length", "terminal_state", "truncated", "img_row", "goal_row")
LOGK = ("success", "length", "start_distance", "spl", "ep_return")
WANT = np.arange(E) % 4


def walk_actions(steps=STEPS):
    rng = np.random.RandomState(0)
    return [rng.randint(0, 4, E).astype(np.int32) for _ in range(steps)]


def make_log_env(scenes):
    """37 envs over the three scenes (env e on scene e mod 3), a schedule of 8 sampled pairs per
    env, time limit 6."""
    env = _vnav().VectorEnv(scenes, E, seed=3, max_episode_steps=LIMIT, nav_info=True)
    draws = [env.sample_episodes(k, 8 * E, 1, None, seed=21, salt=k)[0].cpu().numpy() for k in range(3)]
    sched = np.stack([draws[e % 3][8 * e:8 * e + 8] for e in range(E)])
    env.set_schedule(sched)
    return env, sched


def fill_sentinel(log):
    for k in LOGK:
        getattr(log, k).view(torch.uint8).fill_(SENT)


def snap_log(log):
    return dict({k: getattr(log, k).cpu().numpy().copy() for k in LOGK}, count=log.count.cpu().numpy().copy())


def run_log(scenes, route, log_on, actions):
    from vnav import _lib
    env, sched = make_log_env(scenes)
    log = None
    if log_on:
        log = env.set_episode_log(CAP, WANT)
        fill_sentinel(log)
    env.reset()
    st0 = env.get_state().cpu().numpy()
    assert (st0[1] == sched[:, 0, 0]).all() and (st0[2] == sched[:, 0, 1]).all()
    out = None
    if route == "out":
        H, W, C = env.frame_shape
        out = dict(image=torch.zeros((E, H, W, C), dtype=torch.uint8, device="cuda"),
                   goal=torch.zeros((E, H, W, C), dtype=torch.uint8, device="cuda"),
                   reward=torch.zeros(E, dtype=torch.float32, device="cuda"),
                   done=torch.zeros(E, dtype=torch.bool, device="cuda"),
                   state=torch.zeros(E, dtype=torch.int32, device="cuda"))
    if route == "a2c":
        pol = torch.zeros((E, 8), dtype=torch.float32, device="cuda")
        act = torch.zeros(E, dtype=torch.int32, device="cuda")
        s = _lib.A2CStep()
        s.policy_out, s.num_actions, s.seed, s.counter_base_dev = pol.data_ptr(), 4, 99, None
        s.actions = act.data_ptr()
        reward = torch.zeros(E, dtype=torch.float32, device="cuda")
        done = torch.zeros(E, dtype=torch.bool, device="cuda")
        state = torch.zeros(E, dtype=torch.int32, device="cuda")
    steps = []
    for t, a in enumerate(actions):
        if route == "a2c":
            lg = np.zeros((E, 8), dtype=np.float32)
            lg[np.arange(E), a] = 1e4
            pol.copy_(torch.as_tensor(lg))
            s.counter = t
            env.step_a2c(s, reward, done, state)
            frames, info = (), dict(env._info)
            r, d, info["state"] = reward, done, state
        else:
            frames, r, d, info = env.step(dev(a), **(dict(out=out) if out is not None else {}))
        one = dict(reward=r.clone(), done=d.clone(), state=info["state"].clone(), table=env.get_state().clone())
        for i, f in enumerate(frames):
            one["frame%d" % i] = f.clone()
        for k in INFO + NAV:
            one[k] = info[k].clone()
        steps.append(one)
    rec = {k: torch.stack([s_[k] for s_ in steps]).cpu().numpy() for k in steps[0]}
    rec["stats"] = env.nav_episode_stats().cpu().numpy()
    rec["flags"] = env.error_flags()
    return env, log, rec


@pytest.fixture(scope="module")
def log_off(scenes):
    out = {}
    for route in ("step", "out", "a2c"):
        env, _, rec = run_log(scenes, route, False, walk_actions())
        env.close()
        out[route] = rec
    return out


@pytest.mark.parametrize("route", ["step", "out", "a2c"])
def test_log_holds_the_steps_own_values(scenes, log_off, route):
    env, log, rec = run_log(scenes, route, True, walk_actions())
    got = snap_log(log)
    # every other output of every step is bitwise what it is with the log off
    off = log_off[route]
    assert set(rec) == set(off)
    for k in off:
        assert same_bits(rec[k], off[k]) if k != "flags" else rec[k] == off[k] == 0, (route, k)
    # the log against the rule, driven by what each step itself reported
    ref = er.EpisodeLogRef(CAP, WANT)
    for t in range(STEPS):
        ref.step(rec["done"][t], rec["success"][t], rec["spl"][t], rec["start_distance"][t], rec["ep_length"][t],
                 rec["ep_return"][t])
    dones = rec["done"].sum(axis=0)
    assert same_bits(got["count"].astype(np.int64), dones.astype(np.int64)) and (got["count"] == ref.count).all()
    assert (np.minimum(got["count"], WANT) == np.minimum(dones, WANT)).all()  # recorded = min(dones, want)
    assert (np.minimum(got["count"], WANT) == ref.written.sum(axis=0)).all()
    assert dones.min() >= CAP  # every env fills every slot it wants: 200 steps, episodes of <= 6
    for k in LOGK:
        g, w = got[k], getattr(ref, k)
        assert g.dtype == w.dtype and g.shape == (CAP, E)
        assert same_bits(g[ref.written], w[ref.written]), (route, k)
        # unwanted slots still hold the sentinel
        assert (g[~ref.written].view(np.uint8) == SENT).all(), (route, k)
    assert ref.written.sum() == WANT.sum() and (~ref.written).sum() > 0
    # not vacuous: successes with SPL 1 and below 1, and time-outs, are all in the log
    ok = got["success"][ref.written] == 1
    spl = got["spl"][ref.written]
    assert ok.sum() >= 3 and (~ok).sum() >= 10 and (spl[ok] < 1).any() and (spl[ok] == 1).any()
    assert (got["length"][ref.written][~ok] == LIMIT).all()
    # switched off: nothing is written any more
    env.set_episode_log(None)
    fill_sentinel(log)
    for a in walk_actions(12):
        env.step(dev(a))
    after = snap_log(log)
    assert same_bits(after["count"], got["count"])
    assert all((after[k].view(np.uint8) == SENT).all() for k in LOGK)
    env.close()


def test_log_return_without_an_info_buffer(scenes, log_off):
    """No ep_return info buffer set: the nav state's stand-in carries the return."""
    from vnav import _lib
    env, _ = make_log_env(scenes)
    i = env._info
    _lib.check(env.lib.vn_set_info_buffers(env._ctx, None, _lib.ptr(i["ep_length"]), _lib.ptr(i["terminal_state"]),
                                           _lib.ptr(i["truncated"]), _lib.ptr(i["img_row"]), _lib.ptr(i["goal_row"])),
               "vn_set_info_buffers")
    log = env.set_episode_log(CAP, WANT)
    env.reset()
    ref = er.EpisodeLogRef(CAP, WANT)
    off = log_off["step"]
    for t, a in enumerate(walk_actions(60)):
        env.step(dev(a), gather=False)
        ref.step(off["done"][t], off["success"][t], off["spl"][t], off["start_distance"][t], off["ep_length"][t],
                 off["ep_return"][t])
    got = snap_log(log)
    assert ref.written.sum() >= 40
    assert same_bits(got["ep_return"][ref.written], ref.ep_return[ref.written])
    assert same_bits(got["length"][ref.written], ref.length[ref.written])
    env.close()


def test_captured_graph_keeps_its_log(scenes, log_off):
    """A graph captured with log A replays into A after the env was given log B."""
    acts = walk_actions(40)
    env, sched = make_log_env(scenes)
    log_a = env.set_episode_log(CAP, WANT)
    env.reset()
    H, W, C = env.frame_shape
    out = dict(image=torch.zeros((E, H, W, C), dtype=torch.uint8, device="cuda"),
               goal=torch.zeros((E, H, W, C), dtype=torch.uint8, device="cuda"),
               reward=torch.zeros(E, dtype=torch.float32, device="cuda"),
               done=torch.zeros(E, dtype=torch.bool, device="cuda"),
               state=torch.zeros(E, dtype=torch.int32, device="cuda"))
    static = torch.zeros(E, dtype=torch.int32, device="cuda")
    for t in range(4):
        static.copy_(dev(acts[t]))
        env.step(static, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(static, out=out)
    count_a = log_a.count.clone()
    log_b = env.set_episode_log(CAP, np.full(E, CAP))  # zeroes B's count only; A's tensors stay alive
    fill_sentinel(log_b)
    for t in range(4, 40):
        static.copy_(dev(acts[t]))
        g.replay()
    torch.cuda.synchronize()
    off = log_off["out"]
    ref = er.EpisodeLogRef(CAP, WANT)
    for t in range(40):
        ref.step(off["done"][t], off["success"][t], off["spl"][t], off["start_distance"][t], off["ep_length"][t],
                 off["ep_return"][t])
    a, b = snap_log(log_a), snap_log(log_b)
    assert (a["count"] == ref.count).all() and (a["count"] > count_a.cpu().numpy()).any()
    for k in LOGK:
        assert same_bits(a[k][ref.written], getattr(ref, k)[ref.written]), k
        assert (b[k].view(np.uint8) == SENT).all(), k
    assert (b["count"] == 0).all()
    # an eager step uses the new arguments
    env.step(static, out=out)
    env.step(static, out=out)
    for _ in range(LIMIT):
        env.step(static, out=out)
    assert (log_b.count.cpu().numpy() >= 1).all()
    env.close()
