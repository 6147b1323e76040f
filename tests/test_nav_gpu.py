"""Navigation info of vn_step on the GPU (vn_nav_enable, VectorEnv(nav_info=True)): the geodesic
tables against scipy's directed BFS, the six per-step outputs against the restatement in
tests/nav_ref.py driven by the step's own state / done / truncated / ep_length, on every step
route, through resets, a mid-episode enable, a checkpoint and a captured graph."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import nav_ref as nr

pytestmark = pytest.mark.gpu

E, SEED, LIMIT, STEPS = 37, 3, 11, 200
NAV = ("distance_to_goal", "optimal_action", "optimal_mask", "success", "spl", "start_distance")
INFO = ("ep_return", "ep_length", "terminal_state", "truncated", "img_row", "goal_row")
ST = dict(scene=0, state=1, goal=2, elapsed=4)
ROUTES = ("step", "out", "index", "f32", "aux", "a2c")


def _vnav():
    import vnav
    return vnav


def dev(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int32), device="cuda")


def walk_actions(steps=STEPS, n=E):
    rng = np.random.RandomState(0)
    return [rng.randint(0, 4, n).astype(np.int32) for _ in range(steps)]


@pytest.fixture(scope="module")
def scenes():
    return nr.shared_scenes()


@pytest.fixture(scope="module")
def tables(scenes):
    return [s.graph for s in scenes], [nr.geodesic(s.graph) for s in scenes]


def aux_scenes(scenes):
    out = []
    for k, s in enumerate(scenes):
        rng = np.random.RandomState(40 + k)
        H, W = s.frame_shape[:2]
        out.append(dataclasses.replace(
            s, depth=rng.randint(0, 256, size=(s.n_states, H, W, 1)).astype(np.uint8),
            segmentation=rng.randint(0, 256, size=(s.n_states, H, W, 3)).astype(np.uint8)))
    return out


def make_env(route, scenes, nav, **kw):
    vnav = _vnav()
    opts = dict(seed=SEED, max_episode_steps=LIMIT, nav_info=nav)
    opts.update(kw)
    if route == "aux":
        return vnav.make("AuxiliaryGraph-v0", aux_scenes(scenes), E, **opts)
    if route == "f32":
        return vnav.VectorEnv(scenes, E, obs_format="f32_chw", **opts)
    return vnav.VectorEnv(scenes, E, **opts)


def nav_now(env):
    return {k: v.clone() for k, v in env.nav_outputs().items()}


def run_route(route, scenes, nav, actions, stats_every=50):
    """The trajectory on one route. Returns per-step records (device clones, stacked and
    copied at the end): frames, reward, done, state, info, the env state table, and with nav
    the six outputs; plus the values after reset(), the stats reads and the error flags."""
    from vnav import _lib
    env = make_env(route, scenes, nav)
    frames0 = env.reset()
    rec = dict(reset_frames=[f.clone() for f in frames0], reset_state=env.get_state().clone())
    if nav:
        rec["reset_nav"] = nav_now(env)
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
    steps, stats = [], []
    for t, a in enumerate(actions):
        if route == "a2c":
            # logits that make the categorical draw certain: p = 1 on the wanted action
            lg = np.zeros((E, 8), dtype=np.float32)
            lg[np.arange(E), a] = 1e4
            pol.copy_(torch.as_tensor(lg))
            s.counter = t
            env.step_a2c(s, reward, done, state)
            assert np.array_equal(act.cpu().numpy(), a)
            frames, info = (), dict(env._info)
            r, d, info["state"] = reward, done, state
        else:
            kw = dict(out=out) if out is not None else {}
            if route == "index":
                kw["gather"] = False
            frames, r, d, info = env.step(dev(a), **kw)
            frames = tuple(f for f in frames if f is not None)
        one = dict(frames=[f.clone() for f in frames], reward=r.clone(), done=d.clone(), state=info["state"].clone(),
                   table=env.get_state().clone())
        for k in INFO + (NAV if nav else ()):
            one[k] = info[k].clone()
        assert all((k in info) == nav for k in NAV)
        steps.append(one)
        if nav and (t + 1) % stats_every == 0:
            stats.append(env.nav_episode_stats().clone())
    rec["flags"] = env.error_flags()
    rec["steps"] = {k: torch.stack([s_[k] for s_ in steps]).cpu().numpy() for k in steps[0] if k != "frames"}
    rec["frames"] = [torch.stack([s_["frames"][i] for s_ in steps]).cpu().numpy()
                     for i in range(len(steps[0]["frames"]))]
    rec["stats"] = [x.cpu().numpy() for x in stats]
    for k in ("reset_frames",):
        rec[k] = [f.cpu().numpy() for f in rec[k]]
    rec["reset_state"] = rec["reset_state"].cpu().numpy()
    if nav:
        rec["reset_nav"] = {k: v.cpu().numpy() for k, v in rec["reset_nav"].items()}
    env.close()
    return rec


@pytest.fixture(scope="module")
def base(scenes):
    """The random walk through step() with nav on: every route is compared with it."""
    return run_route("step", scenes, True, walk_actions())


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_against_restatement(tables_, st_rows, rec, nav_steps, first=None, enable_at=None):
    """nav_steps[k][t] for every key against nav_ref.nav_outputs over the steps' own values.
    st_rows: dict of [T, ...] arrays (table, done, truncated, ep_length). Returns the per-step
    length offsets in force (before each step)."""
    graphs, geos = tables_
    offsets = []
    for t in range(len(st_rows["done"])):
        tb = st_rows["table"][t]
        offsets.append(rec.offset.copy())
        want = nr.nav_outputs(graphs, geos, tb[ST["scene"]], tb[ST["state"]], tb[ST["goal"]], tb[ST["elapsed"]],
                              st_rows["done"][t], st_rows["truncated"][t], st_rows["ep_length"][t], rec)
        for k in NAV:
            got = nav_steps[k][t]
            assert got.dtype == want[k].dtype, (k, got.dtype)
            assert same_bits(got, want[k]), (t, k, got, want[k])
    return np.array(offsets)


# ---- tables ---------------------------------------------------------------------------------
def test_tables_three_scenes_one_context(scenes, tables):
    env = _vnav().VectorEnv(scenes, 4, seed=1, nav_info=True)
    for k, want in enumerate(tables[1]):
        got = env.geodesic(k)
        assert got.dtype == torch.int16 and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want), k
    assert np.array_equal(env.geodesic(2).cpu().numpy().T, nr.TABLE_C)
    env.close()


def test_table_more_states_than_threads():
    """376 states: more than one state per thread of the 256-thread group, 31 levels."""
    vnav = _vnav()
    s = vnav.synthetic_scene(0, grid=12, frame_shape=nr.FRAME)
    want = nr.geodesic(s.graph)
    assert s.n_states == 376 and want.max() == 31
    env = vnav.VectorEnv([s], 4, seed=1, nav_info=True)
    assert np.array_equal(env.geodesic(0).cpu().numpy(), want)
    env.close()


# ---- the random walk --------------------------------------------------------------------------
def test_random_walk_matches_restatement(scenes, tables, base):
    graphs, geos = tables
    rec = nr.NavRecord(E)
    tb = base["reset_state"]
    want = nr.nav_refresh(graphs, geos, tb[ST["scene"]], tb[ST["state"]], tb[ST["goal"]], tb[ST["elapsed"]], rec)
    for k in ("distance_to_goal", "optimal_mask", "optimal_action"):
        assert same_bits(base["reset_nav"][k], want[k]), k
    S = base["steps"]
    pre_scene = np.concatenate([tb[ST["scene"]][None], S["table"][:-1, ST["scene"]]])
    offsets = check_against_restatement(tables, S, rec, S)
    assert base["flags"] == 0
    # the trajectory is not vacuous
    done, ok, trunc = S["done"], S["success"], S["truncated"].astype(bool)
    l, p = S["start_distance"], S["ep_length"] - offsets
    assert ok.sum() >= 50 and all((ok & (pre_scene == k)).sum() > 0 for k in range(3))
    assert (done & trunc).sum() >= 300
    assert (ok & (p == l)).sum() >= 10
    assert (ok & (p > l)).sum() >= 40
    assert (done & (l < 0)).sum() >= 50
    assert (ok & (S["ep_length"] == LIMIT)).sum() >= 1
    assert not (ok & (l < 0)).any() and not (ok & (p < l)).any()
    assert ((S["spl"] >= 0) & (S["spl"] <= 1)).all()
    # the accumulators: fp64 sums of the per-step outputs between two reads
    assert len(base["stats"]) == STEPS // 50
    for i, got in enumerate(base["stats"]):
        w = slice(50 * i, 50 * (i + 1))
        d = done[w]
        want4 = np.array([d.sum(), ok[w].sum(), S["spl"][w].astype(np.float64)[d].sum(),
                          l[w].astype(np.float64)[d].sum()])
        assert got.dtype == np.float32
        assert np.all(np.abs(got.astype(np.float64) - want4) <= 1e-6 * np.abs(want4)), (i, got, want4)


@pytest.mark.parametrize("route", ROUTES)
def test_same_numbers_on_every_route(scenes, base, route):
    """The nav outputs are identical on every route (and the stats repeat bit for bit), and
    every other output is bitwise what the route gives with nav_info off."""
    acts = walk_actions()
    on = run_route(route, scenes, True, acts)
    off = run_route(route, scenes, False, acts)
    for k in NAV:
        assert same_bits(on["steps"][k], base["steps"][k]), (route, k)
    for k in base["reset_nav"]:
        assert same_bits(on["reset_nav"][k], base["reset_nav"][k]), (route, k)
    assert len(on["stats"]) == len(base["stats"])
    for a, b in zip(on["stats"], base["stats"]):
        assert same_bits(a, b), (route, a, b)
    assert set(on["steps"]) - set(NAV) == set(off["steps"])
    for k in off["steps"]:
        assert same_bits(on["steps"][k], off["steps"][k]), (route, k)
    assert len(on["frames"]) == len(off["frames"]) == dict(step=2, out=2, index=0, f32=2, aux=5, a2c=0)[route]
    for a, b in zip(on["frames"] + on["reset_frames"], off["frames"] + off["reset_frames"]):
        assert same_bits(a, b), route
    assert same_bits(on["reset_state"], off["reset_state"])
    assert on["flags"] == off["flags"] == 0
    # the walk itself is the base's on this route too
    for k in ("table", "done", "ep_length", "truncated"):
        assert same_bits(on["steps"][k], base["steps"][k]), (route, k)


def test_info_ownership(scenes):
    """Fresh clones without out=, the env's own buffers with it."""
    env = make_env("step", scenes, True)
    a = dev(walk_actions(1)[0])
    _, _, _, i1 = env.step(a)
    keep = {k: i1[k].clone() for k in NAV}
    _, _, _, i2 = env.step(a)
    own = env.nav_outputs()
    for k in NAV:
        assert i1[k].data_ptr() != i2[k].data_ptr() != own[k].data_ptr()
        assert torch.equal(i1[k], keep[k])  # step t's info survives step t + 1
    H, W, C = env.frame_shape
    out = dict(image=torch.zeros((E, H, W, C), dtype=torch.uint8, device="cuda"),
               goal=torch.zeros((E, H, W, C), dtype=torch.uint8, device="cuda"))
    for _ in range(2):  # the validating call and the cached-pointer call
        _, _, _, i3 = env.step(a, out=out)
        for k in NAV:
            assert i3[k] is own[k]
    g0 = env.config_generation
    env.set_nav_info(False)
    assert env.config_generation == g0 + 1
    _, _, _, i4 = env.step(a)
    assert not any(k in i4 for k in NAV)
    with pytest.raises(_vnav().VnavError):
        env.geodesic(0)
    env.set_nav_info(True)
    assert env.config_generation == g0 + 2
    env.close()


# ---- shortest-path follower -------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_shortest_path_follower(scenes, which):
    n = 8
    env = _vnav().VectorEnv([scenes[which]], n, seed=5, max_episode_steps=40, nav_info=True)
    env.reset()
    nav = nav_now(env)
    dist, act = nav["distance_to_goal"].cpu().numpy(), nav["optimal_action"]
    episodes = 0
    for t in range(60):
        assert (act >= 0).all()
        _, _, done, info = env.step(act)
        d = done.cpu().numpy()
        new = info["distance_to_goal"].cpu().numpy()
        assert (new[~d] == dist[~d] - 1).all(), t
        assert (dist[d] == 1).all(), t  # the finishing step started one action from the goal
        assert info["success"].cpu().numpy()[d].all()
        assert not info["success"].cpu().numpy()[~d].any()
        assert (info["ep_length"].cpu().numpy()[d] == info["start_distance"].cpu().numpy()[d]).all()
        assert (info["spl"].cpu().numpy()[d] == np.float32(1.0)).all()
        assert (info["spl"].cpu().numpy()[~d] == 0).all()
        episodes += int(d.sum())
        dist, act = new, info["optimal_action"]
    assert episodes >= 50
    st = env.nav_episode_stats().cpu().numpy()
    assert st[0] == episodes and st[1] == episodes and st[2] == episodes
    env.close()


# ---- mid-episode enable through the raw ABI ---------------------------------------------------
def test_mid_episode_enable_raw_abi(scenes, tables):
    from vnav import _lib
    env = make_env("step", scenes, False)
    lib, ctx = env.lib, env._ctx
    acts = walk_actions(85)
    for a in acts[:5]:
        env.step(dev(a))
    bufs = [torch.zeros(E, dtype=dt, device="cuda")
            for dt in (torch.int32, torch.int32, torch.uint8, torch.uint8, torch.float32, torch.int32)]
    torch.cuda.synchronize()
    assert lib.vn_set_nav_buffers(ctx, *[_lib.ptr(b) for b in bufs]) == -4  # VN_ESTATE before enable
    assert lib.vn_get_nav_state(ctx, _lib.ptr(bufs[0]), None) == -4
    _lib.check(lib.vn_nav_enable(ctx, 1), "vn_nav_enable")
    _lib.check(lib.vn_set_nav_buffers(ctx, *[_lib.ptr(b) for b in bufs]), "vn_set_nav_buffers")
    graphs, geos = tables
    tb = env.get_state().cpu().numpy()
    assert (tb[ST["elapsed"]] > 0).sum() >= E // 2
    rec = nr.NavRecord(E)
    want = nr.nav_refresh(graphs, geos, tb[ST["scene"]], tb[ST["state"]], tb[ST["goal"]], tb[ST["elapsed"]], rec,
                          enable=True)
    assert np.array_equal(bufs[0].cpu().numpy(), want["distance_to_goal"])
    assert np.array_equal(bufs[1].cpu().numpy(), want["optimal_action"])
    assert np.array_equal(bufs[2].cpu().numpy(), want["optimal_mask"])
    state2 = torch.zeros((2, E), dtype=torch.int32, device="cuda")
    _lib.check(lib.vn_get_nav_state(ctx, _lib.ptr(state2), None), "vn_get_nav_state")
    torch.cuda.synchronize()
    assert np.array_equal(state2.cpu().numpy(), np.stack([rec.start, rec.offset]))
    running = rec.offset > 0
    rows = dict(table=[], done=[], truncated=[], ep_length=[])
    got = {k: [] for k in NAV}
    for a in acts[5:]:
        _, _, done, info = env.step(dev(a))
        assert not any(k in info for k in NAV)  # the Python env did not enable it
        rows["table"].append(env.get_state().cpu().numpy())
        rows["done"].append(done.cpu().numpy())
        rows["truncated"].append(info["truncated"].cpu().numpy())
        rows["ep_length"].append(info["ep_length"].cpu().numpy())
        for k, b in zip(NAV, bufs):
            v = b.cpu().numpy()
            got[k].append(v.astype(bool) if k == "success" else v)
    rows = {k: np.array(v) for k, v in rows.items()}
    got = {k: np.array(v) for k, v in got.items()}
    offsets = check_against_restatement(tables, rows, rec, got)
    # the episodes that were running: start distance = the distance at the enabling point, and
    # the path is counted from there
    first_done = np.argmax(rows["done"], axis=0)
    e = np.nonzero(running & rows["done"].any(axis=0))[0]
    assert len(e) >= E // 2
    assert np.array_equal(got["start_distance"][first_done[e], e], want["distance_to_goal"][e])
    assert np.array_equal(offsets[first_done[e], e], tb[ST["elapsed"]][e])
    win = e[got["success"][first_done[e], e]]
    assert len(win) >= 1
    p = rows["ep_length"][first_done[win], win] - tb[ST["elapsed"]][win]
    l = want["distance_to_goal"][win]
    assert same_bits(got["spl"][first_done[win], win],
                     np.array([nr.spl_value(True, int(a), int(b)) for a, b in zip(l, p)], dtype=np.float32))
    assert (offsets[-1][rows["done"].any(axis=0)] == 0).all()  # every later episode: offset 0
    _lib.check(lib.vn_nav_enable(ctx, 0), "vn_nav_enable")
    assert lib.vn_nav_table(ctx, 0, None, None) == -4
    env.step(dev(acts[0]))
    env.close()


# ---- autoreset off ----------------------------------------------------------------------------
def test_autoreset_off(scenes, tables):
    graphs, geos = tables
    env = make_env("step", scenes, True, autoreset=False)
    env.reset()
    rec = nr.NavRecord(E)
    tb = env.get_state().cpu().numpy()
    nr.nav_refresh(graphs, geos, tb[ST["scene"]], tb[ST["state"]], tb[ST["goal"]], tb[ST["elapsed"]], rec)
    acts = walk_actions(60)
    seen_done_again = 0
    last_done = np.zeros(E, bool)
    for t, a in enumerate(acts):
        _, _, done, info = env.step(dev(a))
        tb = env.get_state().cpu().numpy()
        d = done.cpu().numpy()
        rows = dict(table=tb[None], done=d[None], truncated=info["truncated"].cpu().numpy()[None],
                    ep_length=info["ep_length"].cpu().numpy()[None])
        got = {k: info[k].cpu().numpy()[None] for k in NAV}
        check_against_restatement(tables, rows, rec, got)
        seen_done_again += int((d & last_done).sum())
        last_done = d
        if t % 20 == 19:  # the caller resets the finished envs
            env.reset(mask=d)
            tb = env.get_state().cpu().numpy()
            want = nr.nav_refresh(graphs, geos, tb[ST["scene"]], tb[ST["state"]], tb[ST["goal"]], tb[ST["elapsed"]],
                                  rec)
            now = env.nav_outputs()
            for k in ("distance_to_goal", "optimal_mask", "optimal_action"):
                assert same_bits(now[k].cpu().numpy(), want[k]), (t, k)
            assert d.any()
            last_done = np.zeros(E, bool)
    assert seen_done_again >= 20  # steps on and after a done step were covered
    env.close()


# ---- checkpoint -------------------------------------------------------------------------------
def collect(env, acts):
    out = []
    for a in acts:
        _, r, d, info = env.step(dev(a))
        out.append(torch.cat([r.view(torch.int32), d.to(torch.int32), info["state"]] +
                             [info[k].to(torch.float32).view(torch.int32) if info[k].dtype == torch.float32
                              else info[k].to(torch.int32) for k in INFO + NAV]))
    return torch.stack(out).cpu().numpy()


def test_checkpoint_restore(scenes):
    acts = walk_actions(100)
    env = make_env("step", scenes, True)
    collect(env, acts[:50])
    saved = (env.get_state().clone(), env.get_episode_returns().clone(), env.get_nav_state().clone())
    assert saved[2].shape == (2, E) and saved[2].dtype == torch.int32
    env.nav_episode_stats()
    want = collect(env, acts[50:])
    want_stats = env.nav_episode_stats().cpu().numpy()
    env.close()
    fresh = make_env("step", scenes, True)
    fresh.set_state(saved[0])
    fresh.set_episode_returns(saved[1])
    fresh.set_nav_state(saved[2])
    assert torch.equal(fresh.get_nav_state(), saved[2])
    got = collect(fresh, acts[50:])
    assert np.array_equal(got, want)
    assert same_bits(fresh.nav_episode_stats().cpu().numpy(), want_stats)
    with pytest.raises(ValueError):
        fresh.set_nav_state(torch.zeros((2, E + 1), dtype=torch.int32))
    fresh.close()


def test_set_state_leaves_nav_record(scenes):
    env = make_env("step", scenes, True)
    collect(env, walk_actions(7))
    before = env.get_nav_state().clone()
    env.set_state(env.get_state())
    assert torch.equal(env.get_nav_state(), before)
    env.close()


# ---- hipGraph ---------------------------------------------------------------------------------
def test_graph_replay(scenes):
    acts = walk_actions(54)
    H, W, C = nr.FRAME
    keys = ("reward", "done", "state") + INFO + NAV

    def outs():
        return dict(image=torch.zeros((E, H, W, C), dtype=torch.uint8, device="cuda"),
                    goal=torch.zeros((E, H, W, C), dtype=torch.uint8, device="cuda"),
                    reward=torch.zeros(E, dtype=torch.float32, device="cuda"),
                    done=torch.zeros(E, dtype=torch.bool, device="cuda"),
                    state=torch.zeros(E, dtype=torch.int32, device="cuda"))

    def snap(ret):
        (img, goal), r, d, info = ret
        vals = dict(info, reward=r, done=d, image=img, goal=goal)
        return {k: vals[k].cpu().numpy().copy() for k in keys + ("image", "goal")}

    eager_env, out_e = make_env("step", scenes, True), outs()
    eager = [snap(eager_env.step(dev(a), out=out_e)) for a in acts]
    eager_stats = eager_env.nav_episode_stats().cpu().numpy()
    eager_env.close()
    env, out = make_env("step", scenes, True), outs()
    static = torch.zeros(E, dtype=torch.int32, device="cuda")
    for t in range(4):
        static.copy_(dev(acts[t]))
        got = snap(env.step(static, out=out))
        assert all(same_bits(got[k], eager[t][k]) for k in got), t
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
        captured = env.step(static, out=out)
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0  # nothing allocated in capture
    for k in NAV:
        assert captured[3][k] is env.nav_outputs()[k]
    for t in range(4, 54):
        static.copy_(dev(acts[t]))
        g.replay()
        got = snap(captured)
        for k in got:
            assert same_bits(got[k], eager[t][k]), (t, k)
    assert same_bits(env.nav_episode_stats().cpu().numpy(), eager_stats)
    assert env.error_flags() == 0
    env.close()


# ---- refusals and the single-env wrapper ------------------------------------------------------
def test_python_buffer_refusals(scenes):
    env = make_env("step", scenes, False)
    dts = [torch.int32, torch.int32, torch.uint8, torch.bool, torch.float32, torch.int32]

    def bufs(**repl):
        b = [torch.zeros(E, dtype=dt, device="cuda") for dt in dts]
        for i, t in repl.items():
            b[int(i[1:])] = t
        return b

    bad = [bufs(_0=torch.zeros(E, dtype=torch.int64, device="cuda")),      # wrong dtype
           bufs(_4=torch.zeros(E, dtype=torch.float64, device="cuda")),
           bufs(_3=torch.zeros(E, dtype=torch.uint8, device="cuda")),
           bufs(_1=torch.zeros(E, dtype=torch.int32)),                      # wrong device
           bufs(_5=torch.zeros(E - 1, dtype=torch.int32, device="cuda")),  # wrong length
           bufs(_2=torch.zeros(2 * E, dtype=torch.uint8, device="cuda")[::2]),  # not contiguous
           bufs()[:5]]
    for b in bad:
        with pytest.raises(ValueError):
            env.set_nav_info(True, buffers=b)
        assert not env.nav_info
    for call in (env.nav_episode_stats, env.get_nav_state, env.nav_outputs, lambda: env.geodesic(0)):
        with pytest.raises(_vnav().VnavError):
            call()
    # a partial set: the rest is not written, the keys not reported
    mine = bufs()
    mine[2] = mine[4] = None
    env.set_nav_info(True, buffers=mine)
    _, _, _, info = env.step(dev(walk_actions(1)[0]), out=None)
    assert "optimal_mask" not in info and "spl" not in info and "distance_to_goal" in info
    with pytest.raises(ValueError):
        env.nav_episode_stats(out=torch.zeros(3, dtype=torch.float32, device="cuda"))
    with pytest.raises(_vnav().VnavError):
        env.geodesic(3)
    env.close()


def test_single_env_wrapper_scalars(scenes, tables):
    vnav = _vnav()
    sc = dataclasses.replace(scenes[0], observations=np.zeros((22,) + nr.FRAME, dtype=np.uint8))
    env = vnav.CachedThorEnv(sc, seed=2, max_episode_steps=30, nav_info=True)
    env.reset()
    s, g = env.state
    graph, geo = tables[0][0], tables[1][0]
    d, _, a = nr.distance_mask_action(graph, geo, s, g)
    steps = 0
    while True:
        _, _, done, info = env.step(a)
        steps += 1
        assert type(info["distance_to_goal"]) is int and type(info["spl"]) is float
        assert type(info["success"]) is bool and type(info["optimal_action"]) is int
        assert info["distance_to_goal"] == d - steps
        if done:
            break
        a = info["optimal_action"]
    assert steps == d and info["success"] and info["spl"] == 1.0 and info["start_distance"] == d
    env.close()
    plain = vnav.CachedThorEnv(sc, seed=2, max_episode_steps=30)
    plain.reset()
    assert not any(k in plain.step(0)[3] for k in NAV)
    plain.close()
