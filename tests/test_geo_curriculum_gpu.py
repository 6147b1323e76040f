"""The geodesic start curriculum on the GPU (vn_nav_curriculum, VectorEnv.set_geodesic_curriculum):
the device-built start tables, every reset's draw and the level controller, bit for bit against
the restatement in tests/curriculum_ref.py; through a checkpoint, a captured graph, switching it
off again, and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import curriculum_ref as cr
import nav_ref as nr

pytestmark = pytest.mark.gpu

E, SEED = 37, 5
TASKS = [(0, 3), (1, -1), (2, 0), (1, 5), (2, 4)]


def dev(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int32), device="cuda")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def flat(s):
    return nr.Scene(graph=s.graph, spd=s.spd, frame_shape=nr.FRAME, observations=None, synth_id=7,
                    rewards=s.rewards, terminal_obs=0, name=s.name)


@pytest.fixture(scope="module")
def scenes():
    return nr.shared_scenes()


@pytest.fixture(scope="module")
def geos(scenes):
    return [nr.geodesic(s.graph) for s in scenes]


def oracle_scenes(scenes, geos):
    return [dict(graph=s.graph, spd=s.spd, rewards=s.rewards, terminal_obs=s.terminal_obs, geo=g)
            for s, g in zip(scenes, geos)]


def make_env(scenes, n=E, limit=3, tasks=None, **kw):
    import vnav
    return vnav.VectorEnv(scenes, n, seed=SEED, max_episode_steps=limit, tasks=tasks, **kw)


def table(env):
    st = env.get_state().cpu().numpy()
    return st[0], st[1], st[2], st[4]  # scene, state, goal, elapsed


def assert_same_envs(env, o, t):
    sc, s, g, el = table(env)
    assert np.array_equal(sc, o.scene) and np.array_equal(s, o.state) and np.array_equal(g, o.goal), t
    return sc, s, g, el


# ---- T1: the tables ---------------------------------------------------------------------------
def test_tables_exact(scenes):
    from vnav.scenes import maze_scene, synthetic_scene
    five = list(scenes) + [flat(synthetic_scene(0, grid=12)), flat(maze_scene(np.ones((1, 300), dtype=bool), (0, 0)))]
    assert [s.n_states for s in five] == [22, 92, 7, 376, 300]
    env = make_env(five, n=8)
    env.set_geodesic_curriculum(level=1)
    Ds = env.curriculum_state().cpu().numpy()[3]
    for k, s in enumerate(five):
        geo = nr.geodesic(s.graph)
        assert np.array_equal(env.geodesic(k).cpu().numpy(), geo)
        order, count, D = cr.tables(geo)
        got_order, got_count = (t.cpu().numpy() for t in env.curriculum_tables(k))
        assert Ds[k] == D
        assert same_bits(got_count, count), k
        assert same_bits(got_order, order), k
        # every goal has a start one action away: the rejection fallback is never taken
        assert (count[:, 2] > count[:, 1]).all(), k
    assert list(Ds) == [int(nr.geodesic(s.graph).max()) for s in five] and Ds[3] == 31 and Ds[4] == 299
    # scene c: 24 unreachable pairs in bucket 0
    assert int(env.curriculum_tables(2)[1][:, 0].sum()) == 24
    assert env.error_flags() == 0
    env.close()


# ---- T2: the draws ----------------------------------------------------------------------------
def run_draws(scenes, geos, level, mode, tasks):
    env = make_env(scenes, tasks=tasks)
    o = cr.GeoCurriculumOracle(oracle_scenes(scenes, geos), E, SEED, max_steps=3, tasks=tasks)
    Ds = [cr.scene_D(g) for g in geos]
    env.set_geodesic_curriculum(level=level, mode=mode)
    levels = [cr.clamp_level(level, 1, D) for D in Ds]
    assert list(env.curriculum_state().cpu().numpy()[0]) == levels
    o.set_geo_curriculum(mode, levels)
    # the tasks reach the env after its constructor's reset: both draw every env anew, by the curriculum
    env.reset()
    o.reset()
    assert_same_envs(env, o, -1)
    rng = np.random.RandomState(level * 7 + mode)
    starts = 0
    for t in range(60):
        a = rng.randint(0, 4, E).astype(np.int32)
        env.step(dev(a))
        o.step(a)
        sc, s, g, el = assert_same_envs(env, o, t)
        new = el == 0
        starts += int(new.sum())
        d = np.array([geos[sc[e]][g[e], s[e]] for e in range(E)])
        if mode == 1:
            assert ((d[new] >= 1) & (d[new] <= np.array(levels)[sc[new]])).all(), t
        else:
            assert (d[new] >= 1).all(), t
    assert starts > 10 * E  # max_episode_steps = 3: every env restarted many times
    assert env.error_flags() == 0 and o.flags == 0
    env.close()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("level", [1, 2, "D", "D+5"])
def test_draws_exact(scenes, geos, level, mode):
    Dmax = max(cr.scene_D(g) for g in geos)
    level = {"D": Dmax, "D+5": Dmax + 5}.get(level, level)
    run_draws(scenes, geos, level, mode, None)


def test_draws_exact_with_tasks(scenes, geos):
    run_draws(scenes, geos, 2, 2, TASKS)


# ---- T3 / T4: the controller ------------------------------------------------------------------
def run_controller(scenes, geos, n, tasks, cfg, limit, steps, optimal):
    """Steps the env and the restatement side by side, advance after every step. Returns the
    level row after every step."""
    env = make_env(scenes, n=n, limit=limit, tasks=tasks)
    o = cr.GeoCurriculumOracle(oracle_scenes(scenes, geos), n, SEED, max_steps=limit, tasks=tasks)
    env.set_geodesic_curriculum(**cfg)
    ctl = cr.Controller([cr.scene_D(g) for g in geos], o.scene, **cfg)
    o.set_geo_curriculum(cfg["mode"], ctl.level)
    env.reset()  # with the tasks, by the curriculum; vn_reset's refresh form notes the new scenes
    o.reset()
    ctl.refresh(o.scene)
    assert_same_envs(env, o, -1)
    assert same_bits(env.curriculum_state().cpu().numpy(), ctl.state())
    rng = np.random.RandomState(11)
    levels = []
    for t in range(steps):
        if optimal:
            a = env.nav_outputs()["optimal_action"].cpu().numpy()
            a = np.where(a < 0, 0, a).astype(np.int32)
        else:
            a = rng.randint(0, 4, n).astype(np.int32)
        _, _, done, info = env.step(dev(a))
        ref = o.step(a)
        assert np.array_equal(done.cpu().numpy(), ref["done"]), t
        assert np.array_equal(info["truncated"].cpu().numpy().astype(bool), ref["truncated"]), t
        ctl.count(ref["done"], ref["truncated"], o.scene)
        assert same_bits(env.curriculum_state().cpu().numpy(), ctl.state()), t
        env.curriculum_advance()
        ctl.advance()
        o.set_geo_curriculum(cfg["mode"], ctl.level)
        assert same_bits(env.curriculum_state().cpu().numpy(), ctl.state()), t
        assert_same_envs(env, o, t)
        levels.append(ctl.level.copy())
    assert env.error_flags() == 0 and o.flags == 0
    env.close()
    return np.array(levels), ctl


def test_controller_climbs_one_scene_300_envs(scenes, geos):
    """300 envs on scene b: two workgroups add to one counter."""
    cfg = dict(level=1, mode=1, window=16, up=0.8, down=0.3, step=1, level_min=1)
    D = cr.scene_D(geos[1])
    levels, _ = run_controller([scenes[1]], [geos[1]], 300, None, cfg, 30, 70, True)
    assert levels[0, 0] <= 2 and (levels[-10:, 0] == D).all() and (np.diff(levels[:, 0]) >= 0).all()


def test_controller_climbs_three_scenes_tasks(scenes, geos):
    cfg = dict(level=1, mode=1, window=16, up=0.8, down=0.3, step=2, level_min=1)
    levels, ctl = run_controller(scenes, geos, E, TASKS, cfg, 30, 260, True)
    assert (levels[-10:] == ctl.D).all() and (np.diff(levels, axis=0) >= 0).all()


@pytest.mark.parametrize("n,tasks", [(300, None), (E, TASKS)])
def test_controller_falls(scenes, geos, n, tasks):
    sc, gs = ([scenes[1]], [geos[1]]) if tasks is None else (scenes, geos)
    Dmax = max(cr.scene_D(g) for g in gs)
    cfg = dict(level=Dmax, mode=1, window=16, up=0.8, down=0.3, step=3, level_min=2)
    levels, ctl = run_controller(sc, gs, n, tasks, cfg, 2, 60 if tasks is None else 80, False)
    floor = np.minimum(2, ctl.D)
    assert (levels[0] > floor).any() and (levels[-10:] == floor).all()


def test_window_zero_is_fixed(scenes, geos):
    cfg = dict(level=3, mode=2, window=0, up=0.8, down=0.3, step=1, level_min=1)
    env = make_env(scenes, limit=4)
    env.set_geodesic_curriculum(**cfg)
    s0 = env.curriculum_state().cpu().numpy()
    assert same_bits(s0, cr.Controller([cr.scene_D(g) for g in geos], np.zeros(E), **cfg).state())
    rng = np.random.RandomState(2)
    for t in range(50):
        env.step(dev(rng.randint(0, 4, E)))
        env.curriculum_advance()
        assert same_bits(env.curriculum_state().cpu().numpy(), s0), t
    env.close()


# ---- T5: save and restore ---------------------------------------------------------------------
CFG = dict(level=2, mode=2, window=16, up=0.6, down=0.3, step=2, level_min=1)


def walk(env, acts, record):
    for a in acts:
        env.step(dev(a))
        env.curriculum_advance()
        record.append((env.get_state().cpu().numpy(), env.get_nav_state().cpu().numpy(),
                       env.curriculum_state().cpu().numpy(), env.get_episode_returns().cpu().numpy()))


def test_save_restore(scenes):
    rng = np.random.RandomState(4)
    acts = [rng.randint(0, 4, E).astype(np.int32) for _ in range(40)]
    whole, first, second = [], [], []
    a = make_env(scenes, limit=4, tasks=TASKS)
    a.set_geodesic_curriculum(**CFG)
    walk(a, acts, whole)
    a.close()
    b = make_env(scenes, limit=4, tasks=TASKS)
    b.set_geodesic_curriculum(**CFG)
    walk(b, acts[:20], first)
    saved = (b.get_state().clone(), b.get_nav_state().clone(), b.curriculum_state().clone(),
             b.get_episode_returns().clone())
    b.close()
    c = make_env(scenes, limit=4, tasks=TASKS)
    c.set_geodesic_curriculum(**CFG)
    c.set_state(saved[0])
    c.set_nav_state(saved[1])
    c.set_curriculum_state(saved[2])
    c.set_episode_returns(saved[3])
    walk(c, acts[20:], second)
    c.close()
    assert len({tuple(w[2][0]) for w in whole}) > 1  # the levels moved
    for t, (x, y) in enumerate(zip(whole, first + second)):
        for u, v in zip(x, y):
            assert same_bits(u, v), t


# ---- T6: a captured graph ---------------------------------------------------------------------
def test_graph_replay(scenes):
    rng = np.random.RandomState(6)
    acts = [rng.randint(0, 4, E).astype(np.int32) for _ in range(44)]

    def outs():
        H, W, C = nr.FRAME
        return dict(image=torch.zeros((E, H, W, C), dtype=torch.uint8, device="cuda"),
                    goal=torch.zeros((E, H, W, C), dtype=torch.uint8, device="cuda"),
                    reward=torch.zeros(E, dtype=torch.float32, device="cuda"),
                    done=torch.zeros(E, dtype=torch.bool, device="cuda"),
                    state=torch.zeros(E, dtype=torch.int32, device="cuda"))

    def snap(env, out):
        d = {k: v.cpu().numpy() for k, v in out.items()}
        d["table"] = env.get_state().cpu().numpy()
        d["cur"] = env.curriculum_state().cpu().numpy()
        return d

    cfg = dict(CFG, window=8)
    eager_env, out_e = make_env(scenes, limit=4, tasks=TASKS), outs()
    eager_env.set_geodesic_curriculum(**cfg)
    eager = []
    for a in acts:
        eager_env.step(dev(a), out=out_e)
        eager_env.curriculum_advance()
        eager.append(snap(eager_env, out_e))
    eager_env.close()
    env, out = make_env(scenes, limit=4, tasks=TASKS), outs()
    env.set_geodesic_curriculum(**cfg)
    static = torch.zeros(E, dtype=torch.int32, device="cuda")
    for t in range(4):
        static.copy_(dev(acts[t]))
        env.step(static, out=out)
        env.curriculum_advance()
        got = snap(env, out)
        assert all(same_bits(got[k], eager[t][k]) for k in got), t
    torch.cuda.synchronize()
    gen = env.config_generation
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(static, out=out)
        env.curriculum_advance()
    seen = set()
    for t in range(4, 44):
        static.copy_(dev(acts[t]))
        g.replay()
        got = snap(env, out)
        seen.add(tuple(got["cur"][0]))
        for k in got:
            assert same_bits(got[k], eager[t][k]), (t, k)
    assert len(seen) > 1  # the levels moved under the one captured graph
    assert env.config_generation == gen and env.error_flags() == 0
    env.close()


# ---- T7: off restores -------------------------------------------------------------------------
def follow(env, o, steps, seed):
    rng = np.random.RandomState(seed)
    for t in range(steps):
        a = rng.randint(0, 4, E).astype(np.int32)
        env.step(dev(a))
        o.step(a)
        assert_same_envs(env, o, t)


def test_off_restores(scenes, geos):
    from oracle.envs import VectorEnvOracle
    env = make_env(scenes)
    o = VectorEnvOracle(oracle_scenes(scenes, geos), E, SEED, max_steps=3)
    env.set_geodesic_curriculum(level=2, window=4)
    env.set_geodesic_curriculum(None)
    assert env.geo_curriculum is None
    follow(env, o, 30, 0)  # uniform starts again
    modes, offs = [s.curriculum[0] for s in scenes], [s.curriculum[1] for s in scenes]
    env.set_complexity(0.3)
    o.set_curriculum(0.3, modes, offs)
    follow(env, o, 30, 1)
    # a set_complexity curriculum that was active before is active again afterwards
    env.set_geodesic_curriculum(level=1, mode=2)
    g = cr.GeoCurriculumOracle(oracle_scenes(scenes, geos), E, SEED, max_steps=3)
    for k in ("scene", "state", "goal", "obs_state", "elapsed", "episode", "sched_pos", "ep_ret"):
        setattr(g, k, getattr(o, k).copy())
    g.set_curriculum(0.3, modes, offs)
    g.set_geo_curriculum(2, [1, 1, 1])
    follow(env, g, 20, 2)
    env.set_geodesic_curriculum(None)
    g.set_geo_curriculum(0, None)
    follow(env, g, 30, 3)
    env.set_nav_info(False)  # switches a running curriculum off first
    env.set_geodesic_curriculum(level=1)
    env.set_nav_info(False)
    assert env.geo_curriculum is None
    follow(env, g, 10, 4)
    assert env.error_flags() == 0
    env.close()


# ---- T8: refusals -----------------------------------------------------------------------------
def test_refusals(scenes):
    from vnav import _lib
    env = make_env(scenes)
    lib = env.lib
    ok = dict(mode=1, level=1, level_min=1, step=1, window=0, up=0.8, down=0.3)
    c = _lib.GeoCurriculum(**ok)
    assert lib.vn_nav_curriculum(env._ctx, ctypes.byref(c)) == -4  # VN_ESTATE before vn_nav_enable
    assert lib.vn_nav_curriculum(env._ctx, None) == -4
    env.set_nav_info(True)
    buf = torch.zeros((4, 3), dtype=torch.int32, device="cuda")
    for fn in (lib.vn_nav_curriculum_advance,):
        assert fn(env._ctx, None) == -4  # off
    assert lib.vn_nav_curriculum_get_state(env._ctx, _lib.ptr(buf), None) == -4
    assert lib.vn_nav_curriculum_set_state(env._ctx, _lib.ptr(buf), None) == -4
    assert lib.vn_nav_curriculum_tables(env._ctx, 0, None, None, None, None) == -4
    with pytest.raises(_lib.VnavError):
        env.curriculum_advance()
    bad = [dict(mode=0), dict(mode=3), dict(level=0), dict(level_min=0), dict(step=0), dict(window=-1),
           dict(up=0.3, down=0.3), dict(up=0.2, down=0.5), dict(up=1.5), dict(down=-0.1), dict(up=float("nan")),
           dict(down=float("nan"))]
    before = env.get_state().cpu().numpy()
    for b in bad:
        c = _lib.GeoCurriculum(**dict(ok, **b))
        assert lib.vn_nav_curriculum(env._ctx, ctypes.byref(c)) == -1, b  # VN_EINVAL
        with pytest.raises(_lib.VnavError):
            env.set_geodesic_curriculum(**dict(ok, **b))
        assert env.geo_curriculum is None
        assert lib.vn_nav_curriculum_advance(env._ctx, None) == -4  # still off
    env.set_complexity(0.5)  # allowed while it is off
    env.set_complexity(None)
    env.set_geodesic_curriculum(**ok)
    with pytest.raises(_lib.VnavError):
        env.set_complexity(0.5)
    with pytest.raises(_lib.VnavError):
        env.set_hardness(None)
    assert lib.vn_set_curriculum(env._ctx, ctypes.c_double(0.5), 1, ctypes.c_double(0.0)) == -4
    assert lib.vn_nav_curriculum_tables(env._ctx, 3, None, None, None, None) == -1
    good = env.curriculum_state()
    for t in (good.cpu(), good.to(torch.int64), good[:3], good.t().contiguous(), good.flatten(), good.cpu().numpy()):
        with pytest.raises(ValueError):
            env.set_curriculum_state(t)
    with pytest.raises(ValueError):
        env.curriculum_state(out=torch.zeros((4, 3), dtype=torch.float32, device="cuda"))
    env.set_curriculum_state(good)
    assert same_bits(env.curriculum_state().cpu().numpy(), good.cpu().numpy())
    assert same_bits(env.get_state().cpu().numpy(), before)
    env.close()
