"""The per-env record of vn_step (DESIGN.md "vn_step: one record per env"): every path that
reads or writes it, bit-exact against oracle.envs.VectorEnvOracle.

The record caches the graph neighbours of the env's state and the scene fields a step needs,
so the cases here are the ones where a stale cache would show: resets that change the scene
(tasks over scenes of different sizes, every step or every other step), terminal_obs, companion
frames, bad actions, autoreset off, set_state to a hand-made table, the a2c step sharing the
records with the frame step, graph replay and replay schedules. Shapes are the smallest that
reach every block shape (E = 1, 3, 4, 5, 9: partial and full blocks of 4 envs) and every copy
path (16-B, 4-B and byte lanes). No tolerances: integers, copied bytes and exact f32 sums."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import envs as oe
from test_env_gpu import compare_step, oracle_of, small_scenes

pytestmark = pytest.mark.gpu

SHAPES = {16: (4, 8, 3), 4: (6, 10, 3), 1: (5, 7, 3)}  # frame bytes 96 / 180 / 105: one per VEC path
REWARDS = (1.0, -0.01, -0.1)  # goal, step, collision: all different, sums exact in f32 only by order
TASKS = [(0, 3), (1, -1), (0, -1), (1, 7)]  # spans scenes 0 (6x8 maze) and 1 (5x5): different n_states


def _vnav():
    import vnav
    return vnav


def dev(a, dtype=torch.int32):
    return torch.as_tensor(np.asarray(a), device="cuda").to(dtype)


def scenes_of(shape, terminal_obs=0):
    return [dataclasses.replace(s, rewards=REWARDS, terminal_obs=terminal_obs) for s in small_scenes(shape)]


def arena_of(sc):
    return np.concatenate([s.observations for s in sc])


def actions(rng, n, t, bad=True):
    a = rng.randint(0, 4, size=n).astype(np.int32)
    if bad and t % 7 == 3:
        a[0] = 4
        a[-1] = -1
    return a


def oracle_table(o):
    return np.stack([o.scene, o.state, o.goal, o.obs_state, o.elapsed, o.episode, o.sched_pos]).astype(np.int32)


def check_state(env, o, tag):
    assert np.array_equal(env.get_state().cpu().numpy(), oracle_table(o)), tag
    assert np.array_equal(env.get_episode_returns().cpu().numpy().view(np.uint32), o.ep_ret.view(np.uint32)), tag


def make_out(n, shape):
    return dict(image=torch.zeros((n,) + shape, dtype=torch.uint8, device="cuda"),
                goal=torch.zeros((n,) + shape, dtype=torch.uint8, device="cuda"),
                reward=torch.empty(n, dtype=torch.float32, device="cuda"),
                done=torch.empty(n, dtype=torch.bool, device="cuda"),
                state=torch.empty(n, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("vec", [16, 4, 1])
@pytest.mark.parametrize("E", [1, 3, 4, 5, 9])
def test_env_counts_and_copy_paths(E, vec):
    """Partial and full blocks, each copy path, tasks over two scenes of different size, bad
    actions in the stream; the step limit cycles through 1, 2 and 900 over the cases."""
    vnav = _vnav()
    shape = SHAPES[vec]
    max_steps = (1, 2, 900)[(E + vec) % 3]
    sc = scenes_of(shape)
    arena = arena_of(sc)
    env = vnav.VectorEnv(sc, E, seed=77 + E, max_episode_steps=max_steps, tasks=TASKS)
    o = oracle_of(sc, E, 77 + E, max_steps=max_steps, tasks=TASKS)
    env.reset()
    o.reset()
    out = make_out(E, shape)
    rng = np.random.RandomState(E * 31 + vec)
    for t in range(30):
        a = actions(rng, E, t)
        compare_step(env.step(dev(a), out=out if t % 5 else None), o.step(a), arena, (E, vec, max_steps, t))
    check_state(env, o, (E, vec))
    assert env.error_flags() == o.flags == oe.FLAG_BAD_ACTION


@pytest.mark.parametrize("terminal_obs", [0, 1])
@pytest.mark.parametrize("max_steps", [1, 2, 900])
def test_resets_change_scene(max_steps, terminal_obs):
    """A reset every step / every other step / at the goal only: the cached row bases, graph
    offset, terminal_obs, rewards and neighbours follow the env into its new scene."""
    vnav = _vnav()
    shape = SHAPES[16]
    sc = scenes_of(shape, terminal_obs)
    arena = arena_of(sc)
    E = 5
    env = vnav.VectorEnv(sc, E, seed=5, max_episode_steps=max_steps, tasks=TASKS)
    o = oracle_of(sc, E, 5, max_steps=max_steps, tasks=TASKS)
    env.reset()
    o.reset()
    out = make_out(E, shape)
    rng = np.random.RandomState(max_steps * 2 + terminal_obs)
    scenes_seen = set()
    for t in range(40):
        a = actions(rng, E, t, bad=False)
        compare_step(env.step(dev(a), out=out), o.step(a), arena, (max_steps, terminal_obs, t))
        scenes_seen.update(o.scene.tolist())
    assert scenes_seen == {0, 1}
    check_state(env, o, (max_steps, terminal_obs))
    assert env.error_flags() == 0


def test_bad_actions_leave_the_record():
    """Actions 4 and -1: no transition, VN_FLAG_BAD_ACTION, scored as a collision; of the
    state table only the elapsed count moves."""
    vnav = _vnav()
    shape = SHAPES[16]
    sc = scenes_of(shape)
    arena = arena_of(sc)
    E = 4
    env = vnav.VectorEnv(sc, E, seed=8, max_episode_steps=900)
    o = oracle_of(sc, E, 8, max_steps=900)
    rng = np.random.RandomState(2)
    for t in range(5):
        a = actions(rng, E, t, bad=False)
        compare_step(env.step(dev(a)), o.step(a), arena, t)
    assert env.error_flags() == 0
    before = env.get_state().cpu().numpy()
    ret = env.get_episode_returns().cpu().numpy()
    a = np.array([4, -1, 4, -1], dtype=np.int32)
    step = env.step(dev(a))
    compare_step(step, o.step(a), arena, "bad")
    assert np.array_equal(step[1].cpu().numpy(), np.full(E, REWARDS[2], dtype=np.float32))
    after = env.get_state().cpu().numpy()
    expect = before.copy()
    expect[4] += 1  # elapsed
    assert np.array_equal(after, expect)
    assert np.array_equal(env.get_episode_returns().cpu().numpy(), (ret + np.float32(REWARDS[2])).astype(np.float32))
    assert env.error_flags() == oe.FLAG_BAD_ACTION
    for t in range(5):  # and the cached neighbours still belong to the unchanged state
        a = actions(rng, E, t, bad=False)
        compare_step(env.step(dev(a)), o.step(a), arena, ("after", t))


def test_companion_frames():
    """One scene with companion frames: the second output is companion[obs_state], addressed
    through the record's cached comp_base."""
    vnav = _vnav()
    shape = SHAPES[16]
    s0 = scenes_of(shape)[0]
    comp = np.random.RandomState(3).randint(0, 256, size=s0.observations.shape).astype(np.uint8)
    sc = [dataclasses.replace(s0, companion=comp)]
    n = s0.n_states
    E = 5
    env = vnav.VectorEnv(sc, E, seed=21, max_episode_steps=6)
    o = oracle_of(sc, E, 21, max_steps=6)
    out = make_out(E, shape)
    rng = np.random.RandomState(4)
    for t in range(30):
        a = actions(rng, E, t, bad=False)
        (img, second), reward, done, info = env.step(dev(a), out=out)
        ref = o.step(a)
        assert np.array_equal(info["state"].cpu().numpy(), ref["state"]), t
        assert np.array_equal(done.cpu().numpy(), ref["done"]), t
        assert np.array_equal(reward.cpu().numpy().view(np.uint32), ref["reward"].view(np.uint32)), t
        assert np.array_equal(info["img_row"].cpu().numpy(), o.obs_state), t
        assert np.array_equal(info["goal_row"].cpu().numpy(), n + o.obs_state), t
        assert np.array_equal(img.cpu().numpy(), s0.observations[o.obs_state]), t
        assert np.array_equal(second.cpu().numpy(), comp[o.obs_state]), t
    check_state(env, o, "companion")


def test_autoreset_off_steps_past_terminal():
    vnav = _vnav()
    shape = SHAPES[4]
    sc = scenes_of(shape)
    arena = arena_of(sc)
    E = 3
    env = vnav.VectorEnv(sc, E, seed=13, max_episode_steps=3, autoreset=False)
    o = oracle_of(sc, E, 13, max_steps=3, autoreset=False)
    rng = np.random.RandomState(6)
    dones = 0
    for t in range(20):
        a = actions(rng, E, t)
        ref = o.step(a)
        compare_step(env.step(dev(a)), ref, arena, t)
        dones += int(ref["done"].sum())
    assert dones >= 3 * (20 - 2)  # every step from the third on is past the limit
    check_state(env, o, "autoreset off")


def test_set_state_mid_run_and_round_trips():
    """set_state to a hand-made table (scene, state and goal all different from the current
    ones, episode and elapsed non-zero), then 10 steps against an oracle started from that
    table: the first of them runs on the rebuilt neighbours and scene fields."""
    vnav = _vnav()
    shape = SHAPES[16]
    sc = scenes_of(shape)
    arena = arena_of(sc)
    E = 5
    env = vnav.VectorEnv(sc, E, seed=3, max_episode_steps=900)
    o = oracle_of(sc, E, 3, max_steps=900)
    out = make_out(E, shape)
    rng = np.random.RandomState(9)
    for t in range(6):
        a = actions(rng, E, t, bad=False)
        compare_step(env.step(dev(a), out=out), o.step(a), arena, t)
    cur = env.get_state().cpu().numpy()
    table = np.zeros((7, E), dtype=np.int32)
    for e in range(E):
        scene = (int(cur[0, e]) + 1 + e % 2) % len(sc)
        spd = np.asarray(sc[scene].spd)
        pairs = [(s, g) for s in range(spd.shape[0]) for g in range(spd.shape[0])
                 if spd[s, g] > 1 and s != cur[1, e] and g != cur[2, e]]
        s, g = pairs[(7 * e + 3) % len(pairs)]
        table[:, e] = (scene, s, g, s, 5 + e, 11 + e, 0)
    assert (table[0] != cur[0]).all() and (table[1] != cur[1]).all() and (table[2] != cur[2]).all()
    rets = np.array([0.25, -0.5, 0.0, 1.5, -0.125], dtype=np.float32)
    env.set_state(table)
    env.set_episode_returns(rets)
    assert np.array_equal(env.get_state().cpu().numpy(), table)
    assert np.array_equal(env.get_episode_returns().cpu().numpy(), rets)
    o.scene, o.state, o.goal, o.obs_state, o.elapsed, o.episode, o.sched_pos = (table[k].astype(np.int64)
                                                                                for k in range(7))
    o.ep_ret = rets.copy()
    for t in range(10):
        a = actions(rng, E, t, bad=False)
        compare_step(env.step(dev(a), out=out), o.step(a), arena, ("after set_state", t))
    check_state(env, o, "after set_state")


def a2c_step_of(E, A, bufs):
    from vnav import _lib
    s = _lib.A2CStep()
    s.policy_out = bufs["pol"].data_ptr()
    s.num_actions = A
    s.seed = 99
    s.counter_base_dev = None
    s.counter = 0
    s.actions = bufs["act"].data_ptr()
    return s


def test_a2c_and_index_only_steps_share_the_records():
    """Frame steps with reuse on, interleaved with index-only steps and vn_step_a2c on the same
    context. Every path keeps the state, the cached fields and the output record: a frame
    step after k steps without frames writes exactly the rows whose arena row changed since
    its last frame write (checked by poisoning the rows first), and the outputs hold the
    oracle's frames."""
    vnav = _vnav()
    shape = SHAPES[16]
    sc = scenes_of(shape)
    arena = arena_of(sc)
    E, A = 9, 4
    env = vnav.VectorEnv(sc, E, seed=17, max_episode_steps=9)
    o = oracle_of(sc, E, 17, max_steps=9)
    out = make_out(E, shape)
    bufs = dict(pol=torch.zeros((E, 8), dtype=torch.float32, device="cuda"),
                act=torch.zeros(E, dtype=torch.int32, device="cuda"))
    a2c = a2c_step_of(E, A, bufs)
    rng = np.random.RandomState(12)
    last_rows = None  # arena rows the output rows hold
    t = 0
    skipped = written = 0
    for kind in "FFIFAAFIAIFFAF" * 2:
        if kind == "A":
            bufs["pol"].copy_(torch.as_tensor(rng.randn(E, 8).astype(np.float32)))
            a2c.counter = t
            env.step_a2c(a2c, out["reward"], out["done"], out["state"])
            a = bufs["act"].cpu().numpy()
            assert ((a >= 0) & (a < A)).all()
            info = dict(env._info)
            info["state"] = out["state"]
            compare_step(((None, None), out["reward"], out["done"], info), o.step(a), arena, (kind, t))
        elif kind == "I":
            a = actions(rng, E, t)
            compare_step(env.step(dev(a), out=out, gather=False), o.step(a), arena, (kind, t))
        else:
            a = actions(rng, E, t)
            if last_rows is not None:
                out["image"].fill_(0xEE)
                out["goal"].fill_(0xEE)
            (img, goal), reward, done, info = env.step(dev(a), out=out)
            ref = o.step(a)
            compare_step(((None, None), reward, done, info), ref, arena, (kind, t))
            rows = (ref["img_row"], ref["goal_row"])
            for k, buf in enumerate((img, goal)):
                got = buf.cpu().numpy()
                for e in range(E):
                    if last_rows is None or last_rows[k][e] != rows[k][e]:
                        assert np.array_equal(got[e], arena[rows[k][e]]), (kind, t, k, e, "not written")
                        written += 1
                    else:
                        assert (got[e] == 0xEE).all(), (kind, t, k, e, "written again")
                        skipped += 1
                buf.copy_(torch.as_tensor(arena[rows[k]]))  # what the env believes the rows hold
            last_rows = rows
        t += 1
    assert skipped > 0 and written > 0
    check_state(env, o, "interleaved")


def test_graph_replay_advances_the_records():
    vnav = _vnav()
    shape = SHAPES[16]
    sc = scenes_of(shape)
    arena = arena_of(sc)
    E = 5
    env = vnav.VectorEnv(sc, E, seed=23, max_episode_steps=4)
    o = oracle_of(sc, E, 23, max_steps=4)
    out = make_out(E, shape)
    static = torch.zeros(E, dtype=torch.int32, device="cuda")
    rng = np.random.RandomState(14)
    for t in range(2):
        a = actions(rng, E, t, bad=False)
        static.copy_(dev(a))
        compare_step(env.step(static, out=out), o.step(a), arena, ("eager", t))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = env.step(static, out=out)
    for k in range(3):
        a = actions(rng, E, k, bad=False)
        static.copy_(dev(a))
        g.replay()
        compare_step(captured, o.step(a), arena, ("replay", k))
    a = actions(rng, E, 0, bad=False)
    compare_step(env.step(dev(a), out=out), o.step(a), arena, "eager after replays")
    check_state(env, o, "replay")
    del g


def test_schedule_then_rng_resets():
    """A schedule of length 2, then RNG resets: the schedule position advances to 2 and stops."""
    vnav = _vnav()
    shape = SHAPES[16]
    sc = scenes_of(shape)
    arena = arena_of(sc)
    E = 5
    env = vnav.VectorEnv(sc, E, seed=29, max_episode_steps=2)
    o = oracle_of(sc, E, 29, max_steps=2)
    sched = np.zeros((E, 2, 2), dtype=np.int32)
    for e in range(E):
        spd = np.asarray(sc[e % len(sc)].spd)
        pairs = np.argwhere(spd > 2)  # the goal is out of reach within the 2-step limit
        sched[e, 0] = pairs[(3 * e + 1) % len(pairs)]
        sched[e, 1] = pairs[(5 * e + 2) % len(pairs)]
    env.set_schedule(sched)
    o.set_schedule(sched)
    env.reset()
    o.reset()
    assert np.array_equal(env.get_state().cpu().numpy()[6], np.ones(E, dtype=np.int32))
    rng = np.random.RandomState(15)
    pos = []
    for t in range(12):
        a = actions(rng, E, t, bad=False)
        compare_step(env.step(dev(a)), o.step(a), arena, t)
        pos.append(env.get_state().cpu().numpy()[6].copy())
    assert (pos[0] == 1).all() and (pos[1] == 2).all() and all((p == 2).all() for p in pos[1:])
    check_state(env, o, "schedule")
    env.set_schedule(None)  # clears the position through the record
    assert (env.get_state().cpu().numpy()[6] == 0).all()
    assert env.error_flags() == 0
