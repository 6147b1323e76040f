"""The state-visit counts of vn_step on the GPU (vn_visit_enable, VectorEnv(visit_counts=True)):
visit_cell, first_visit, coverage, the table, the episode records and the seen bitmaps bitwise the
restatement of tests/visit_ref.py, driven by the step's own state table, done and terminal_state,
with max_episode_steps=3 so that truncations and auto-resets are dense: at the bitmap's word edges
(scenes of 2, 31, 32, 33, 64 and 65 states), at the lane-group and workgroup edges (1, 63, 64, 65 and
257 envs), with resets that change the env's scene, on every step route, with and without info
buffers, with the nav stack on, through masked resets, set_state and auto-reset off; the output
swap, the clear, the statistics, the checkpoint round trip, a captured step and the C ABI's
refusals."""
import ctypes

import numpy as np
import pytest
import torch

import nav_ref as nr
import test_nav_gpu as tn
import visit_ref as vr

pytestmark = pytest.mark.gpu

SEED, LIMIT, STEPS = 5, 3, 40
RESET_AT, SAVE_AT, SET_STATE_AT = 17, 12, 31
SIZES = (2, 31, 32, 33, 64, 65)
FRAME = (8, 8, 3)
ST = dict(scene=0, state=1, goal=2, obs_state=3, elapsed=4)
VN_EINVAL, VN_ESTATE = -1, -4


def ring_scene(n, k):
    """n states on a ring: forward, back, a wall, three forward."""
    from vnav.scenes import Scene
    i = np.arange(n)
    graph = np.stack([(i + 1) % n, (i - 1) % n, np.full(n, -1), (i + 3) % n], axis=1).astype(np.int64)
    spd = nr.geodesic(graph).T.astype(np.int64)
    return Scene(graph=graph, spd=spd, frame_shape=FRAME, observations=None, synth_id=k, terminal_obs=k % 2,
                 name="ring-%d" % n)


@pytest.fixture(scope="module")
def scenes():
    return [ring_scene(n, k) for k, n in enumerate(SIZES)]


def tasks_of(scenes):
    return [(k, -1) for k in range(len(scenes))]  # every reset draws the scene too


def make_env(route, scenes, E, visits=True, **kw):
    import vnav
    opts = dict(seed=SEED, max_episode_steps=LIMIT, visit_counts=visits, tasks=tasks_of(scenes))
    opts.update(kw)
    if route == "aux":
        return vnav.make("AuxiliaryGraph-v0", tn.aux_scenes(scenes), E, **opts)
    if route == "f32":
        return vnav.VectorEnv(scenes, E, obs_format="f32_chw", **opts)
    return vnav.VectorEnv(scenes, E, **opts)


def actions_of(E, steps=STEPS):
    rng = np.random.RandomState([7, E])
    return [rng.randint(0, 4, E).astype(np.int32) for _ in range(steps)]


def table_of(env):
    tb = env.get_state().cpu().numpy()
    return tb[ST["scene"]], tb[ST["state"]]


class Checked:
    """An env with visits on, its restatement started from the env's states, and the three
    output buffers; step() steps on one route and compares everything by bits."""

    def __init__(self, route, env, scenes, E, autoreset=True):
        from vnav import _lib
        self.route, self.env, self.E, self.autoreset = route, env, E, autoreset
        self.vs = vr.VisitState([s.n_states for s in scenes], E)
        vr.visit_start(self.vs, *table_of(env))
        self.bufs = [torch.full((E,), -9, dtype=torch.int32, device="cuda"),
                     torch.zeros(E, dtype=torch.bool, device="cuda"),
                     torch.full((E,), -9, dtype=torch.int32, device="cuda")]
        env.set_visit_outputs(*self.bufs)
        self.cases = dict(done=0, scene_change=0, truncated=0, reentry=0, first=0)
        if route == "a2c":
            self.pol = torch.zeros((E, 8), dtype=torch.float32, device="cuda")
            self.act = torch.zeros(E, dtype=torch.int32, device="cuda")
            s = _lib.A2CStep()
            s.policy_out, s.num_actions, s.seed, s.counter_base_dev = self.pol.data_ptr(), 4, 99, None
            s.actions = self.act.data_ptr()
            self.s = s
            self.reward = torch.zeros(E, dtype=torch.float32, device="cuda")
            self.done = torch.zeros(E, dtype=torch.bool, device="cuda")
            self.state = torch.zeros(E, dtype=torch.int32, device="cuda")

    def env_step(self, t, a):
        env, E = self.env, self.E
        if self.route == "a2c":
            lg = np.zeros((E, 8), dtype=np.float32)
            lg[np.arange(E), a] = 1e4  # the categorical draw is certain
            self.pol.copy_(torch.as_tensor(lg))
            self.s.counter = t
            env.step_a2c(self.s, self.reward, self.done, self.state)
            assert np.array_equal(self.act.cpu().numpy(), a)
            return self.done, dict(env._info)
        kw = dict(gather=False) if self.route == "index" else {}
        _, _, d, info = env.step(tn.dev(a), **kw)
        return d, info

    def check_state(self, where):
        got = self.env.get_visit_state().cpu().numpy()
        want = self.vs.packed()
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got, want), (where, np.flatnonzero(got != want)[:8])

    def step(self, t, a):
        prev_scene = self.vs.ep_scene.copy()
        d, info = self.env_step(t, a)
        done = d.cpu().numpy() != 0
        scene, state = table_of(self.env)
        cell, first, cov = vr.visit_step(self.vs, scene, state, done, info["terminal_state"].cpu().numpy(),
                                         autoreset=self.autoreset)
        got = [b.cpu().numpy() for b in self.bufs]
        assert np.array_equal(got[0], cell), (t, got[0], cell)
        assert np.array_equal(got[1].astype(np.uint8), first), (t, got[1], first)
        assert np.array_equal(got[2], cov), (t, got[2], cov)
        self.check_state(t)
        c = self.cases
        c["done"] += int(done.sum())
        c["scene_change"] += int((done & (scene != prev_scene)).sum())
        c["truncated"] += int((done & (info["truncated"].cpu().numpy() != 0)).sum())
        c["reentry"] += int((first == 0).sum())
        c["first"] += int((first != 0).sum())
        return done

    def reset(self, mask):
        self.env.reset(mask=tn.dev(mask))
        vr.visit_start(self.vs, *table_of(self.env), mask=mask)
        self.check_state("reset")

    def set_state(self, table):
        self.env.set_state(table)
        vr.visit_start(self.vs, *table_of(self.env), add=False)
        self.check_state("set_state")


def walk(route, scenes, E, autoreset=True, **kw):
    """The scripted trajectory: random actions, a masked reset() after step RESET_AT, a
    set_state() to the table of step SAVE_AT after step SET_STATE_AT; with auto-reset off, a
    masked reset of the finished envs after every second step (so finished envs are also
    stepped on)."""
    env = make_env(route, scenes, E, autoreset=autoreset, **kw)
    env.reset()
    env.clear_visits()  # the states before reset() were counted at the enable
    ck = Checked(route, env, scenes, E, autoreset)
    ck.check_state("start")
    rng = np.random.RandomState([8, E])
    saved = None
    for t, a in enumerate(actions_of(E)):
        done = ck.step(t, a)
        if t == SAVE_AT:
            saved = env.get_state().clone()
        mask = None
        if not autoreset and t % 2 == 1 and done.any():
            mask = done.astype(np.int32)
        if t == RESET_AT:
            extra = (rng.rand(E) < 0.4).astype(np.int32) if E > 1 else np.ones(1, dtype=np.int32)
            mask = extra if mask is None else (mask | extra)
        if mask is not None:
            ck.reset(mask)
        if t == SET_STATE_AT:
            ck.set_state(saved)
    assert env.error_flags() == 0
    return env, ck


@pytest.mark.parametrize("E", [1, 63, 64, 65, 257])
def test_matches_restatement(scenes, E):
    env, ck = walk("u8", scenes, E)
    print("VISITCASES E=%d %s" % (E, ck.cases))
    if E > 1:
        for k, v in ck.cases.items():
            assert v > 0, (k, ck.cases)
    # the statistics and the live views against the restatement's table
    for k in [None] + list(range(len(scenes))):
        assert np.array_equal(env.visit_stats(k).cpu().numpy(), ck.vs.stats(k)), k
    assert np.array_equal(env.visit_stats().cpu().numpy(), env.visit_stats().cpu().numpy())
    off = ck.vs.cell_off
    for k, s in enumerate(scenes):
        view = env.visit_table(k)
        assert view.dtype == torch.int32 and tuple(view.shape) == (s.n_states,) and view.is_cuda
        assert np.array_equal(view.cpu().numpy().view(np.uint32), ck.vs.count[off[k]:off[k + 1]])
    p, q, C = env.visit_cells()
    assert C == sum(SIZES) and p == env.visit_table(0).data_ptr() and q
    env.close()


def test_257_envs_on_two_states():
    """Every env adds to the same two cells in one launch: the table is still exact."""
    two = [ring_scene(2, 0)]
    env, ck = walk("u8", two, 257)
    total = int(env.visit_stats().cpu().numpy()[1])
    assert total == int(ck.vs.count.astype(np.int64).sum()) and total > 257 * STEPS
    env.close()


@pytest.mark.parametrize("route", ["index", "f32", "aux", "a2c"])
def test_every_route(scenes, route):
    env, ck = walk(route, scenes, 65)
    assert ck.cases["done"] > 0 and ck.cases["scene_change"] > 0 and ck.cases["reentry"] > 0
    assert {"visit_cell", "first_visit", "coverage"} <= set(env._info)
    env.close()


def test_autoreset_off(scenes):
    env, ck = walk("u8", scenes, 65, autoreset=False)
    assert ck.cases["done"] > 0 and ck.cases["truncated"] > 0
    env.close()


def test_nav_stack_changes_nothing(scenes):
    """With nav info and progress on, every visit output and the whole visit state are what they
    are without them; with the adaptive geodesic curriculum on top (other starts) they are still
    the restatement's."""
    E = 65
    plain, ck0 = walk("u8", scenes, E)
    nav, ck1 = walk("u8", scenes, E, nav_info=True, nav_progress=True)
    assert torch.equal(plain.get_visit_state(), nav.get_visit_state())
    assert torch.equal(plain.get_state(), nav.get_state())
    plain.close()
    nav.close()
    env = make_env("u8", scenes, E, nav_info=True, nav_progress=True)
    env.set_geodesic_curriculum(level=1, window=8)
    env.reset()
    env.clear_visits()
    ck = Checked("u8", env, scenes, E)
    ck.check_state("clear")
    for t, a in enumerate(actions_of(E, 12)):
        ck.step(t, a)
        env.curriculum_advance()
    assert ck.cases["done"] > 0
    env.close()


def test_stand_ins_without_info_buffers(scenes):
    """The raw ABI with no info buffers and no done output: the visit state's own done and
    terminal_state stand in, and the visit outputs are those of an env that has them."""
    from vnav import _lib
    lib = _lib.load()
    E = 65
    a_env, b_env = make_env("u8", scenes, E), make_env("u8", scenes, E)
    a_env.reset()
    b_env.reset()
    _lib.check(lib.vn_set_info_buffers(b_env._ctx, None, None, None, None, None, None), "vn_set_info_buffers")
    outs = [[torch.full((E,), -9, dtype=torch.int32, device="cuda"), torch.zeros(E, dtype=torch.bool, device="cuda"),
             torch.full((E,), -9, dtype=torch.int32, device="cuda")] for _ in range(2)]
    a_env.set_visit_outputs(*outs[0])
    b_env.set_visit_outputs(*outs[1])
    st = _lib.stream_ptr(b_env.device)
    for a in actions_of(E, 16):
        a_env.step(tn.dev(a), gather=False)
        _lib.check(lib.vn_step(b_env._ctx, _lib.ptr(tn.dev(a)), None, None, None, None, None, st), "vn_step")
        for x, y in zip(*outs):
            assert torch.equal(x, y)
    assert torch.equal(a_env.get_visit_state(), b_env.get_visit_state())
    assert int(a_env.visit_stats()[1]) > E * 16  # episodes did end on the way
    a_env.close()
    b_env.close()


def test_output_swap_and_clear(scenes):
    """info's tensors are the env's own buffers until the outputs are pointed elsewhere; a NULL
    output is not written; all-None points them back; clear_visits restarts the table."""
    E = 63
    env = make_env("u8", scenes, E)
    env.reset()
    env.clear_visits()
    ck = Checked("u8", env, scenes, E)
    env.set_visit_outputs(None, None, None)  # back to the env's own
    own = [env._info[k] for k in ("visit_cell", "first_visit", "coverage")]
    acts = actions_of(E, 12)
    for t, a in enumerate(acts):
        if t == 4:
            env.set_visit_outputs(ck.bufs[0], None, None)  # the cell only
            kept = [x.clone() for x in own]
            for b in ck.bufs[1:]:
                b.fill_(0)
        if t == 8:
            env.set_visit_outputs(None, None, None)
            mine = ck.bufs[0].clone()
        _, _, d, info = env.step(tn.dev(a), out=None)
        cell, first, cov = vr.visit_step(ck.vs, *table_of(env), d.cpu().numpy(), info["terminal_state"].cpu().numpy())
        if 4 <= t < 8:
            assert np.array_equal(ck.bufs[0].cpu().numpy(), cell)
            assert all(torch.equal(x, y) for x, y in zip(own, kept))
            assert not ck.bufs[1].any() and not ck.bufs[2].any()
        else:
            assert np.array_equal(own[0].cpu().numpy(), cell) and np.array_equal(own[2].cpu().numpy(), cov)
            assert np.array_equal(own[1].cpu().numpy().astype(np.uint8), first) and own[1].dtype == torch.bool
            assert np.array_equal(info["visit_cell"].cpu().numpy(), cell)  # fresh clones without out=
            if t >= 8:
                assert torch.equal(ck.bufs[0], mine)
    ck.check_state("swap")
    env.clear_visits()
    vr.visit_clear(ck.vs, *table_of(env))
    ck.check_state("clear")
    assert list(env.visit_stats().cpu().numpy())[1] == E
    with pytest.raises(ValueError):
        env.set_visit_outputs(torch.zeros(E + 1, dtype=torch.int32, device="cuda"), None, None)
    with pytest.raises(ValueError):
        env.set_visit_outputs(None, torch.zeros(E, dtype=torch.uint8, device="cuda"), None)
    env.close()


def collect(env, acts, bufs):
    out = []
    for a in acts:
        _, r, d, info = env.step(tn.dev(a))
        out.append(torch.cat([r.view(torch.int32), d.to(torch.int32), info["state"]] +
                             [b.to(torch.int32) for b in bufs] + [env.get_visit_state()]))
    return torch.stack(out).cpu().numpy()


def test_state_round_trip(scenes):
    E = 65
    acts = actions_of(E, 40)

    def fresh():
        env = make_env("u8", scenes, E)
        bufs = [torch.full((E,), -9, dtype=torch.int32, device="cuda"), torch.zeros(E, dtype=torch.bool, device="cuda"),
                torch.full((E,), -9, dtype=torch.int32, device="cuda")]
        env.set_visit_outputs(*bufs)
        return env, bufs

    env, bufs = fresh()
    collect(env, acts[:20], bufs)
    saved = (env.get_state().clone(), env.get_episode_returns().clone(), env.get_visit_state().clone())
    want = collect(env, acts[20:], bufs)
    env.close()
    env, bufs = fresh()
    collect(env, acts[:3], bufs)  # another position: the restore must replace all of it
    env.set_state(saved[0])
    env.set_episode_returns(saved[1])
    env.set_visit_state(saved[2])
    assert torch.equal(env.get_visit_state(), saved[2])
    got = collect(env, acts[20:], bufs)
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        env.set_visit_state(torch.zeros(saved[2].numel() + 1, dtype=torch.int32))
    env.close()


def test_captured_step_replays(scenes):
    """A captured step keeps the output pointers it was recorded with and counts into the live
    table: every replay equals the eager run, after the outputs were pointed elsewhere and the
    table was cleared and restored in between."""
    E = 65
    acts = actions_of(E, 24)
    H, W, C = FRAME

    def outs():
        return dict(image=torch.zeros((E, H, W, C), dtype=torch.uint8, device="cuda"),
                    goal=torch.zeros((E, H, W, C), dtype=torch.uint8, device="cuda"),
                    reward=torch.zeros(E, dtype=torch.float32, device="cuda"),
                    done=torch.zeros(E, dtype=torch.bool, device="cuda"),
                    state=torch.zeros(E, dtype=torch.int32, device="cuda"))

    def snap(env):
        return torch.cat([env._info[k].to(torch.int32) for k in ("visit_cell", "first_visit", "coverage")] +
                         [env.get_visit_state()]).cpu().numpy()

    e_env, e_out = make_env("u8", scenes, E), outs()
    eager = []
    for a in acts:
        e_env.step(tn.dev(a), out=e_out)
        eager.append(snap(e_env))
    e_env.close()
    env, out = make_env("u8", scenes, E), outs()
    static = torch.zeros(E, dtype=torch.int32, device="cuda")
    for t in range(4):
        static.copy_(tn.dev(acts[t]))
        env.step(static, out=out)
        assert np.array_equal(snap(env), eager[t]), t
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(static, out=out)
    other = [torch.full((E,), -5, dtype=torch.int32, device="cuda"), torch.zeros(E, dtype=torch.bool, device="cuda"),
             torch.full((E,), -5, dtype=torch.int32, device="cuda")]
    env.set_visit_outputs(*other)  # the graph holds the recorded pointers
    keep = env.get_visit_state().clone()
    env.clear_visits()
    env.set_visit_state(keep)  # the table changed and came back: the graph reads the live one
    for t in range(4, 24):
        static.copy_(tn.dev(acts[t]))
        g.replay()
        assert np.array_equal(snap(env), eager[t]), t
    assert (other[0] == -5).all() and (other[2] == -5).all() and not other[1].any()
    assert env.error_flags() == 0
    env.close()


def test_abi_refusals(scenes):
    """VN_ESTATE before vn_visit_enable, VN_EINVAL for bad arguments, the context unchanged by
    either; visits work with navigation info off and survive vn_nav_enable either way."""
    import vnav
    from vnav import _lib
    lib = _lib.load()
    E = 5
    env = make_env("u8", scenes, E, visits=False)
    env.reset()
    st = _lib.stream_ptr(env.device)
    buf = torch.zeros(4096, dtype=torch.int32, device="cuda")
    p, n, c64 = ctypes.c_void_p(), ctypes.c_int32(), ctypes.c_int64()
    calls = [lambda: lib.vn_set_visit_outputs(env._ctx, None, None, None),
             lambda: lib.vn_visit_table(env._ctx, 0, ctypes.byref(p), ctypes.byref(n)),
             lambda: lib.vn_visit_cells(env._ctx, ctypes.byref(p), None, ctypes.byref(c64)),
             lambda: lib.vn_visit_get_state(env._ctx, _lib.ptr(buf), st),
             lambda: lib.vn_visit_set_state(env._ctx, _lib.ptr(buf), st),
             lambda: lib.vn_visit_clear(env._ctx, st),
             lambda: lib.vn_visit_stats(env._ctx, -1, _lib.ptr(buf), st)]
    for k, f in enumerate(calls):
        assert f() == VN_ESTATE, k
    assert lib.vn_visit_enable(None, 1) == VN_EINVAL
    with pytest.raises(_lib.VnavError):
        env.visit_stats()
    assert "visit_cell" not in env._info
    a = tn.dev(actions_of(E, 1)[0])
    assert "visit_cell" not in env.step(a)[3]  # off: the step is what it was
    env.set_visit_counts(True)
    assert env.visit_counts and not env.nav_info
    before = env.get_visit_state().clone()
    assert lib.vn_visit_table(env._ctx, len(scenes), ctypes.byref(p), ctypes.byref(n)) == VN_EINVAL
    assert lib.vn_visit_table(env._ctx, -1, ctypes.byref(p), ctypes.byref(n)) == VN_EINVAL
    assert lib.vn_visit_stats(env._ctx, len(scenes), _lib.ptr(buf), st) == VN_EINVAL
    assert lib.vn_visit_stats(env._ctx, -2, _lib.ptr(buf), st) == VN_EINVAL
    assert lib.vn_visit_stats(env._ctx, 0, None, st) == VN_EINVAL
    assert lib.vn_visit_get_state(env._ctx, None, st) == VN_EINVAL
    assert lib.vn_visit_set_state(env._ctx, None, st) == VN_EINVAL
    assert torch.equal(env.get_visit_state(), before)
    assert list(env.visit_stats().cpu().numpy()) == [len(set(zip(*[x.tolist() for x in table_of(env)]))), E]
    env.set_nav_info(True)
    env.set_nav_info(False)
    assert env.visit_counts and torch.equal(env.get_visit_state(), before)
    assert set(env.step(a)[3]) >= {"visit_cell", "first_visit", "coverage"}
    env.set_visit_counts(False)
    assert not env.visit_counts and "visit_cell" not in env._info
    assert lib.vn_visit_clear(env._ctx, st) == VN_ESTATE
    env.close()
    made = vnav.make("CachedThor-v0", scenes, 3, visit_counts=True)
    assert made.visit_counts
    made.close()
