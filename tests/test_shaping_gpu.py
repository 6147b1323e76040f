"""The geodesic progress of vn_step on the GPU (vn_nav_progress, VectorEnv(nav_progress=True)):
dist_before, dist_after and progress exactly the restatement of tests/shaping_ref.py, driven by the
step's own state table, done, truncated and terminal_state, on every step route, with auto-reset
on and off, through masked resets and a mid-episode set_state, at one lane, a ragged block and a
second workgroup; every other output of the step bitwise what it is with progress off; the record's
checkpoint round trip, a captured step_a2c, and the state rules of the C ABI."""
import numpy as np
import pytest
import torch

import nav_ref as nr
import shaping_ref as sr
import test_nav_gpu as tn

pytestmark = pytest.mark.gpu

SEED, LIMIT, STEPS = 3, 5, 48
RESET_AT, SAVE_AT, SET_STATE_AT = 17, 12, 31
ROUTES = ("u8", "index", "f32", "aux", "a2c")
TASKS = [(0, -1), (1, -1), (2, -1)]  # every reset draws the scene too: envs move between scenes
ST = tn.ST
VN_ESTATE = -4


@pytest.fixture(scope="module")
def scenes():
    return nr.shared_scenes()


@pytest.fixture(scope="module")
def tables(scenes):
    return [s.graph for s in scenes], [nr.geodesic(s.graph) for s in scenes]


def make_env(route, scenes, E, progress, autoreset=True):
    import vnav
    opts = dict(seed=SEED, max_episode_steps=LIMIT, nav_info=True, nav_progress=progress, autoreset=autoreset,
                tasks=TASKS)
    if route == "aux":
        return vnav.make("AuxiliaryGraph-v0", tn.aux_scenes(scenes), E, **opts)
    if route == "f32":
        return vnav.VectorEnv(scenes, E, obs_format="f32_chw", **opts)
    return vnav.VectorEnv(scenes, E, **opts)


def actions_of(E, steps=STEPS):
    rng = np.random.RandomState([1, E])
    return [rng.randint(0, 4, E).astype(np.int32) for _ in range(steps)]


class Stepper:
    """One env stepped on one route; step() returns the step's outputs as device clones."""

    def __init__(self, route, env, E):
        from vnav import _lib
        self.route, self.env, self.E = route, env, E
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

    def step(self, t, a):
        env, E = self.env, self.E
        if self.route == "a2c":
            lg = np.zeros((E, 8), dtype=np.float32)
            lg[np.arange(E), a] = 1e4  # the categorical draw is certain
            self.pol.copy_(torch.as_tensor(lg))
            self.s.counter = t
            env.step_a2c(self.s, self.reward, self.done, self.state)
            assert np.array_equal(self.act.cpu().numpy(), a)
            frames, info = (), dict(env._info)
            r, d, info["state"] = self.reward, self.done, self.state
        else:
            kw = dict(gather=False) if self.route == "index" else {}
            frames, r, d, info = env.step(tn.dev(a), **kw)
            frames = tuple(f for f in frames if f is not None)
        one = dict(reward=r.clone(), done=d.clone().to(torch.uint8), state=info["state"].clone(),
                   table=env.get_state().clone())
        for k in tn.INFO + tn.NAV:
            one[k] = info[k].clone()
        one["frames"] = [f.clone() for f in frames]
        one["info_keys"] = sorted(info)
        return one


def run(route, scenes, E, progress, autoreset=True):
    """The scripted trajectory: random actions, a masked reset() after step RESET_AT, a set_state()
    to the table of step SAVE_AT after step SET_STATE_AT; with auto-reset off, a masked reset of
    the finished envs after every step. Returns the steps' stacked outputs, the three progress
    outputs per step and the refresh events [(after step, mask or None, table after)]."""
    env = make_env(route, scenes, E, progress, autoreset)
    env.reset()
    bufs = None
    if progress:
        assert env._info["distance_before"].dtype == torch.int32 and env._info["progress"].shape == (E,)
        bufs = [torch.full((E,), -99, dtype=torch.int32, device="cuda") for _ in range(3)]
        env.set_nav_progress_outputs(*bufs)
    st = Stepper(route, env, E)
    rec = dict(table0=env.get_state().cpu().numpy(), steps=[], prog=[], events=[], actions=actions_of(E))
    rng = np.random.RandomState([2, E])
    saved = None
    for t, a in enumerate(rec["actions"]):
        one = st.step(t, a)
        rec["steps"].append(one)
        if progress:
            rec["prog"].append(torch.stack(bufs).clone())
        if t == SAVE_AT:
            saved = one["table"].clone()
        mask = None
        if not autoreset and bool(one["done"].any()):
            mask = one["done"].cpu().numpy().astype(np.int32)
        if t == RESET_AT:
            extra = (rng.rand(E) < 0.4).astype(np.int32)
            mask = extra if mask is None else (mask | extra)
            if E == 1:
                mask = np.ones(1, dtype=np.int32)
        if mask is not None:
            env.reset(mask=tn.dev(mask))
            rec["events"].append((t, mask, env.get_state().cpu().numpy()))
        if t == SET_STATE_AT:
            env.set_state(saved)
            rec["events"].append((t, None, env.get_state().cpu().numpy()))
    rec["flags"] = env.error_flags()
    keys = [k for k in rec["steps"][0] if k not in ("frames", "info_keys")]
    rec["out"] = {k: torch.stack([s[k] for s in rec["steps"]]).cpu().numpy() for k in keys}
    rec["frames"] = [torch.stack([s["frames"][i] for s in rec["steps"]]).cpu().numpy()
                     for i in range(len(rec["steps"][0]["frames"]))]
    rec["info_keys"] = rec["steps"][0]["info_keys"]
    if progress:
        rec["prog"] = torch.stack(rec["prog"]).cpu().numpy()  # [steps, 3, E]
        rec["own"] = (env._info["distance_before"].cpu().numpy(), env._info["progress"].cpu().numpy())
    del rec["steps"]
    env.close()
    return rec


def restate(tables_, rec, E):
    """The restatement over the run's own tables and step values; returns ([steps, 3, E], the
    counts of the cases the trajectory contains)."""
    graphs, geos = tables_
    o = rec["out"]
    record = sr.ProgressRecord(E)
    tb = rec["table0"]
    sr.progress_refresh(geos, tb[ST["scene"]], tb[ST["state"]], tb[ST["goal"]], record)
    events = {}
    for t, mask, table in rec["events"]:
        events.setdefault(t, []).append((mask, table))
    want = []
    count = dict(success=0, truncated_far=0, blocked=0, other_scene=0, plus=0, zero=0, minus=0, invalid=0,
                 masked_reset=0, set_state=0)
    prev = tb
    for t in range(len(o["done"])):
        tb = o["table"][t]
        done, trunc = o["done"][t] != 0, o["truncated"][t] != 0
        scene_p = record.scene.copy()
        b, a, p = sr.progress_ref(geos, tb[ST["scene"]], tb[ST["state"]], tb[ST["goal"]], done, trunc,
                                  o["terminal_state"][t], record)
        want.append(np.stack([b, a, p]))
        count["success"] += int((done & ~trunc).sum())
        count["truncated_far"] += int((done & trunc & (a > 0)).sum())
        moved = np.array([graphs[int(prev[ST["scene"]][e])][int(prev[ST["state"]][e]), int(rec["actions"][t][e])]
                          for e in range(E)])
        count["blocked"] += int((moved == -1).sum())
        count["other_scene"] += int((done & (tb[ST["scene"]] != scene_p)).sum())
        valid = (b >= 0) & (a >= 0)
        count["plus"] += int((valid & (p == 1)).sum())
        count["zero"] += int((valid & (p == 0)).sum())
        count["minus"] += int((valid & (p == -1)).sum())
        count["invalid"] += int((~valid).sum())
        assert (p[~valid] == 0).all()
        prev = tb
        for mask, table in events.get(t, ()):
            if mask is not None:  # a reset into another scene (with auto-reset off the only ones)
                count["other_scene"] += int(((mask != 0) & (table[ST["scene"]] != record.scene)).sum())
            sr.progress_refresh(geos, table[ST["scene"]], table[ST["state"]], table[ST["goal"]], record, mask)
            count["masked_reset" if mask is not None else "set_state"] += 1
            prev = table
    return np.stack(want), count


def check(tables_, rec, E):
    want, count = restate(tables_, rec, E)
    got = rec["prog"]
    assert got.dtype == np.int32 and got.shape == want.shape
    for t in range(len(want)):
        assert np.array_equal(got[t], want[t]), (t, got[t], want[t])
    assert rec["flags"] == 0
    return count


@pytest.mark.parametrize("autoreset", [True, False])
@pytest.mark.parametrize("E", [1, 37, 300])
def test_progress_matches_restatement(scenes, tables, E, autoreset):
    """vn_step (u8). 37 envs: a ragged block; 300: a second workgroup. The trajectory of more than
    one env contains every case of the rule."""
    rec = run("u8", scenes, E, True, autoreset)
    count = check(tables, rec, E)
    print("SHAPECASES E=%d autoreset=%s %s" % (E, autoreset, count))
    assert count["masked_reset"] > 0 and count["set_state"] == 1
    if E > 1:
        for k in ("success", "truncated_far", "blocked", "plus", "zero", "minus", "invalid", "other_scene"):
            assert count[k] > 0, (k, count)
    assert len({s.n_states for s in scenes}) >= 2


@pytest.mark.parametrize("autoreset", [True, False])
@pytest.mark.parametrize("route", ROUTES[1:])
def test_progress_on_every_route(scenes, tables, route, autoreset):
    E = 37
    rec = run(route, scenes, E, True, autoreset)
    count = check(tables, rec, E)
    for k in ("success", "truncated_far", "blocked", "plus", "zero", "minus", "invalid"):
        assert count[k] > 0, (k, count)
    assert {"distance_before", "progress"} <= set(rec["info_keys"])


@pytest.mark.parametrize("route", ROUTES)
def test_every_other_output_is_bitwise_unchanged(scenes, route):
    E = 37
    on, off = run(route, scenes, E, True), run(route, scenes, E, False)
    assert set(on["info_keys"]) - set(off["info_keys"]) == {"distance_before", "progress"}
    assert set(on["out"]) == set(off["out"])
    for k in on["out"]:
        assert tn.same_bits(on["out"][k], off["out"][k]), k
    assert len(on["frames"]) == len(off["frames"]) and (len(on["frames"]) > 0) == (route not in ("index", "a2c"))
    for a, b in zip(on["frames"], off["frames"]):
        assert tn.same_bits(a, b)
    assert len(on["events"]) == len(off["events"])
    for (_, _, ta), (_, _, tb) in zip(on["events"], off["events"]):
        assert np.array_equal(ta, tb)


def test_env_own_buffers_and_output_redirection(scenes, tables):
    """info's distance_before / progress are the env's own buffers until the outputs are pointed
    elsewhere; all-None points them back; a NULL output is not written."""
    E = 37
    env = make_env("u8", scenes, E, True)
    env.reset()
    graphs, geos = tables
    record = sr.ProgressRecord(E)
    tb = env.get_state().cpu().numpy()
    sr.progress_refresh(geos, tb[ST["scene"]], tb[ST["state"]], tb[ST["goal"]], record)
    acts = actions_of(E, 12)
    mine = [torch.full((E,), -99, dtype=torch.int32, device="cuda") for _ in range(2)]
    for t, a in enumerate(acts):
        if t == 4:
            env.set_nav_progress_outputs(mine[0], mine[1])  # before, after; no progress output
        if t == 8:
            env.set_nav_progress_outputs(None, None)
        _, _, d, info = env.step(tn.dev(a))
        tb = env.get_state().cpu().numpy()
        b, af, p = sr.progress_ref(geos, tb[ST["scene"]], tb[ST["state"]], tb[ST["goal"]], d.cpu().numpy(),
                                   info["truncated"].cpu().numpy(), info["terminal_state"].cpu().numpy(), record)
        if 4 <= t < 8:
            assert np.array_equal(mine[0].cpu().numpy(), b) and np.array_equal(mine[1].cpu().numpy(), af)
            assert np.array_equal(info["progress"].cpu().numpy(), kept[1])  # not written
            assert np.array_equal(info["distance_before"].cpu().numpy(), kept[0])
        else:
            assert np.array_equal(info["distance_before"].cpu().numpy(), b)
            assert np.array_equal(info["progress"].cpu().numpy(), p)
            kept = (b, p)
    with pytest.raises(ValueError):
        env.set_nav_progress_outputs(torch.zeros(E + 1, dtype=torch.int32, device="cuda"), None)
    with pytest.raises(ValueError):
        env.set_nav_progress_outputs(None, torch.zeros(E, dtype=torch.float32, device="cuda"))
    env.close()


def collect(env, acts, bufs):
    out = []
    for a in acts:
        _, r, d, info = env.step(tn.dev(a))
        out.append(torch.cat([r.view(torch.int32), d.to(torch.int32), info["state"]] + list(bufs)))
    return torch.stack(out).cpu().numpy()


def test_state_round_trip(scenes):
    E = 37
    acts = actions_of(E, 40)

    def fresh():
        env = make_env("u8", scenes, E, True)
        bufs = [torch.full((E,), -99, dtype=torch.int32, device="cuda") for _ in range(3)]
        env.set_nav_progress_outputs(*bufs)
        return env, bufs

    env, bufs = fresh()
    collect(env, acts[:20], bufs)
    saved = (env.get_state().clone(), env.get_episode_returns().clone(), env.get_nav_state().clone(),
             env.get_nav_progress_state().clone())
    assert saved[3].shape == (3, E) and saved[3].dtype == torch.int32
    tb = saved[0].cpu().numpy()
    assert np.array_equal(saved[3][:2].cpu().numpy(), tb[[ST["scene"], ST["goal"]]])
    want = collect(env, acts[20:], bufs)
    env.close()
    env, bufs = fresh()
    collect(env, acts[:3], bufs)  # another position: the restore must replace all of it
    env.set_state(saved[0])
    env.set_episode_returns(saved[1])
    env.set_nav_state(saved[2])
    env.set_nav_progress_state(saved[3])
    assert torch.equal(env.get_nav_progress_state(), saved[3])
    got = collect(env, acts[20:], bufs)
    assert np.array_equal(got, want)
    # a record that differs from the states is what the next step reports as `before`
    odd = saved[3].clone()
    odd[2] = 7
    env.set_nav_progress_state(odd)
    collect(env, acts[:1], bufs)
    assert (bufs[0].cpu().numpy() == 7).all()
    with pytest.raises(ValueError):
        env.set_nav_progress_state(torch.zeros((3, E + 1), dtype=torch.int32))
    env.close()


def test_captured_step_a2c_writes_the_slots(scenes, tables):
    """A captured vn_step_a2c keeps the output pointers it was recorded with: every replay
    writes the same slots, with the values of the eager run."""
    E = 37
    acts = actions_of(E, 30)
    eager = run("a2c", scenes, E, True)["prog"]  # the same actions_of(E) prefix
    env = make_env("a2c", scenes, E, True)
    env.reset()
    st = Stepper("a2c", env, E)
    slots = torch.full((3, E), -99, dtype=torch.int32, device="cuda")
    env.set_nav_progress_outputs(slots[0], slots[1], slots[2])
    lg = torch.zeros((E, 8), dtype=torch.float32, device="cuda")

    def logits(a):
        x = np.zeros((E, 8), dtype=np.float32)
        x[np.arange(E), a] = 1e4
        lg.copy_(torch.as_tensor(x))

    for t in range(3):
        logits(acts[t])
        st.pol.copy_(lg)
        env.step_a2c(st.s, st.reward, st.done, st.state)
        assert np.array_equal(slots.cpu().numpy(), eager[t])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st.pol.copy_(lg)
        env.step_a2c(st.s, st.reward, st.done, st.state)
    other = torch.full((3, E), -5, dtype=torch.int32, device="cuda")
    env.set_nav_progress_outputs(other[0], other[1], other[2])  # the graph holds the recorded pointers
    for t in range(3, 12):
        logits(acts[t])
        g.replay()
        assert np.array_equal(slots.cpu().numpy(), eager[t]), t
    assert (other.cpu().numpy() == -5).all()
    assert env.error_flags() == 0
    env.close()


def test_abi_state_rules(scenes):
    """VN_ESTATE without nav and without progress; vn_nav_enable (either way) switches progress
    off; the stand-in terminal_state serves a caller that set no info buffers."""
    import vnav
    from vnav import _lib
    lib = _lib.load()
    E = 37
    env = vnav.VectorEnv(scenes, E, seed=SEED, max_episode_steps=LIMIT, tasks=TASKS)
    buf = torch.zeros((3, E), dtype=torch.int32, device="cuda")
    st = _lib.stream_ptr(env.device)
    assert lib.vn_nav_progress(env._ctx, 1) == VN_ESTATE
    assert lib.vn_set_nav_progress_outputs(env._ctx, None, None, None) == VN_ESTATE
    with pytest.raises(_lib.VnavError):
        env.set_nav_progress(True)
    with pytest.raises(ValueError):
        vnav.VectorEnv(scenes, E, nav_progress=True)
    env.set_nav_info(True)
    assert lib.vn_get_nav_progress_state(env._ctx, _lib.ptr(buf), st) == VN_ESTATE
    env.set_nav_progress(True)
    assert env.nav_progress and "progress" in env._info
    assert lib.vn_get_nav_progress_state(env._ctx, _lib.ptr(buf), st) == 0
    env.set_nav_info(True)  # re-enabled: progress is off again
    assert not env.nav_progress and "progress" not in env._info and "distance_before" not in env._info
    assert lib.vn_get_nav_progress_state(env._ctx, _lib.ptr(buf), st) == VN_ESTATE
    assert lib.vn_set_nav_progress_state(env._ctx, _lib.ptr(buf), st) == VN_ESTATE
    env.set_nav_progress(True)
    env.set_nav_info(False)
    assert not env.nav_progress
    assert lib.vn_nav_progress(env._ctx, 1) == VN_ESTATE
    with pytest.raises(_lib.VnavError):
        env.get_nav_progress_state()
    # the raw ABI with no info buffers: the progress state's own terminal_state stands in
    env.set_nav_info(True)
    env.set_nav_progress(True)
    _lib.check(lib.vn_set_info_buffers(env._ctx, None, None, None, None, None, None), "vn_set_info_buffers")
    out = torch.full((3, E), -99, dtype=torch.int32, device="cuda")
    env.set_nav_progress_outputs(out[0], out[1], out[2])
    geos = [nr.geodesic(s.graph) for s in scenes]
    record = sr.ProgressRecord(E)
    tb = env.get_state().cpu().numpy()
    sr.progress_refresh(geos, tb[ST["scene"]], tb[ST["state"]], tb[ST["goal"]], record)
    done = torch.zeros(E, dtype=torch.bool, device="cuda")
    state = torch.zeros(E, dtype=torch.int32, device="cuda")
    trunc_seen = 0
    for t, a in enumerate(actions_of(E, 14)):
        elapsed = tb[ST["elapsed"]]
        _lib.check(lib.vn_step(env._ctx, _lib.ptr(tn.dev(a)), None, None, None, _lib.ptr(done), _lib.ptr(state), st),
                   "vn_step")
        d = done.cpu().numpy()
        tb2 = env.get_state().cpu().numpy()
        # without info buffers: truncated = done at the limit off the goal, terminal_state = the
        # state the walk reached, restated from the table before the step
        graph_next = np.array([scenes[int(tb[ST["scene"]][e])].graph[int(tb[ST["state"]][e]), int(a[e])]
                               for e in range(E)])
        reached = np.where(graph_next == -1, tb[ST["state"]], graph_next)
        trunc = d & (reached != tb[ST["goal"]]) & (elapsed + 1 >= LIMIT)
        trunc_seen += int(trunc.sum())
        b, af, p = sr.progress_ref(geos, tb2[ST["scene"]], tb2[ST["state"]], tb2[ST["goal"]], d, trunc, reached,
                                   record)
        assert np.array_equal(out.cpu().numpy(), np.stack([b, af, p])), t
        tb = tb2
    assert trunc_seen > 0
    env.close()
