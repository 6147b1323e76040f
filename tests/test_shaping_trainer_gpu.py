"""A2CTrainer(shaping_weight=..., gae_lambda=...): the per-step distance slots of the index-only
rollout against tests/shaping_ref.py on the states the rollout visited, the update's returns
against the restatement formed from the trainer's own buffers, and the trainer-level contracts:
a zero weight with lambda 1 changes nothing, the captured hipGraph is bit-identical to eager with
shaping, anneal and GAE on, a resume is exact, evaluate_episodes leaves the trainer as it was, and
the replay ring carries the distances. 16 envs x 5 steps on two 84 x 84 synthetic scenes of
different state counts (the policy needs 84 x 84 frames; the 16 x 16 scenes of nav_ref do not
fit it)."""
import copy
import warnings

import numpy as np
import pytest
import torch

import nav_ref as nr
import shaping_ref as sr

pytestmark = pytest.mark.gpu

E, T, LIMIT = 16, 5, 6
ST_SCENE, ST_STATE, ST_GOAL = 0, 1, 2
EPS24 = 2.0 ** -24
BASE_KEYS = {"step", "updates", "value_loss", "action_loss", "entropy", "loss", "episodes", "reward",
             "episode_length", "grad_norm", "return_mean", "fps"}
SHAPING_KEYS = {"shaping_reward", "shaping_weight"}


def _vnav():
    import vnav
    return vnav


def scenes():
    vnav = _vnav()
    return [vnav.synthetic_scene(0, grid=6), vnav.synthetic_scene(1, grid=5)]


def make(limit=LIMIT, env_seed=5, **kw):
    vnav = _vnav()
    env = vnav.VectorEnv(scenes(), E, seed=env_seed, max_episode_steps=limit)
    opts = dict(num_steps=T, seed=9, max_time_steps=1e6)
    opts.update(kw)
    return vnav.A2CTrainer(env, **opts)


def geos_of(tr):
    return [nr.geodesic(np.asarray(s.graph)) for s in tr.env.scenes]


def reference_returns(tr, w):
    """(float64 returns [T, E], M) from the trainer's own rollout buffers and the weight w."""
    return sr.returns_ex64(tr.rewards.cpu().numpy(), tr.dones.cpu().numpy(), tr.boot_out.cpu().numpy(),
                           tr.out.cpu().numpy(), tr.shape_dist.cpu().numpy() if tr.shaping else None, tr.A, tr.gamma,
                           tr.gae_lambda, w=w, gamma_phi=tr.shaping_gamma)


@pytest.mark.parametrize("recurrent", [False, True], ids=["ff", "lstm"])
@pytest.mark.parametrize("lam", [1.0, 0.95])
def test_slots_and_returns_vs_restatement(recurrent, lam):
    tr = make(recurrent=recurrent, shaping_weight=0.5, shaping_gamma=0.99, gae_lambda=lam, nav_metrics=True)
    assert tr.env.nav_progress and tr.shape_dist.shape == (T, 2, E) and tr.shape_dist.dtype == torch.int32
    assert len({s.n_states for s in tr.env.scenes}) == 2
    geos = geos_of(tr)
    record = sr.ProgressRecord(E)
    tb = tr.env.get_state().cpu().numpy()
    sr.progress_refresh(geos, tb[ST_SCENE], tb[ST_STATE], tb[ST_GOAL], record)
    seen = []
    step = tr.env.step_a2c

    def recording_step(*a):
        step(*a)
        seen.append((tr.env.get_state().clone(), tr.env._info["truncated"].clone(),
                     tr.env._info["terminal_state"].clone()))

    tr.env.step_a2c = recording_step
    dones = truncs = 0
    for r in range(3):
        del seen[:]
        m = tr.step()
        torch.cuda.synchronize()
        assert set(m) == BASE_KEYS | SHAPING_KEYS | {"success_rate", "spl"}
        want = np.zeros((T, 2, E), dtype=np.int32)
        d = tr.dones.cpu().numpy()
        for t in range(T):
            tb = seen[t][0].cpu().numpy()
            b, a, _ = sr.progress_ref(geos, tb[ST_SCENE], tb[ST_STATE], tb[ST_GOAL], d[t], seen[t][1].cpu().numpy(),
                                      seen[t][2].cpu().numpy(), record)
            want[t, 0], want[t, 1] = b, a
            truncs += int((d[t] & (seen[t][1].cpu().numpy() != 0)).sum())
        dones += int(d.sum())
        got = tr.shape_dist.cpu().numpy()
        assert np.array_equal(got, want), (r, got, want)
        ref, M = reference_returns(tr, np.float32(0.5))
        k = sr.K_NSTEP_SHAPED if lam == 1.0 else sr.K_GAE_SHAPED
        err = np.abs(tr.returns.cpu().numpy().reshape(T, E).astype(np.float64) - ref).max()
        print("SHAPEERR trainer returns lambda=%g worst %.3e bound %.3e" % (lam, err, 2 * k * T * EPS24 * M))
        assert err <= 2 * k * T * EPS24 * M
        if lam == 1.0:  # and the float32 restatement, operation for operation
            want32 = sr.returns_ex32(tr.rewards.cpu().numpy(), d, tr.boot_out.cpu().numpy(), got, tr.A, tr.gamma,
                                     w=0.5, gamma_phi=0.99)
            assert want32.tobytes() == tr.returns.cpu().numpy().reshape(T, E).tobytes()
        stats = sr.shaping_stats(got)
        assert list(tr.shape_stats.cpu().numpy()) == list(stats)
        assert m["shaping_weight"] == 0.5
        want_mean = 0.5 * (stats[0] - float(np.float32(0.99)) * stats[1]) / (T * E)
        assert abs(m["shaping_reward"] - want_mean) <= 1e-12 * max(1.0, abs(want_mean))
        # the env's reward stays the environment's own: the sparse goal reward
        assert set(np.unique(tr.rewards.cpu().numpy())) <= {0.0, 1.0}
    assert dones > 0 and truncs > 0
    assert tr.env.error_flags() == 0


def test_off_is_todays_trainer():
    """shaping_weight=0.0 with lambda 1 goes through vn_a2c_returns_ex and gives the default
    trainer's parameters by bits; the default trainer allocates nothing and enables nothing."""
    runs = {}
    for w in (None, 0.0):
        tr = make(shaping_weight=w, gae_lambda=1.0)
        ms = [tr.step() for _ in range(3)]
        torch.cuda.synchronize()
        runs[w] = (tr.params.clone(), tr.square_avg.clone(), tr.returns.clone(), ms, tr)
    off, on = runs[None], runs[0.0]
    for a, b in zip(on[:3], off[:3]):
        assert torch.equal(a, b)
    assert all(set(m) == BASE_KEYS for m in off[3])
    assert all(set(m) == BASE_KEYS | SHAPING_KEYS for m in on[3])
    tr = off[4]
    assert not tr.returns_ex and not hasattr(tr, "shape_dist") and not hasattr(tr, "shape_stats")
    assert not tr.env.nav_info and not tr.env.nav_progress
    assert on[4].returns_ex and on[4].env.nav_progress
    for a, b in zip(on[3], off[3]):
        for k in BASE_KEYS - {"fps"}:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k
        assert a["shaping_weight"] == 0.0 and a["shaping_reward"] == 0.0
    with pytest.raises(ValueError):
        make(gae_lambda=1.5)


@pytest.mark.parametrize("recurrent", [False, True], ids=["ff", "lstm"])
def test_graph_is_bit_identical_to_eager(recurrent):
    """80 env-steps per update against a horizon of 300: the weight changes at every update and
    is 0 at the fifth, which a captured update shows only if it reads the weight on the device."""
    w0, horizon = 0.8, 300
    want = [float(sr.anneal_weight(w0, k * E * T, horizon)) for k in range(5)]
    assert len(set(want)) == 5 and want[-1] == 0.0
    runs = {}
    for graph in (False, True):
        tr = make(recurrent=recurrent, shaping_weight=w0, shaping_gamma=0.99, shaping_anneal_steps=horizon,
                  gae_lambda=0.95, cuda_graph=graph)
        ms = [tr.step() for _ in range(5)]
        torch.cuda.synchronize()
        assert [m["shaping_weight"] for m in ms] == want, (graph, ms)
        runs[graph] = (tr.params.clone(), tr.square_avg.clone(), tr.shape_dist.clone(), tr.returns.clone(),
                       tr.shape_stats.clone(), [m["shaping_reward"] for m in ms])
    for a, b in zip(runs[True][:5], runs[False][:5]):
        assert torch.equal(a, b)
    assert runs[True][5] == runs[False][5]


@pytest.mark.parametrize("recurrent", [False, True], ids=["ff", "lstm"])
def test_resume_is_exact(recurrent):
    kw = dict(recurrent=recurrent, shaping_weight=0.8, shaping_anneal_steps=2000, gae_lambda=0.95, limit=4)
    a = make(**kw)
    a.step()
    a.step()
    sd = copy.deepcopy(a.state_dict())
    assert tuple(sd["env_nav_progress"].shape) == (3, E)
    a.step()
    a.step()
    b = make(**kw)
    b.step()  # somewhere else: the load must replace it
    b.load_state_dict(sd)
    assert torch.equal(b.env.get_nav_progress_state().cpu(), sd["env_nav_progress"])
    b.step()
    b.step()
    torch.cuda.synchronize()
    assert torch.equal(b.params, a.params) and torch.equal(b.square_avg, a.square_avg)
    assert torch.equal(b.shape_dist, a.shape_dist) and torch.equal(b.returns, a.returns)
    # a checkpoint without the record: a warning, and the record starts from the restored states
    del sd["env_nav_progress"]
    c = make(**kw)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        c.load_state_dict(sd)
    assert any("progress" in str(x.message) for x in caught)
    tb = c.env.get_state().cpu().numpy()
    record = sr.ProgressRecord(E)
    sr.progress_refresh(geos_of(c), tb[ST_SCENE], tb[ST_STATE], tb[ST_GOAL], record)
    assert np.array_equal(c.env.get_nav_progress_state().cpu().numpy(), record.table())


def test_evaluate_episodes_leaves_the_trainer_as_it_was():
    vnav = _vnav()
    tr = make(recurrent=True, shaping_weight=0.5, gae_lambda=0.95, nav_metrics=True)
    tr.step()
    tr.step()
    torch.cuda.synchronize()

    def snapshot():
        out = dict(params=tr.params, square_avg=tr.square_avg, env=tr.env.get_state(),
                   ret=tr.env.get_episode_returns(), nav=tr.env.get_nav_state(),
                   progress=tr.env.get_nav_progress_state(), sched=tr.sched, shape_steps=tr.shape_steps)
        for k in tr._RECURRENT_STATE:
            out[k] = getattr(tr, k)
        return {k: v.clone() for k, v in out.items()}

    before = snapshot()
    eps = vnav.EpisodeSet.sample(tr.env, 2, buckets=((1, 3), (4, None)), seed=2)
    for policy in ("sample", "greedy"):
        res = tr.evaluate_episodes(eps, policy=policy, seed=5)
        assert res["episodes"] == len(eps)
    after = snapshot()
    for k in before:
        assert torch.equal(before[k], after[k]), k
    # and it goes on exactly as a trainer that was never evaluated
    other = make(recurrent=True, shaping_weight=0.5, gae_lambda=0.95, nav_metrics=True)
    for _ in range(2):
        other.step()
    tr.step()
    other.step()
    torch.cuda.synchronize()
    assert torch.equal(tr.params, other.params) and torch.equal(tr.shape_dist, other.shape_dist)
    assert torch.equal(tr.returns, other.returns)


def test_replay_ring_carries_the_distances():
    """unreal_source='replay' with a one-slot ring draws the rollout just pushed: the drawn
    slot's distances are the first S envs' of shape_dist, and the replayed value replay's returns
    are the restatement on the drawn slot under the current weight."""
    vnav = _vnav()
    from test_unreal_gpu import _unreal_env
    S = 8
    tr = vnav.A2CTrainer(_unreal_env(E, seed=5), num_steps=T, seed=3, max_time_steps=1e9, recurrent=True, unreal=True,
                         unreal_envs=S, unreal_source="replay", replay_size=1, shaping_weight=0.5,
                         shaping_anneal_steps=1000, gae_lambda=0.95)
    assert len(tr._replay_segs) == 15
    for r in range(2):
        m = tr.step()
        torch.cuda.synchronize()
        dist = tr.shape_dist.cpu().numpy()
        drawn = tr.ur_cur["shape_dist"].cpu().numpy()
        assert drawn.shape == (T, 2, S) and np.array_equal(drawn, dist[:, :, :S])
        assert np.array_equal(tr.ur["shape_dist"][0].cpu().numpy(), drawn)
        w = sr.anneal_weight(0.5, r * E * T, 1000)
        assert m["shaping_weight"] == float(w)
        u = tr.ur_cur
        out = tr.ur_out.cpu().numpy()
        ref, M = sr.returns_ex64(u["rewards"].cpu().numpy(), u["dones"].cpu().numpy(), out[T * S:], out[:T * S],
                                 drawn, tr.A, tr.gamma, 0.95, w=w, gamma_phi=1.0)
        got = tr.ur_returns.cpu().numpy().reshape(T, S).astype(np.float64)
        assert np.abs(got - ref).max() <= 2 * sr.K_GAE_SHAPED * T * EPS24 * M
        assert list(tr.ur_shape_stats.cpu().numpy()) == list(sr.shaping_stats(drawn))
    # a checkpoint whose ring lacks the segment: the ring restarts empty, with a warning
    sd = copy.deepcopy(tr.state_dict())
    assert "ur_shape_dist" in sd
    del sd["ur_shape_dist"]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        tr.load_state_dict(sd)
    assert any("ring restarts empty" in str(x.message) and "shaping" in str(x.message) for x in caught)
    assert tr.replay_filled == 0
