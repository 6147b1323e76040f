"""A2CTrainer(novelty_weight=..., first_visit_weight=..., novelty_anneal_steps=...): with both
weights 0 the trainer is bitwise the one built without the arguments; with them on, the visit
histories of the index-only rollout and rewards_aug, the input of the returns kernel, are the
restatement of tests/visit_ref.py on the trainer's own states and table, and everything else
stays on the env's reward; the captured hipGraph equals eager by bits with the anneal on; a resume
is exact, table, records and bitmaps included; evaluate_episodes and evaluate leave the visit
state as it was; it composes with shaping, GAE, the expert loss and the curriculum; update(None),
the inline UNREAL pass and the stream guard behave as without it. 4 envs x 5 steps, LSTM, on two
84 x 84 synthetic scenes of different state counts."""
import copy
import os
import warnings

import numpy as np
import pytest
import torch

import shaping_ref as sr
import visit_ref as vr

pytestmark = pytest.mark.gpu

E, T, LIMIT = 4, 5, 6
ST_SCENE, ST_STATE = 0, 1
BASE_KEYS = {"step", "updates", "value_loss", "action_loss", "entropy", "loss", "episodes", "reward",
             "episode_length", "grad_norm", "return_mean", "fps"}
NOVELTY_KEYS = {"novelty_bonus", "first_visit_rate", "states_seen"}
ON = dict(novelty_weight=0.1, first_visit_weight=0.05)


def _vnav():
    import vnav
    return vnav


def make(limit=LIMIT, env_seed=5, **kw):
    vnav = _vnav()
    env = vnav.VectorEnv([vnav.synthetic_scene(0, grid=6), vnav.synthetic_scene(1, grid=5)], E, seed=env_seed,
                         max_episode_steps=limit)
    opts = dict(num_steps=T, seed=9, max_time_steps=1e6, recurrent=True)
    opts.update(kw)
    return vnav.A2CTrainer(env, **opts)


def table_of(env):
    tb = env.get_state().cpu().numpy()
    return tb[ST_SCENE], tb[ST_STATE]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def restated_aug(tr, steps, anneal=0, w=ON):
    """rewards_aug from the trainer's own histories and the env's live table."""
    C = tr.env.visit_cells()[2]
    count = tr.env.get_visit_state()[:C].cpu().numpy().view(np.uint32)
    return vr.novelty_rewards32(tr.rewards.cpu().numpy(), tr.visit_cell.cpu().numpy(), tr.visit_first.cpu().numpy(),
                                count, w["novelty_weight"], w["first_visit_weight"], steps=steps, anneal_steps=anneal)


def test_off_is_todays_trainer():
    runs = []
    for kw in ({}, dict(novelty_weight=0.0, first_visit_weight=0.0, novelty_anneal_steps=0)):
        tr = make(**kw)
        raws = [tr.step(sync=False)["raw"].clone() for _ in range(3)]
        torch.cuda.synchronize()
        runs.append((tr, raws))
    (a, ra), (b, rb) = runs
    assert torch.equal(a.params, b.params) and torch.equal(a.square_avg, b.square_avg)
    assert torch.equal(a.returns, b.returns)
    for x, y in zip(ra, rb):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))
    for tr in (a, b):
        assert not tr.novelty and not tr.env.visit_counts and "novelty" not in tr._metric_layout
        assert not any(hasattr(tr, k) for k in ("rewards_aug", "visit_cell", "visit_first", "novelty_stats"))
    assert set(b.step()) == BASE_KEYS
    for bad in (dict(novelty_weight=-0.1), dict(first_visit_weight=-1.0), dict(novelty_weight=0.1, novelty_anneal_steps=-1)):
        with pytest.raises(ValueError):
            make(**bad)


def test_histories_and_returns_input_vs_restatement():
    anneal = 50  # 20 env steps per update: the weights are 1, 0.6 and 0.2 of their start
    tr = make(novelty_anneal_steps=anneal, **ON)
    env = tr.env
    assert tr.novelty and env.visit_counts and not env.nav_info
    assert tr.visit_cell.shape == (T, E) and tr.visit_first.dtype == torch.bool
    vs = vr.VisitState([s.n_states for s in env.scenes], E)
    vr.visit_start(vs, *table_of(env))
    assert np.array_equal(env.get_visit_state().cpu().numpy(), vs.packed())
    seen = []
    step = env.step_a2c

    def recording_step(*a):
        step(*a)
        seen.append((env.get_state().clone(), env._info["terminal_state"].clone()))

    env.step_a2c = recording_step
    dones = firsts = 0
    for r in range(3):
        del seen[:]
        m = tr.step()
        torch.cuda.synchronize()
        assert set(m) == BASE_KEYS | NOVELTY_KEYS
        d = tr.dones.cpu().numpy()
        cell = np.zeros((T, E), np.int32)
        first = np.zeros((T, E), np.uint8)
        for t in range(T):
            tb = seen[t][0].cpu().numpy()
            cell[t], first[t], _ = vr.visit_step(vs, tb[ST_SCENE], tb[ST_STATE], d[t], seen[t][1].cpu().numpy())
        assert np.array_equal(tr.visit_cell.cpu().numpy(), cell), r
        assert np.array_equal(tr.visit_first.cpu().numpy().astype(np.uint8), first), r
        assert np.array_equal(env.get_visit_state().cpu().numpy(), vs.packed()), r
        rewards = tr.rewards.cpu().numpy()
        want, st = vr.novelty_rewards32(rewards, cell, first, vs.count, steps=r * T * E, anneal_steps=anneal,
                                        w_count=ON["novelty_weight"], w_first=ON["first_visit_weight"])
        assert np.array_equal(bits(tr.rewards_aug.cpu().numpy()), bits(want)), r
        assert bits(tr.novelty_stats.cpu().numpy())[3] == bits(st["wc"])
        assert st["wc"] == vr.anneal_weight(0.1, r * T * E, anneal) and st["wc"] > 0
        # rewards_aug is what the returns kernel read; the env's reward stays its own
        ret = sr.returns_ex32(want, d, tr.boot_out.cpu().numpy(), None, tr.A, tr.gamma)
        assert ret.tobytes() == tr.returns.cpu().numpy().reshape(T, E).tobytes()
        assert set(np.unique(rewards)) <= {0.0, 1.0} and (want != rewards).any()
        assert abs(m["novelty_bonus"] - st["added"] / (T * E)) <= 1e-6 * st["added"] / (T * E)
        assert m["first_visit_rate"] == st["firsts"] / (T * E) and m["states_seen"] == vs.stats()[0]
        dones += int(d.sum())
        firsts += int(first.sum())
    assert dones > 0 and 0 < firsts < 3 * T * E
    assert env.error_flags() == 0
    # outside a rollout the steps write the env's own buffers again
    env.step_a2c = step
    keep = tr.visit_cell.clone()
    env.step(torch.zeros(E, dtype=torch.int32, device="cuda"), gather=False)
    assert torch.equal(tr.visit_cell, keep)


def test_graph_is_bit_identical_to_eager():
    """20 env-steps per update against a horizon of 70: the weights change at every update and
    are 0 at the fifth, which a captured update shows only if it reads them on the device."""
    horizon = 70
    want = [float(vr.anneal_weight(0.1, k * E * T, horizon)) for k in range(5)]
    assert len(set(want)) == 5 and want[-1] == 0.0
    runs = {}
    for graph in (False, True):
        tr = make(novelty_anneal_steps=horizon, cuda_graph=graph, **ON)
        ms, wc = [], []
        for _ in range(5):
            ms.append(tr.step())
            wc.append(float(tr.novelty_stats[3]))
        torch.cuda.synchronize()
        assert wc == want, (graph, wc)
        runs[graph] = (tr.params.clone(), tr.square_avg.clone(), tr.rewards_aug.clone(), tr.returns.clone(),
                       tr.visit_cell.clone(), tr.visit_first.clone(), tr.env.get_visit_state().clone(),
                       [[m[k] for k in sorted(NOVELTY_KEYS)] for m in ms])
    for a, b in zip(runs[True][:7], runs[False][:7]):
        assert torch.equal(a, b)
    assert runs[True][7] == runs[False][7]
    assert runs[True][7][-1][sorted(NOVELTY_KEYS).index("novelty_bonus")] == 0.0


def test_resume_is_exact():
    kw = dict(novelty_anneal_steps=2000, limit=4, **ON)
    a = make(**kw)
    a.step()
    a.step()
    sd = copy.deepcopy(a.state_dict())
    assert sd["env_visits"].dtype == torch.int32 and sd["env_visits"].numel() == a.env._visit_words()
    a.step()
    b = make(**kw)
    b.step()  # somewhere else: the load must replace it
    b.load_state_dict(sd)
    assert torch.equal(b.env.get_visit_state().cpu(), sd["env_visits"])
    b.step()
    torch.cuda.synchronize()
    assert torch.equal(b.params, a.params) and torch.equal(b.square_avg, a.square_avg)
    assert torch.equal(b.rewards_aug, a.rewards_aug) and torch.equal(b.returns, a.returns)
    assert torch.equal(b.env.get_visit_state(), a.env.get_visit_state())
    # a checkpoint without the visit state: a warning, the records start from the restored states
    del sd["env_visits"]
    c = make(**kw)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        c.load_state_dict(sd)
    assert any("visit" in str(x.message) for x in caught)
    vs = vr.VisitState([s.n_states for s in c.env.scenes], E)
    vr.visit_start(vs, *table_of(c.env), add=False)
    C = vs.C
    assert np.array_equal(c.env.get_visit_state().cpu().numpy()[C:], vs.packed()[C:])


def test_evaluations_leave_the_visit_state():
    vnav = _vnav()
    tr = make(nav_metrics=True, **ON)
    tr.step()
    tr.step()
    torch.cuda.synchronize()
    before = tr.env.get_visit_state().clone()
    steps = tr.novelty_steps.clone()
    eps = vnav.EpisodeSet.sample(tr.env, 2, buckets=((1, 3), (4, None)), seed=2)
    for policy in ("sample", "greedy"):
        res = tr.evaluate_episodes(eps, policy=policy, seed=5)
        assert res["episodes"] == len(eps)
        assert torch.equal(tr.env.get_visit_state(), before) and torch.equal(tr.novelty_steps, steps)
    # and it goes on exactly as a trainer that was never evaluated
    other = make(nav_metrics=True, **ON)
    for _ in range(2):
        other.step()
    tr.step()
    other.step()
    torch.cuda.synchronize()
    assert torch.equal(tr.params, other.params) and torch.equal(tr.rewards_aug, other.rewards_aug)
    assert torch.equal(tr.env.get_visit_state(), other.env.get_visit_state())
    # evaluate(): the table counts the evaluation alone meanwhile, and comes back
    before = tr.env.get_visit_state().clone()
    res = tr.evaluate(episodes=2)
    total = sum(s.n_states for s in tr.env.scenes)
    assert 0 < res["states_seen"] <= total and res["coverage"] == res["states_seen"] / total
    assert torch.equal(tr.env.get_visit_state(), before)


def test_composes_with_shaping_gae_expert_and_curriculum():
    runs = {}
    for graph in (False, True):
        tr = make(shaping_weight=0.5, gae_lambda=0.95, expert_weight=0.3, nav_metrics=True,
                  geo_curriculum=dict(level=2, window=4), cuda_graph=graph, **ON)
        for r in range(3):
            m = tr.step()
            torch.cuda.synchronize()
            assert NOVELTY_KEYS | {"shaping_reward", "expert_loss", "curriculum_level", "success_rate"} <= set(m)
            want, st = restated_aug(tr, r * T * E)
            assert np.array_equal(bits(tr.rewards_aug.cpu().numpy()), bits(want)), (graph, r)
            # the shaped lambda-return is formed on rewards_aug, not on the env's reward
            ref, M = sr.returns_ex64(want, tr.dones.cpu().numpy(), tr.boot_out.cpu().numpy(), tr.out.cpu().numpy(),
                                     tr.shape_dist.cpu().numpy(), tr.A, tr.gamma, 0.95, w=np.float32(0.5))
            err = np.abs(tr.returns.cpu().numpy().reshape(T, E).astype(np.float64) - ref).max()
            assert err <= 2 * sr.K_GAE_SHAPED * T * 2.0 ** -24 * M
            assert m["states_seen"] == int(tr.env.visit_stats()[0])
        runs[graph] = (tr.params.clone(), tr.square_avg.clone(), tr.rewards_aug.clone(), tr.returns.clone(),
                       tr.env.get_visit_state().clone())
    for a, b in zip(runs[True], runs[False]):
        assert torch.equal(a, b)


def test_inline_pass_stream_guard_and_update_without_batch():
    """With the UNREAL losses on replayed sequences: the ring and the reward-prediction labels
    keep the env's reward; the inline pass, the stream guard and update(None) change nothing."""
    from test_rp_skewed_trainer_gpu import _same_state, _trainer

    def run(inline=False, debug=False, bare=False):
        if inline:
            os.environ["VN_UNREAL_INLINE"] = "1"
        try:
            tr = _trainer(E=4, S=4, rp_sampling="sequence", **ON)
        finally:
            os.environ.pop("VN_UNREAL_INLINE", None)
        assert tr._unreal_inline == inline
        tr.debug_streams = debug
        for _ in range(4):
            if bare:  # update(None): the push and the draws happen inside the update
                tr.rollout()
                tr.update(None)
            else:
                tr.step(sync=True)
        torch.cuda.synchronize()
        return tr

    a = run()
    for other in (run(inline=True), run(debug=True), run(bare=True)):
        _same_state(a, other)
        assert torch.equal(a.rewards_aug, other.rewards_aug) and torch.equal(a.returns, other.returns)
        assert torch.equal(a.env.get_visit_state(), other.env.get_visit_state())
    env_rewards = {float(np.float32(r)) for r in a.env.scenes[0].rewards} | {0.0}
    assert {float(r) for r in np.unique(a.ur["rewards"].cpu().numpy())} <= env_rewards
    assert (a.rewards_aug != a.rewards).any()
    names = [k for k, _ in a._main_owned()]
    for k in ("rewards_aug", "novelty_stats", "visit_seen"):
        assert k in names
