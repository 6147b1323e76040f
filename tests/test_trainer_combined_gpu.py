"""A2CTrainer with every kind of per-env state live at once — nav metrics, the expert term, an
adapting geodesic curriculum, annealed shaping with GAE, an LSTM, and the UNREAL losses replayed
from the ring: a checkpoint resumes bit for bit, and a fixed-episode evaluation between two
updates leaves the second as it would have been. Both guard the order in which the per-env tables
are restored (vnav/checkpoint.py ENV_STATE); no single-feature test has all five live.

4 envs x 5 steps, BigHouseModel's heads on 84 x 84 frames (the frame its 20-cell pixel control
needs) and one replayed sequence. The raw vectors are compared bitwise, so the shape keeps every
statistic in them free of summation order: the pixel-control loss sums one partial per 256 cells
with float atomics, S x 20 x 20 = 400 cells are two partials, and a sum of two is the same in
either order (at S = 4 on the 42-cell heads it is 28 partials and differs in the last bits from
run to run, tests/test_replay_gpu.py); every other float statistic here comes from one block."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

E, T, LIMIT = 4, 5, 6
# down just under up: every full window moves the level (test_geo_curriculum_trainer_gpu.py)
CUR = dict(level=3, mode=1, window=4, up=0.5, down=0.49, step=1, level_min=1)
ENV_TABLES = ("get_state", "get_episode_returns", "get_nav_state", "curriculum_state", "get_nav_progress_state")


def make():
    import vnav
    env = vnav.VectorEnv([vnav.synthetic_scene(0, grid=6)], E, seed=5, max_episode_steps=LIMIT)
    return vnav.A2CTrainer(env, num_steps=T, seed=9, max_time_steps=1e6, recurrent=True, arch="bighouse", unreal=True,
                           unreal_envs=1, unreal_source="replay", replay_size=2, nav_metrics=True, expert_weight=0.5,
                           geo_curriculum=CUR, shaping_weight=0.8, shaping_anneal_steps=200, gae_lambda=0.95)


def raw_step(tr):
    return tr.step(sync=False)["raw"].clone()


def state(tr):
    torch.cuda.synchronize()
    out = dict(params=tr.params, square_avg=tr.square_avg, replay_rows=tr.replay_rows, replay_meta=tr.replay_meta,
               sched=tr.sched)
    out.update({"ur_" + k: v for k, v in tr.ur.items()})
    out.update({k: getattr(tr.env, k)() for k in ENV_TABLES})
    out.update({k: getattr(tr, k) for k in tr._RECURRENT_STATE})
    return {k: v.detach().clone() for k, v in out.items()}


def assert_raws_same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        bad = (g != w).nonzero().flatten().tolist()
        assert not bad, "update %d, raw%s: %s != %s" % (k, bad, g[bad].tolist(), w[bad].tolist())


def assert_same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def straight():
    """Four updates in a row: the checkpoint and the state after two, the parameters after three,
    the state after four, and the raw vectors of all four."""
    tr = make()
    raws = [raw_step(tr) for _ in range(2)]
    sd, mid = copy.deepcopy(tr.state_dict()), state(tr)
    raws.append(raw_step(tr))
    torch.cuda.synchronize()
    third = tr.params.clone()
    raws.append(raw_step(tr))
    assert tr.env.error_flags() == 0
    return dict(sd=sd, raws=raws, mid=mid, third=third, end=state(tr))


def test_every_kind_of_state_is_live(straight):
    sd, raws = straight["sd"], straight["raws"]
    for key in ("env_state", "env_ep_return", "env_nav", "env_curriculum", "env_nav_progress", "replay_rows",
                "replay_meta", "ur_shape_dist", "h0"):
        assert key in sd, key
    # base 12 + nav 4 + expert 4 + curriculum 1 + shaping 3, fp64 with shaping on
    assert all(r.shape == (24,) and r.dtype == torch.float64 for r in raws)
    assert len({float(r[20]) for r in raws}) > 1  # the curriculum level moved
    assert float(raws[0][23]) == 0 and float(raws[3][23]) == 3 * E * T  # the anneal's step count runs
    assert not torch.equal(straight["mid"]["get_nav_progress_state"], straight["end"]["get_nav_progress_state"])


def test_combined_resume_is_bitwise(straight):
    b = make()
    raw_step(b)  # somewhere else: the load must replace it
    b.load_state_dict(straight["sd"])
    assert_same(state(b), straight["mid"])
    raws = [raw_step(b) for _ in range(2)]
    assert_same(state(b), straight["end"])
    assert_raws_same(raws, straight["raws"][2:])
    assert b.env.error_flags() == 0


@pytest.mark.parametrize("policy", ["sample", "greedy"])
def test_evaluation_between_two_updates_changes_neither(straight, policy):
    import vnav
    tr = make()
    raws = [raw_step(tr) for _ in range(2)]
    eps = vnav.EpisodeSet.sample(tr.env, 3, buckets=((1, 3), (4, None)), seed=2)
    res = tr.evaluate_episodes(eps, policy=policy, seed=5)
    assert res["episodes"] == len(eps) == 6
    assert_same(state(tr), straight["mid"])
    raws.append(raw_step(tr))
    assert_raws_same(raws, straight["raws"][:3])
    torch.cuda.synchronize()
    assert torch.equal(tr.params, straight["third"]) and tr.env.error_flags() == 0

