"""The reward-skewed reward-prediction draw's restatement (tests/rp_sample_ref.py) against a second
one in plain Python loops, the skew it claims, the metric segment and the command-line flags. No GPU."""
import itertools
import math

import numpy as np
import pytest

import rp_sample_ref as rr
from oracle import philox
from test_metric_layout import EXPECTED, FLAGS


# ---- a second restatement: plain loops over (r, ts, e), nothing shared but Philox ----------------
def loop_candidates(rewards, dones, filled):
    R, T, S = len(rewards), len(rewards[0]), len(rewards[0][0])
    q0, q1 = [], []
    for r in range(min(filled, R)):
        for ts in range(2, T):
            for e in range(S):
                if dones[r][ts - 2][e] or dones[r][ts - 1][e]:
                    continue
                i = (r * (T - 2) + (ts - 2)) * S + e
                (q0 if float(rewards[r][ts][e]) == 0.0 else q1).append((i, r, ts, e))
    return q0, q1


def loop_sample(rewards, dones, rows, filled, count, skew, seed, ctr):
    R, T, S = len(rewards), len(rewards[0]), len(rewards[0][0])
    q = loop_candidates(rewards, dones, filled)
    thr = int(skew * 4294967296.0)
    out = []
    for j in range(count):
        x, y, z, _ = (int(v) for v in philox.philox4x32_10(j, ctr & 0xFFFFFFFF, ctr >> 32, 6, seed & 0xFFFFFFFF,
                                                           seed >> 32))
        k = 1 if x < thr else 0
        if not q[k]:
            k = 1 - k
        if not q[k]:
            out.append(([0, 0, 0], [0, 0, 0], -1, -1))
            continue
        i, r, ts, e = q[k][((y * 2 ** 32 + z) * len(q[k])) >> 64]
        rw = float(rewards[r][ts][e])
        out.append(([int(rows[r][0][(ts - 2 + m) * S + e]) for m in range(3)],
                    [int(rows[r][1][(ts - 2 + m) * S + e]) for m in range(3)],
                    0 if rw == 0.0 else (1 if rw > 0.0 else 2), i))
    return out, (len(q[0]), len(q[1]), sum(o[2] > 0 for o in out), sum(o[2] >= 0 for o in out))


def hand_ring(R, T, S, seed, named=True):
    """A random ring; ``named`` (S >= 4) plants the cases the rule names in slot 0: a -0.0 reward
    (env 0) and a negative one (env S - 1) at the end of qualifying windows, a window skipped for
    a done at ts - 2 (env 1) and one for a done at ts - 1 (env 2)."""
    rng = np.random.default_rng(seed)
    rew = np.where(rng.random((R, T, S)) < 0.3, 1.0, 0.0).astype(np.float32)
    don = rng.random((R, T, S)) < 0.15
    if named:
        rew[0, T - 1, 0] = -0.0
        don[0, T - 3, 0] = don[0, T - 2, 0] = False
        rew[0, 2, S - 1] = -0.75
        don[0, 0, S - 1] = don[0, 1, S - 1] = False
        don[0, 0, 1] = True  # window ts = 2 of env 1: a done at ts - 2
        don[0, 1, 1] = False
        don[0, T - 3, 2] = False
        don[0, T - 2, 2] = True  # window ts = T - 1 of env 2: a done at ts - 1
    rows = rng.integers(0, 5000, size=(R, 2, (T + 1) * S)).astype(np.int32)
    return rew, don, rows


# (capacity, T, S, filled): filled < capacity throughout, T = 3 twice
RINGS = [(3, 5, 4, 2), (4, 3, 4, 3), (2, 3, 5, 1), (5, 7, 4, 3), (3, 4, 6, 2)]


@pytest.mark.parametrize("k,shape", list(enumerate(RINGS)) + [(5, (2, 3, 1, 1)), (6, (3, 4, 2, 3))])
def test_restatement_equals_plain_loops(k, shape):
    R, T, S, filled = shape
    named = k < len(RINGS)
    rew, don, rows = hand_ring(R, T, S, 100 + k, named)
    q = rr.candidates(rew, don, filled)
    lq = loop_candidates(rew.tolist(), don.tolist(), filled)
    assert [c[0] for c in lq[0]] == q[0].tolist() and [c[0] for c in lq[1]] == q[1].tolist()
    if named:  # the named cases are where the rule puts them
        assert filled < R and np.signbit(rew[0, T - 1, 0]) and rew[0, T - 1, 0] == 0
        assert (T - 3) * S + 0 in q[0] and 0 * S + S - 1 in q[1]  # -0.0 counts as zero, a negative reward does not
        both = set(q[0].tolist()) | set(q[1].tolist())
        assert 0 * S + 1 not in both and (T - 3) * S + 2 not in both  # the two skipped windows
    for skew, ctr, count in ((0.5, 0, 64), (0.3, 1, 33), (0.0, 2 ** 32 + 5, 20), (1.0, 7, 20)):
        got = rr.sample(rew, don, rows, filled, count, skew, 0xC0FFEE1234, ctr)
        want, stats = loop_sample(rew.tolist(), don.tolist(), rows.tolist(), filled, count, skew, 0xC0FFEE1234, ctr)
        assert got[0].tolist() == [w[0] for w in want] and got[1].tolist() == [w[1] for w in want]
        assert got[2].tolist() == [w[2] for w in want] and got[3].tolist() == [w[3] for w in want]
        assert tuple(got[4].tolist()) == stats
        assert all(a.dtype == np.int32 for a in got)


def issue_ring():
    rng = np.random.default_rng(7)
    R, T, S = 3, 5, 4
    rew = np.where(rng.random((R, T, S)) < 0.15, 1.0, -0.0).astype(np.float32)
    rew[rng.random((R, T, S)) < 0.05] = -0.5
    don = rng.random((R, T, S)) < 0.2
    rows = np.arange(R * 2 * (T + 1) * S, dtype=np.int32).reshape(R, 2, -1)
    return rew, don, rows


def test_skew_is_what_it_claims():
    rew, don, rows = issue_ring()
    q = rr.candidates(rew, don, 3)
    assert (len(q[0]), len(q[1])) == (20, 6)
    n = 4096
    for skew, ctr, recorded in ((0.5, 2 ** 32 + 5, 2067), (0.25, 0, 1069)):
        lab = rr.sample(rew, don, rows, 3, n, skew, 0x5EED, ctr)[2]
        pos = int((lab > 0).sum())
        sigma = math.sqrt(n * skew * (1 - skew))
        assert abs(pos - skew * n) <= 4 * sigma, (skew, pos)
        assert pos == recorded
    for ctr in (0, 9):
        assert int((rr.sample(rew, don, rows, 3, n, 0.0, 0x5EED, ctr)[2] > 0).sum()) == 0
        assert int((rr.sample(rew, don, rows, 3, n, 1.0, 0x5EED, ctr)[2] > 0).sum()) == n
    # the negative rewards are drawn as class 2, and every draw's source is a candidate of its set
    ri, rg, lab, src, stats = rr.sample(rew, don, rows, 3, n, 0.5, 0x5EED, 1)
    assert set(lab.tolist()) == {0, 1, 2}
    assert set(src[lab == 0].tolist()) <= set(q[0].tolist()) and set(src[lab > 0].tolist()) <= set(q[1].tolist())
    assert len(set(src.tolist())) == 26  # with replacement, 4096 draws reach every candidate


def test_fallback_and_void_draws():
    rew, don, rows = issue_ring()
    q = rr.candidates(rew, don, 1)
    assert len(q[1]) == 0 and len(q[0]) > 0
    ri, rg, lab, src, stats = rr.sample(rew, don, rows, 1, 512, 0.5, 0x5EED, 3)
    assert (lab == 0).all() and set(src.tolist()) <= set(q[0].tolist())
    assert stats.tolist() == [len(q[0]), 0, 0, 512]
    ri, rg, lab, src, stats = rr.sample(rew, don, rows, 0, 512, 0.5, 0x5EED, 3)
    assert (lab == -1).all() and (src == -1).all() and not ri.any() and not rg.any()
    assert stats.tolist() == [0, 0, 0, 0]


def test_loss_reference_on_a_hand_case():
    lg = np.array([[0.0, 0.0, 0.0, 9.0], [1.0, 2.0, 3.0, -4.0], [5.0, 1.0, 1.0, 0.0]])
    ce, used, g = rr.rp_loss_labels(lg, [0, -1, 2], weight=2.0)
    z = 2 * math.exp(-4.0) + 1
    want = (math.log(3.0) + math.log(z) + 5.0 - 1.0) / 2
    assert used == 2 and abs(ce - want) < 1e-15
    assert not g[1].any() and not g[:, 3].any()
    assert np.allclose(g[0, :3], np.array([-2 / 3, 1 / 3, 1 / 3]) * 2.0 / 2, rtol=1e-15)
    assert abs(g.sum()) < 1e-15  # a softmax gradient sums to 0 per sample
    assert rr.rp_loss_labels(lg, [-1, -1, -1])[:2] == (0.0, 0)


# ---- metrics ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", sorted(EXPECTED))
def test_metric_segment_is_appended(flags):
    from vnav.metrics import metric_layout
    kw = {k: bool(v) for k, v in zip(FLAGS, flags)}
    today, width = EXPECTED[flags]
    assert metric_layout(**kw, rp_sampling=False) == today == metric_layout(**kw)
    on = metric_layout(**kw, rp_sampling=True)
    assert list(on) == list(today) + ["rp_sampling"]
    assert {k: v for k, v in on.items() if k != "rp_sampling"} == today
    assert on["rp_sampling"] == (width, 4)
    assert metric_layout(*kw.values(), True) == on  # the trainer passes it by position, last


# ---- command line ------------------------------------------------------------------------------------
def test_flags_reach_the_trainer(monkeypatch):
    from vnav import train
    seen = []

    class Exp:
        def run(self, resume=False):
            seen.append("run")

    def make(name, **kw):
        seen.append(kw)
        return Exp()

    monkeypatch.setattr(train, "make_trainer", make)
    monkeypatch.setattr(train.vdist, "init_distributed", lambda: None)
    base = dict(env_kwargs={}, save_dir=None, seed=0)
    assert train.main(["thor-cached-auxiliary"]) == 0
    assert seen == [base, "run"]  # without the flags nothing is passed
    del seen[:]
    assert train.main(["thor-cached-auxiliary", "--rp-sampling", "skewed"]) == 0
    assert seen[0] == dict(base, rp_sampling="skewed")
    del seen[:]
    assert train.main(["thor-cached-auxiliary", "--rp-sampling", "skewed", "--rp-batch", "32", "--rp-skew", "0.25",
                       "--no-cuda-graph"]) == 0
    assert seen[0] == dict(base, rp_sampling="skewed", rp_batch=32, rp_skew=0.25, cuda_graph=False)
    del seen[:]
    assert train.main(["thor-cached-auxiliary", "--rp-sampling", "sequence"]) == 0
    assert seen[0] == dict(base, rp_sampling="sequence")
    del seen[:]
    for bad in (["cached-thor", "--rp-batch", "8"], ["cached-thor", "--rp-skew", "0.5"],
                ["cached-thor", "--rp-sampling", "sequence", "--rp-batch", "8"],
                ["cached-thor", "--rp-sampling", "skewed", "--rp-skew", "1.5"],
                ["cached-thor", "--rp-sampling", "skewed", "--rp-batch", "0"],
                ["cached-thor", "--rp-sampling", "uniform"], ["cached-thor", "--cuda-graph", "--no-cuda-graph"]):
        with pytest.raises(SystemExit):
            train.main(bad)
    assert not seen


def test_experiment_passes_them_on():
    """The experiment attributes are the trainer's arguments; the registered experiments keep the
    defaults (thor-cached-auxiliary stays on 'sequence')."""
    import inspect

    from vnav import train
    from vnav.a2c import A2CTrainer
    exp = train.make_trainer("thor-cached-auxiliary", rp_sampling="skewed", rp_batch=32, rp_skew=0.25,
                             cuda_graph=False)
    assert (exp.rp_sampling, exp.rp_batch, exp.rp_skew, exp.cuda_graph) == ("skewed", 32, 0.25, False)
    params = inspect.signature(A2CTrainer.__init__).parameters
    src = inspect.getsource(train.Experiment.create_trainer)
    for name in train.registered():
        off = train.make_trainer(name)
        assert (off.rp_sampling, off.rp_batch, off.rp_skew) == ("sequence", None, 0.5)
    for name in ("rp_sampling", "rp_batch", "rp_skew"):
        assert "%s=self.%s" % (name, name) in src
        assert params[name].default == getattr(off, name)
    assert train.make_trainer("thor-cached-auxiliary").cuda_graph is True
