"""tests/expert_ref.py (the fp64 restatement the GPU expert tests compare against) checked on
the CPU: its loss and gradient against torch fp64 autograd of oracle.a2c's loss plus
-w mean([M != 0] logsumexp(logp[M])), the annealing rule at its five points, and the slot
convention of the trainer's mask history on oracle.envs.VectorEnvOracle + nav_ref."""
import numpy as np
import pytest
import torch

from oracle import a2c as oa2c
from oracle import envs as oe

import expert_ref as er
import nav_ref as nr


def torch_loss(out, actions, rets, mask, A, vc, ec, pg, w):
    """oracle.a2c.loss (pg scaling its action term) + the expert term, fp64, with autograd.
    inv_n is the fp32 reciprocal the kernel multiplies by, so the comparison isolates the
    formulas."""
    o = torch.tensor(np.asarray(out, dtype=np.float64), requires_grad=True)
    n = o.shape[0]
    total, st = oa2c.loss(o[:, :A], o[:, A], torch.as_tensor(np.asarray(actions, dtype=np.int64)),
                          torch.tensor(np.asarray(rets, dtype=np.float64)), vc, ec)
    total = total + (pg - 1.0) * st["action_loss"]
    logp = torch.log_softmax(o[:, :A], dim=-1)
    bits = torch.as_tensor(er.mask_bits(mask, A))
    valid = bits.any(1)
    lq = torch.logsumexp(torch.where(bits, logp, torch.full_like(logp, -float("inf")))[valid], dim=1)
    total = total - w * lq.sum() / n
    scale = float(np.float32(1.0) / np.float32(n)) * n  # mean -> sum * (fp32 1 / n)
    total = total * scale
    g, = torch.autograd.grad(total, o)
    return float(total.detach()), g.numpy()


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("A", [1, 3, 4, 7])
def test_loss_and_gradient_vs_autograd(A, scale):
    """All 16 mask values (several samples each), pg 1 / 0 / 0.25. Gradient within 1e-9 of its
    scale, loss within 1e-9 relative: both sides are fp64, the difference is the order of
    their sums."""
    rng = np.random.RandomState([11, A, int(scale)])
    mask = np.repeat(np.arange(16, dtype=np.uint8), 3)
    n = len(mask)
    out = np.zeros((n, 8), dtype=np.float32)
    out[:, :A] = (rng.randn(n, A) * scale).astype(np.float32)
    out[:, A] = rng.randn(n).astype(np.float32)
    actions = rng.randint(0, A, size=n).astype(np.int32)
    rets = rng.randn(n).astype(np.float32)
    vc, ec = float(np.float32(0.5)), float(np.float32(0.01))
    for pg in (1.0, 0.0, 0.25):
        for w in (0.75, 0.0):
            ref = er.expert_loss_grad64(out, actions, rets, mask, A, vc, ec, pg, w)
            loss, g = torch_loss(out, actions, rets, mask, A, vc, ec, pg, w)
            assert abs(ref["loss"] - loss) <= 1e-9 * max(abs(loss), 1.0), (pg, w, ref["loss"], loss)
            err = np.abs(ref["dout"][:, :A + 1] - g[:, :A + 1]).max()
            assert err <= 1e-9 * np.abs(g).max(), (pg, w, err)
            assert (ref["dout"][:, A + 1:] == 0.0).all()
    # w = 0, pg = 1: oracle.a2c.loss_grad64 itself
    base, s4, m4 = oa2c.loss_grad64(out, actions, rets, A, 0.5, 0.01)
    ref = er.expert_loss_grad64(out, actions, rets, mask, A, 0.5, 0.01, 1.0, 0.0)
    assert np.array_equal(ref["dout"], base) and np.array_equal(ref["stats4"], s4) and np.array_equal(ref["mags4"], m4)
    # the counts: labelled = masks with a bit below A
    bits = er.mask_bits(mask, A)
    assert ref["expert3"][2] == bits.any(1).sum()
    assert ref["expert3"][1] == bits[np.arange(n), actions].sum()


def test_extreme_mass_is_finite_and_exact():
    """A mask whose actions hold < 1e-30 of the mass: log q = the logit gap, gradient = p -
    one-hot over the mask; a mask holding all of it: log q = -(the others' mass), gradient 0
    to that mass."""
    out = np.zeros((2, 8), dtype=np.float32)
    out[0, :4] = (80.0, 0.0, -1.0, 0.0)   # mask {1, 2}: ~ e^-80 = 1.8e-35 of the mass
    out[1, :4] = (80.0, 79.0, 0.0, 0.0)   # mask {0, 1}: all but ~ 2 e^-80 / 1.37
    mask = np.array([0b0110, 0b0011], dtype=np.uint8)
    ref = er.expert_loss_grad64(out, np.zeros(2, np.int32), out[:, 4], mask, 4, 0.5, 0.0, 0.0, 1.0)
    d = ref["dout"][:, :4] * 2.0
    assert np.isfinite(d).all()
    lq0 = -80.0 + np.log1p(np.exp(-1.0))
    assert abs(-ref["expert3"][0] - (lq0 - 0.0)) <= 1e-12 * 80 + 1e-30
    r = np.exp(np.array([0.0, -1.0])) / (1.0 + np.exp(-1.0))
    assert np.allclose(d[0], [1.0, -r[0], -r[1], 0.0], rtol=0, atol=1e-12)
    assert np.abs(d[1]).max() <= 1e-30 and np.abs(d[1, 2:]).min() > 0.0


def test_annealing_rule():
    w0, anneal = 0.7, 1000
    f = float(np.float32(w0))
    want = {0: f, anneal // 2: f * 0.5, anneal: 0.0, 2 * anneal: 0.0}
    for s, v in want.items():
        got = er.anneal_weight(w0, s, anneal)
        assert got.dtype == np.float32 and got == np.float32(v), (s, got, v)
    for s in (0, 500, 10 ** 12):
        assert er.anneal_weight(w0, s, 0) == np.float32(w0)
        assert er.anneal_weight(w0, s, -5) == np.float32(w0)
    # fp64 then one rounding: a step count past 2^24 still moves the weight
    assert er.anneal_weight(1.0, 2 ** 30 + 1, 2 ** 31) != er.anneal_weight(1.0, 2 ** 30 + 129, 2 ** 31)
    assert er.anneal_weight(1.0, 1, 3) == np.float32(1.0 - 1.0 / 3.0)


def test_slot_convention_across_resets():
    """Two rollouts of T = 3 with max_steps = 4: the mask in slot t is the mask of the state
    observed at step t (the state before the step's action), across truncations and
    auto-resets, slot 0 of the second rollout included; the env's own buffer ends at the
    post-rollout state."""
    scenes = nr.shared_scenes()
    graphs = [np.asarray(s.graph) for s in scenes]
    geos = [nr.geodesic(g) for g in graphs]
    E, T = 7, 3
    env = oe.VectorEnvOracle([dict(graph=s.graph, spd=s.spd, rewards=s.rewards, terminal_obs=s.terminal_obs)
                              for s in scenes], E, 5, max_steps=4)
    rng = np.random.RandomState(3)
    own = er.observed_masks(graphs, geos, env.scene, env.state, env.goal)  # vn_set_nav_buffers' write
    resets = 0
    for _ in range(2):
        observed, after = [], []
        for t in range(T):
            observed.append(er.observed_masks(graphs, geos, env.scene, env.state, env.goal))
            resets += int(env.step(rng.randint(0, 4, size=E))["done"].sum())
            after.append(er.observed_masks(graphs, geos, env.scene, env.state, env.goal))
        hist, own = er.rollout_mask_history(own, after)
        assert np.array_equal(hist, np.stack(observed))
        assert np.array_equal(own, er.observed_masks(graphs, geos, env.scene, env.state, env.goal))
    assert resets >= E  # every env was reset inside the window at least once


def test_cli_flags_reach_the_trainer(monkeypatch):
    """--expert-weight / --expert-anneal / --imitation -> the experiment's overrides."""
    from vnav import train
    seen = []

    class Stub:
        def run(self, resume=False):
            pass

    def fake(name, **kw):
        seen.append(kw)
        return Stub()

    monkeypatch.setattr(train, "make_trainer", fake)
    monkeypatch.setattr(train.vdist, "init_distributed", lambda *a, **k: None)
    keys = ("expert_weight", "expert_anneal_steps", "pg_coefficient")

    def pick(kw):
        return {k: kw[k] for k in keys if k in kw}

    train.main(["cached-thor"])
    assert pick(seen[-1]) == {}
    train.main(["cached-thor", "--expert-weight", "0.25", "--expert-anneal", "5000"])
    assert pick(seen[-1]) == {"expert_weight": 0.25, "expert_anneal_steps": 5000}
    train.main(["cached-thor", "--imitation"])
    assert pick(seen[-1]) == {"expert_weight": 1.0, "pg_coefficient": 0.0}
    train.main(["cached-thor", "--imitation", "--expert-weight", "2", "--expert-anneal", "7"])
    assert pick(seen[-1]) == {"expert_weight": 2.0, "pg_coefficient": 0.0, "expert_anneal_steps": 7}
    with pytest.raises(SystemExit):
        train.main(["cached-thor", "--expert-anneal", "7"])
    for k in keys:
        assert hasattr(train.Experiment, k)
