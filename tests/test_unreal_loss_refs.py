"""The fp64 references of the UNREAL loss kernels (oracle/unreal.py) on the CPU: against a
second restatement in plain loops (one cell, one step, one sample at a time; no autograd, the
gradient in closed form) on the inputs the GPU tests use (oracle/unreal_cases.py), against
hand-computed cases, and the conditions those inputs must meet so that
tests/test_unreal_loss_kernels_gpu.py cannot pass by skipping what it claims to test.

Tolerance: 1e-12 of the reference's largest magnitude (a gradient element is a difference of
two O(1) numbers, so its own relative error is unbounded; the loops and torch order their
sums differently)."""
import math

import numpy as np
import pytest
import torch

from oracle import unreal
from oracle import unreal_cases as cases


def _close(a, b, rtol, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-300)
    err = np.abs(a - b).max() / scale
    assert err <= rtol, "%s: max err %.3g of scale %.3g" % (what, err, scale)


# ---- the plain restatements ------------------------------------------------------------------

def pixel_change_loops(f0, f1, cells):
    """[cells, cells] of two u8 [H, W, 3] frames."""
    H, W = f0.shape[:2]
    top, left = (H - cells * 4) // 2, (W - cells * 4) // 2
    out = np.zeros((cells, cells))
    for cy in range(cells):
        for cx in range(cells):
            s = 0
            for dy in range(4):
                y = top + cy * 4 + dy
                a = f0[y, left + cx * 4:left + cx * 4 + 4].astype(np.int64)
                b = f1[y, left + cx * 4:left + cx * 4 + 4].astype(np.int64)
                s += int(np.abs(b - a).sum())
            out[cy, cx] = s / (255.0 * 48.0)
    return out


def pc_loss_loops(q, frames, actions, dones, gamma):
    q = np.asarray(q, dtype=np.float64)
    T, S = actions.shape
    C, A = q.shape[2], q.shape[4]
    grad = np.zeros_like(q)
    total = 0.0
    n = T * S * C * C
    for s in range(S):
        R = q[T, s].max(-1)  # [C, C]
        for t in range(T - 1, -1, -1):
            if dones[t, s]:
                R = np.zeros((C, C))
            else:
                R = pixel_change_loops(frames[t, s], frames[t + 1, s], C) + gamma * R
            a = int(actions[t, s])
            for cy in range(C):
                for cx in range(C):
                    d = q[t, s, cy, cx, a] - R[cy, cx]
                    total += d * d
                    grad[t, s, cy, cx, a] = 2.0 * d / n
    return total / n, grad


def rp_loss_loops(logits, rewards, dones):
    logits = np.asarray(logits, dtype=np.float64)
    T, S = rewards.shape
    n = (T - 2) * S
    used = [not (dones[ts - 2, e] or dones[ts - 1, e]) for ts in range(2, T) for e in range(S)]
    count = sum(used)
    grad = np.zeros((n, 3))
    total = 0.0
    for j in range(n):
        if not used[j]:
            continue
        ts, e = 2 + j // S, j % S
        r = float(rewards[ts, e])
        cls = 0 if r == 0 else (1 if r > 0 else 2)
        l = logits[j]
        jm = int(np.argmax(l))
        ex = [1.0 if c == jm else math.exp(l[c] - l[jm]) for c in range(3)]
        so = sum(ex[c] for c in range(3) if c != jm)
        total += math.log1p(so) + (0.0 if cls == jm else l[jm] - l[cls])
        for c in range(3):
            if c == cls:  # p - 1 = -(the other classes' mass)
                grad[j, c] = -sum(ex[k] for k in range(3) if k != c) / (1.0 + so) / count
            else:
                grad[j, c] = ex[c] / (1.0 + so) / count
    return total / max(count, 1), grad, count


def vr_loss_loops(values, returns):
    values, returns = np.asarray(values, dtype=np.float64), np.asarray(returns, dtype=np.float64)
    T, S = values.shape
    grad = np.zeros((T, S))
    total = 0.0
    for t in range(T):
        for s in range(S):
            d = values[t, s] - returns[t, s]
            total += d * d
            grad[t, s] = 2.0 * d / (T * S)
    return total / (T * S), grad


# ---- pixel control ---------------------------------------------------------------------------

@pytest.mark.parametrize("spec", cases.PC_CASES, ids=cases.PC_IDS)
def test_pc_case_conditions_and_oracle_vs_loops(spec):
    c = cases.pc_case(spec)
    T, E, S, A, C = c["T"], c["E"], c["S"], c["A"], c["cells"]
    q, frames, actions, dones = cases.pc_oracle_inputs(c)
    d = dones.numpy()
    # the placed dones, on the used envs
    steps = cases.forced_done_steps(T)
    assert T - 1 in steps and 0 in steps
    for t in (T - 8, T - 9, T - 16):
        assert (t in steps) == (t >= 0)
    assert len(c["forced"]) == len(steps)
    for t, e in c["forced"]:
        assert e < S and d[t, e]
    if S >= 3 and len(steps) >= 2:
        assert len({e for _, e in c["forced"]}) >= 2
    assert c["clean"] is not None and not d[:, c["clean"]].any()
    # every action is taken (a rollout of fewer than A used samples takes T S different ones)
    taken = set(actions.numpy().reshape(-1).tolist())
    assert taken == set(range(A)) if T * S >= A else len(taken) == T * S
    assert c["actions"].min() >= 0 and c["actions"].max() < A
    # both sides of the ReLU mask among the taken value channels
    p2 = c["p2"].reshape(T + 1, S, C, C, 8)
    tv = np.take_along_axis(p2[:T], actions.numpy()[:, :, None, None, None].repeat(C, 2).repeat(C, 3), axis=-1)
    assert (tv == 0).mean() >= 0.05 and (tv > 0).mean() >= 0.05
    assert not p2[..., A + 1:].any() and (p2[..., A] > 0).any()
    assert c["rows_img"].max() < cases.ARENA_ROWS and c["rows_last"].max() < cases.ARENA_ROWS
    assert c["arena"].shape == (cases.ARENA_ROWS, c["H"] * c["W"] * 3 + c["pad"])
    # the oracle against the loops
    gamma = float(np.float32(cases.GAMMA_PC))
    loss, grad = unreal.pc_loss(q, frames, actions, dones, gamma=gamma)
    l2, g2 = pc_loss_loops(q.numpy(), frames.numpy(), actions.numpy(), d, gamma)
    assert abs(loss.item() - l2) <= 1e-12 * l2
    _close(grad.numpy(), g2, 1e-12, "pc grad")
    assert not grad[T].any()
    r = unreal.pixel_change(frames[0, 0], frames[1, 0], C).numpy()
    _close(r, pixel_change_loops(frames[0, 0].numpy(), frames[1, 0].numpy(), C), 1e-12, "pixel change")


def test_pixel_change_by_hand():
    """84x84, 20 cells: the crop starts at (2, 2). One pixel of cell (0, 0) changes by 255 in one
    channel: 1/48 there; a pixel in the margin changes nothing; a whole cell by 51: 0.2."""
    f0 = torch.zeros((84, 84, 3), dtype=torch.uint8)
    f1 = f0.clone()
    f1[2, 2, 1] = 255
    f1[1, 1, :] = 255
    f1[2 + 4 * 19:2 + 4 * 20, 2 + 4 * 3:2 + 4 * 4] = 51
    r = unreal.pixel_change(f1, f0, 20).numpy()  # |f0 - f1|: the order of the frames is immaterial
    want = np.zeros((20, 20))
    want[0, 0], want[19, 3] = 1.0 / 48.0, 0.2
    _close(r, want, 1e-15, "pixel change")
    # 300x400, 42 cells: margins (300 - 168) / 2 = 66 and (400 - 168) / 2 = 116
    g0 = torch.zeros((300, 400, 3), dtype=torch.uint8)
    g1 = g0.clone()
    g1[66 + 4 * 41 + 3, 116 + 4 * 41 + 3, 2] = 255
    g1[65, 116, 0] = 255
    r = unreal.pixel_change(g0, g1, 42).numpy()
    assert r[41, 41] == 1.0 / 48.0 and r.sum() == 1.0 / 48.0


def _flat_frames(T, S, levels):
    """Frames [T+1, S, 84, 84, 3] of one grey level per step."""
    f = torch.zeros((T + 1, S, 84, 84, 3), dtype=torch.uint8)
    for t, v in enumerate(levels):
        f[t] = v
    return f


def test_pc_loss_by_hand_one_step():
    """T = 1, no done: R = r + gamma max_a q_1 with r = 51 / 255 everywhere."""
    q = torch.zeros((2, 1, 20, 20, 2))
    q[0, ..., 1], q[1, ..., 0] = 0.75, 0.5  # exact in float32
    loss, grad = unreal.pc_loss(q, _flat_frames(1, 1, (0, 51)), torch.tensor([[1]]), torch.tensor([[False]]), gamma=0.5)
    d = 0.75 - (0.2 + 0.25)
    assert abs(loss.item() - d * d) < 1e-15
    g = grad.numpy()
    np.testing.assert_allclose(g[0, ..., 1], 2 * d / 400, rtol=1e-12)
    assert not g[0, ..., 0].any() and not g[1].any()


def test_pc_loss_by_hand_every_step_done():
    """Every step done: every target is 0, the bootstrap and the frames do not count."""
    T, S = 3, 2
    q = torch.full((T + 1, S, 20, 20, 3), 0.25)
    q[T] = 100.0
    acts = torch.tensor([[0, 1], [2, 0], [1, 1]])
    loss, grad = unreal.pc_loss(q, _flat_frames(T, S, (0, 255, 0, 255)), acts, torch.ones((T, S), dtype=torch.bool))
    assert loss.item() == 0.0625
    g = grad.numpy()
    assert g.sum() == pytest.approx(2 * 0.25 * T * S * 400 / (T * S * 400), rel=1e-12)
    for t in range(T):
        for s in range(S):
            assert (g[t, s, ..., acts[t, s]] == 2 * 0.25 / (T * S * 400)).all()


def test_pc_loss_by_hand_done_in_the_middle():
    """T = 3, one env, done at step 1: R_2 = r_2 + g q_3, R_1 = 0 (no pseudo-reward across the
    reset, no bootstrap), R_0 = r_0 + g * 0."""
    q = torch.zeros((4, 1, 20, 20, 1))
    q[3] = 1.0
    frames = _flat_frames(3, 1, (0, 51, 255, 204))  # r_0 = 0.2, r_1 = 0.8 (dropped), r_2 = 0.2
    loss, _ = unreal.pc_loss(q, frames, torch.zeros((3, 1), dtype=torch.long), torch.tensor([[False], [True], [False]]),
                             gamma=0.5)
    want = ((0.2 + 0.5) ** 2 + 0.0 + 0.2 ** 2) / 3
    assert abs(loss.item() - want) < 1e-15


# ---- reward prediction -----------------------------------------------------------------------

@pytest.mark.parametrize("spec", cases.RP_CASES, ids=cases.RP_IDS)
def test_rp_case_conditions_and_oracle_vs_loops(spec):
    c = cases.rp_case(spec)
    T, S, n = c["T"], c["S"], c["n"]
    used, (d2, d1, d0) = cases.rp_used(c)
    cls = cases.rp_classes(c["rewards"][2:, :S]).reshape(-1)
    loss, grad, count = cases.rp_expected(c)
    assert count == int(used.sum())
    if c["kind"] == "all_done":
        assert count == 0 and c["dones"].all()
        assert loss == 0.0 and not grad.any()
    else:
        assert 0 < count < n
        # each cause of an unused sample alone, and a used sample that ends an episode itself
        assert (d2 & ~d1).any() and (d1 & ~d2).any()
        assert (used & d0).any()
        # every class among the used samples (n = 4 has two used samples: two classes)
        assert len(set(cls[used].tolist())) == (3 if T >= 4 else 2)
    assert np.isnan(c["logits"][:, 3]).all() and np.isfinite(c["logits"][:, :3]).all()
    if c["kind"] == "trained":
        l = c["logits"][:, :3].astype(np.float64)
        lead = l[np.arange(n), cls]
        others = np.where(np.arange(3) == cls[:, None], -np.inf, l).max(1)
        assert (lead - others >= cases.RP_TRAINED_MARGIN).all()
        assert 0.0 < loss < 2.0 ** -30  # far below fp32 resolution next to 1
    if c["kind"] == "x30":
        assert np.abs(c["logits"][:, :3]).max() > 60.0
    l2, g2, c2 = rp_loss_loops(c["logits"][:, :3], c["rewards"][:, :S], c["dones"][:, :S])
    assert c2 == count
    assert abs(loss - l2) <= 1e-12 * l2
    _close(grad, g2, 1e-12, "rp grad")
    assert not grad[~used].any()


def test_rp_loss_by_hand():
    """One sample per class (T = 3, S = 3, no done), logits 0: CE = log 3, p = 1/3."""
    rewards = torch.tensor([[9.0, 9.0, 9.0], [9.0, 9.0, 9.0], [0.0, 2.0, -0.01]])
    loss, grad, count = unreal.rp_loss(torch.zeros((3, 3)), rewards, torch.zeros((3, 3), dtype=torch.bool))
    assert count == 3 and abs(loss.item() - math.log(3.0)) < 1e-15
    _close(grad.numpy(), (np.full((3, 3), 1.0 / 3.0) - np.eye(3)) / 3.0, 1e-15, "rp grad")


def test_rp_loss_by_hand_dones():
    """T = 4, S = 1. A done at step 1 drops both samples (it is ts - 1 of ts = 2 and ts - 2 of
    ts = 3); a done at step 3 or 2 alone drops ts = 3 only when it is at 2."""
    rewards = torch.tensor([[0.0], [0.0], [1.0], [-1.0]])
    lg = torch.tensor([[0.0, math.log(3.0), 0.0], [0.0, 0.0, math.log(2.0)]])

    def run(*steps):
        d = torch.zeros((4, 1), dtype=torch.bool)
        for s in steps:
            d[s] = True
        return unreal.rp_loss(lg, rewards, d)

    loss, grad, count = run(1)
    assert count == 0 and loss.item() == 0.0 and not grad.any()
    loss, grad, count = run(3)
    want = 0.5 * (math.log(5.0 / 3.0) + math.log(4.0 / 2.0))
    assert count == 2 and abs(loss.item() - want) < 1e-7  # log(3) was rounded to float32
    loss, grad, count = run(2)
    assert count == 1 and abs(loss.item() - math.log(5.0 / 3.0)) < 1e-7 and not grad[1].any()
    loss, grad, count = run(0)
    assert count == 1 and abs(loss.item() - math.log(2.0)) < 1e-7 and not grad[0].any()
    _close(grad[1].numpy(), np.array([0.25, 0.25, -0.5]), 1e-7, "rp grad")


def test_rp_loss_by_hand_saturated():
    """The class leads by 40: CE = log1p(2 e^-40) and d CE / d l_cls = -2 e^-40 / (1 + 2 e^-40),
    to float64 precision (log(1 + s) and p - 1 would both be exactly 0)."""
    rewards = torch.tensor([[0.0], [0.0], [1.0]])
    loss, grad, _ = unreal.rp_loss(torch.tensor([[-37.0, 3.0, -37.0]]), rewards, torch.zeros((3, 1), dtype=torch.bool))
    s = 2.0 * math.exp(-40.0)
    assert abs(loss.item() - math.log1p(s)) <= 1e-15 * s
    g = grad.numpy()[0]
    assert abs(g[1] + s / (1.0 + s)) <= 1e-15 * s and abs(g[0] - 0.5 * s / (1.0 + s)) <= 1e-15 * s


# ---- value replay, scatter, gather, the aux table --------------------------------------------

@pytest.mark.parametrize("T,E,S,A", cases.VR_CASES)
def test_vr_oracle_vs_loops(T, E, S, A):
    out, ret, _ = cases.vr_case(T, E, S, A)
    loss, grad = cases.vr_expected(out, ret, T, E, S, A)
    l2, g2 = vr_loss_loops(out[:T * E, A].reshape(T, E)[:, :S], ret[:T * E].reshape(T, E)[:, :S])
    assert abs(loss - l2) <= 1e-12 * l2
    _close(grad, g2, 1e-12, "vr grad")
    assert loss >= 0.01  # the kernel adds the sum to STATS_PREFILL: not lost next to it


def test_vr_loss_by_hand():
    loss, grad = unreal.vr_loss(torch.tensor([[1.0, 2.0], [0.0, -1.0]]), torch.tensor([[0.0, 2.0], [2.0, 1.0]]))
    assert loss.item() == (1 + 0 + 4 + 4) / 4
    assert grad.tolist() == [[0.5, 0.0], [-1.0, -1.0]]


def test_scatter_and_gather_refs_by_hand():
    """T = 4, E = 2, S = 1, F = 4: frame t collects slot 2 - k of sample ts = t + k."""
    T, E, S, F = 4, 2, 1, 4
    dx = np.arange(2 * 3 * F, dtype=np.float32).reshape(2, 3, F)  # samples ts = 2, 3
    dx4 = np.full((T * E, F), 100.0, dtype=np.float32)
    out = cases.scatter_ref(dx, dx4, T, E, S, F, 0).reshape(T, E, F)
    assert np.array_equal(out[0, 0], dx[0, 0]) and np.array_equal(out[1, 0], dx[0, 1] + dx[1, 0])
    assert np.array_equal(out[2, 0], dx[0, 2] + dx[1, 1]) and np.array_equal(out[3, 0], dx[1, 2])
    assert (out[:, 1] == 100.0).all()
    acc = cases.scatter_ref(dx, dx4, T, E, S, F, 1).reshape(T, E, F)
    assert np.array_equal(acc[:, 0], out[:, 0] + 100.0) and (acc[:, 1] == 100.0).all()
    h_all = np.arange(T * E * 512, dtype=np.float32).reshape(T * E, 512)
    boot = -np.ones((E, 512), dtype=np.float32)
    x4 = np.arange(T * E * F, dtype=np.float32).reshape(T * E, F)
    h_pc, rp_x = cases.gather_ref(h_all, boot, x4, T, E, S, F)
    assert h_pc.shape == (5, 512) and np.array_equal(h_pc[:4], h_all[::2]) and (h_pc[4] == -1).all()
    assert rp_x.shape == (2, 3, F)
    for j in range(2):
        for k in range(3):
            assert np.array_equal(rp_x[j, k], x4[(j + k) * E])
    assert cases.gather_ref(h_all[:2 * E], boot, x4, 2, E, S, F)[1] is None


def test_aux_table_ref_by_hand():
    """174x174 -> 42x42 (margins 3/3), 300x400 -> 74x98 (margins 2/4)."""
    for (H, W), (ph, pw), (top, left) in (((174, 174), (42, 42), (3, 3)), ((300, 400), (74, 98), (2, 4))):
        depth = np.zeros((1, H, W, 1), dtype=np.uint8)
        seg = np.zeros((1, H, W, 3), dtype=np.uint8)
        depth[0, top, left, 0] = 255
        depth[0, top - 1, left, 0] = 255  # margin
        seg[0, top + 4 * (ph - 1):top + 4 * ph, left + 4 * (pw - 1):left + 4 * pw, 2] = 51
        seg[0, top + 4 * ph, left, 1] = 255  # margin
        t = cases.aux_table_ref(depth, seg, ph, pw)
        assert t.shape == (1, ph, pw, 4)
        assert t[0, 0, 0, 0] == 1.0 / 16.0 and abs(t[0, ph - 1, pw - 1, 3] - 0.2) < 1e-15
        assert abs(t.sum() - (1.0 / 16.0 + 0.2)) < 1e-14
