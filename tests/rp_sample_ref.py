"""numpy restatement of the reward-skewed reward-prediction draw (include/vnav.h,
vn_unreal_rp_sample; DESIGN.md "Reward-skewed reward prediction") and of the reward-prediction
loss on explicit labels (vn_unreal_rp_loss_grad_labels). Built on oracle.philox; shared by
test_rp_sample_refs.py (CPU) and the GPU tests."""
import numpy as np

from oracle import philox

STREAM_RP = 6


def candidates(rewards, dones, filled):
    """(Q0, Q1): the window indices i = (r (T-2) + (ts-2)) S + e of the candidates with a zero
    reward (-0.0 included) and of the rest, ascending. rewards / dones [capacity][T][S]."""
    rewards, dones = np.asarray(rewards, dtype=np.float32), np.asarray(dones) != 0
    R, T, S = rewards.shape
    filled = max(0, min(int(filled), R))
    ok = ~dones[:filled, :T - 2] & ~dones[:filled, 1:T - 1]  # [filled][T-2][S], indexed by ts - 2
    zero = rewards[:filled, 2:] == 0
    i0 = np.flatnonzero((ok & zero).reshape(-1))  # row-major = by r, then ts, then e = by i
    i1 = np.flatnonzero((ok & ~zero).reshape(-1))
    return i0.astype(np.int64), i1.astype(np.int64)


def threshold(skew):
    """(uint64)(skew * 2^32), formed in fp64 as the host side of the call forms it."""
    return int(np.float64(skew) * np.float64(4294967296.0))


def sample(rewards, dones, rows, filled, count, skew, seed, ctr):
    """The draws 0..count-1 under draw counter ``ctr``: (rows_img int32 [count, 3], rows_goal
    int32 [count, 3], label int32 [count], src int32 [count], stats4 int32 [4])."""
    rewards = np.asarray(rewards, dtype=np.float32)
    R, T, S = rewards.shape
    rows = np.asarray(rows).reshape(R, 2, (T + 1) * S)
    q = candidates(rewards, dones, filled)
    k0, k1 = philox.seed_key(seed)
    ctr = int(ctr) & 0xFFFFFFFFFFFFFFFF
    x, y, z, _ = philox.philox4x32_10(np.arange(count), ctr & 0xFFFFFFFF, ctr >> 32, STREAM_RP, k0, k1)
    thr = threshold(skew)
    rows_img = np.zeros((count, 3), dtype=np.int32)
    rows_goal = np.zeros((count, 3), dtype=np.int32)
    label = np.full(count, -1, dtype=np.int32)
    src = np.full(count, -1, dtype=np.int32)
    for j in range(count):
        k = 1 if int(x[j]) < thr else 0
        if len(q[k]) == 0:
            k = 1 - k
        if len(q[k]) == 0:
            continue
        u = (int(y[j]) << 32) | int(z[j])
        i = int(q[k][(u * len(q[k])) >> 64])
        w, e = divmod(i, S)
        r, tt = divmod(w, T - 2)
        rw = rewards[r, tt + 2, e]
        label[j] = 0 if rw == 0 else (1 if rw > 0 else 2)
        src[j] = i
        for m in range(3):
            rows_img[j, m] = rows[r, 0, (tt + m) * S + e]
            rows_goal[j, m] = rows[r, 1, (tt + m) * S + e]
    stats4 = np.array([len(q[0]), len(q[1]), int((label > 0).sum()), int((label >= 0).sum())], dtype=np.int32)
    return rows_img, rows_goal, label, src, stats4


def rp_loss_labels(logits, label, weight=1.0):
    """(mean CE over the used samples, used count, dlogits [n, 4]) in fp64, by plain loops: label
    0 / 1 / 2 = the class, anything else = unused. dlogits = weight * d mean CE / d logits
    (column 3 is padding: 0)."""
    logits = np.asarray(logits, dtype=np.float64)
    n = logits.shape[0]
    used = [j for j in range(n) if 0 <= int(label[j]) <= 2]
    g = np.zeros((n, 4), dtype=np.float64)
    total = 0.0
    for j in used:
        l = logits[j, :3]
        m = max(l)
        ex = [np.exp(v - m) for v in l]
        z = sum(ex)
        c = int(label[j])
        total += np.log(z) + m - l[c]
        for a in range(3):
            if a == c:  # p_c - 1 as minus the other classes' mass: no cancellation next to 1
                g[j, a] = -sum(ex[b] for b in range(3) if b != c) / z * weight / len(used)
            else:
                g[j, a] = ex[a] / z * weight / len(used)
    return (total / len(used) if used else 0.0), len(used), g
