"""numpy restatement of the geodesic reward shaping and GAE(lambda) of the A2C update
(vn_nav_progress, vn_a2c_returns_ex, include/vnav.h; DESIGN.md "Reward shaping and GAE"): the
progress record and its per-step outputs on tests/nav_ref.py's geodesic tables, the returns in
float64 for both recurrences, and the lambda = 1 recurrence in float32 in the kernel's stated
operation order. Shared by test_shaping_refs.py (CPU) and the GPU shaping tests."""
import numpy as np

from expert_ref import anneal_weight  # noqa: F401  (the shaping weight anneals as the expert's)

# roundings per step stated in returns_ex_kernel's comment (csrc/vn_shaping.hip)
K_NSTEP, K_NSTEP_SHAPED, K_GAE, K_GAE_SHAPED = 2, 5, 6, 9


def lookup(geos, scene, goal, state):
    """geo[scene][goal][state] with all three clamped to the tables, as the kernel looks up."""
    k = min(max(int(scene), 0), len(geos) - 1)
    n = geos[k].shape[0]
    return int(geos[k][min(max(int(goal), 0), n - 1), min(max(int(state), 0), n - 1)])


class ProgressRecord:
    """The per-env progress record [3][E]: scene, goal, distance of the running episode."""

    def __init__(self, num_envs):
        self.scene = np.zeros(num_envs, dtype=np.int64)
        self.goal = np.zeros(num_envs, dtype=np.int64)
        self.dist = np.zeros(num_envs, dtype=np.int64)

    def table(self):
        return np.stack([self.scene, self.goal, self.dist]).astype(np.int32)


def progress_refresh(geos, scene, state, goal, record, mask=None):
    """The refresh form (vn_nav_progress(1), vn_set_state; vn_reset with its mask): the record of
    every env whose mask word is not 0 from the env's scene, goal and state."""
    for e in range(len(state)):
        if mask is None or mask[e] != 0:
            record.scene[e], record.goal[e] = int(scene[e]), int(goal[e])
            record.dist[e] = lookup(geos, scene[e], goal[e], state[e])


def progress_ref(geos, scene, state, goal, done, truncated, terminal_state, record):
    """One step's (dist_before, dist_after, progress), int32 [E] each. scene / state / goal
    describe the env after the step (get_state(): after an auto-reset the new episode);
    done / truncated / terminal_state are the step's. `record` is read and then advanced."""
    E = len(state)
    before = np.zeros(E, np.int32)
    after = np.zeros(E, np.int32)
    prog = np.zeros(E, np.int32)
    for e in range(E):
        d = lookup(geos, scene[e], goal[e], state[e])
        b = int(record.dist[e])
        if done[e] and not truncated[e]:
            a = 0
        elif done[e]:
            a = lookup(geos, record.scene[e], record.goal[e], terminal_state[e])
        else:
            a = d
        before[e], after[e] = b, a
        prog[e] = b - a if (b >= 0 and a >= 0) else 0
        record.scene[e], record.goal[e], record.dist[e] = int(scene[e]), int(goal[e]), d
    return before, after, prog


def _f32(x):
    return float(np.float32(x))


def shaping_terms64(dist, w, gamma_phi):
    """F [T, E] in float64 from dist [T, 2, E] and the fp32 weight and discount; 0 where a
    distance is < 0. Returns (F, valid)."""
    b = np.asarray(dist)[:, 0].astype(np.float64)
    a = np.asarray(dist)[:, 1].astype(np.float64)
    valid = (b >= 0) & (a >= 0)
    return np.where(valid, _f32(w) * (b - _f32(gamma_phi) * a), 0.0), valid


def returns_ex64(rewards, dones, bootstrap_out, out, dist, num_actions, gamma, lam, w=0.0, gamma_phi=1.0):
    """vn_a2c_returns_ex in float64. rewards, dones [T, E]; bootstrap_out [E, 8]; out [T*E, 8]
    (read only when lam != 1); dist [T, 2, E] or None; w the (annealed) fp32 weight.
    Returns (returns [T, E], M = the largest magnitude among r', V, G and R met on the way)."""
    r = np.asarray(rewards, dtype=np.float64).copy()
    T, E = r.shape
    nd = 1.0 - (np.asarray(dones) != 0).astype(np.float64)
    A = int(num_actions)
    g, lm = _f32(gamma), _f32(lam)
    if dist is not None and _f32(w) != 0.0:
        r = r + shaping_terms64(dist, w, gamma_phi)[0]
    Vn = np.asarray(bootstrap_out, dtype=np.float64)[:, A].copy()
    M = max(np.abs(r).max(), np.abs(Vn).max())
    ret = np.empty_like(r)
    if lm == 1.0:
        R = Vn
        for t in range(T - 1, -1, -1):
            R = r[t] + g * R * nd[t]
            ret[t] = R
        return ret, max(M, np.abs(ret).max())
    V = np.asarray(out, dtype=np.float64).reshape(T, E, 8)[:, :, A]
    gl = float(np.float32(np.float32(gamma) * np.float32(lam)))  # the kernel rounds the product once
    G = np.zeros(E)
    for t in range(T - 1, -1, -1):
        delta = r[t] + g * Vn * nd[t] - V[t]
        G = delta + gl * nd[t] * G
        ret[t] = G + V[t]
        M = max(M, np.abs(G).max())
        Vn = V[t]
    return ret, max(M, np.abs(V).max(), np.abs(ret).max())


def fma32(a, b, c):
    """Correctly rounded float32 fma of float32 arrays: the product is exact in float64, the sum
    is rounded to odd in float64 (TwoSum's remainder sets the sticky bit), and 53 >= 2 * 24 + 2
    bits make the final rounding to float32 the single rounding of the exact result."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    s_arr = np.atleast_1d(s).astype(np.float64)
    e_arr = np.atleast_1d(err)
    bits = s_arr.view(np.int64).copy()
    # an inexact sum (s != 0 then) with an even significand moves one ulp towards the remainder:
    # up in magnitude iff err has s's sign; either neighbour of an even significand is odd
    inexact = (e_arr != 0) & ((bits & 1) == 0) & np.isfinite(s_arr)
    up = (e_arr > 0) == (s_arr > 0)
    bits = np.where(inexact, bits + np.where(up, 1, -1), bits)
    return bits.view(np.float64).astype(np.float32).reshape(np.shape(s))


def returns_ex32(rewards, dones, bootstrap_out, dist, num_actions, gamma, w=0.0, gamma_phi=1.0):
    """The lambda = 1 form in float32, operation for operation as returns_ex_kernel states it:
    F = w * fma(-gamma_phi, after, before); r' = r + F (only where dist is given and w != 0);
    R = fma(gamma * R, 1 - done, r'). Returns float32 [T, E]."""
    f = np.float32
    r = np.asarray(rewards, dtype=f).copy()
    T, E = r.shape
    nd = (f(1.0) - (np.asarray(dones) != 0).astype(f)).astype(f)
    if dist is not None and f(w) != f(0.0):
        b = np.asarray(dist)[:, 0]
        a = np.asarray(dist)[:, 1]
        valid = (b >= 0) & (a >= 0)
        inner = fma32(np.full(b.shape, -f(gamma_phi), dtype=f), a.astype(f), b.astype(f))
        F = np.where(valid, (f(w) * inner).astype(f), f(0.0)).astype(f)
        r = (r + F).astype(f)
    R = np.asarray(bootstrap_out, dtype=f)[:, int(num_actions)].copy()
    ret = np.empty_like(r)
    for t in range(T - 1, -1, -1):
        R = fma32((f(gamma) * R).astype(f), nd[t], r[t])
        ret[t] = R
    return ret


def shaping_stats(dist):
    """[sum of before, sum of after, invalid steps] as exact integers."""
    b = np.asarray(dist)[:, 0].astype(np.int64)
    a = np.asarray(dist)[:, 1].astype(np.int64)
    valid = (b >= 0) & (a >= 0)
    return np.array([b[valid].sum(), a[valid].sum(), (~valid).sum()], dtype=np.int64)
