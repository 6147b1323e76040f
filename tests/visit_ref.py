"""numpy restatement of the state-visit counts and the novelty bonus (vn_visit_enable and its
step / refresh forms, vn_visit_stats, vn_a2c_novelty_rewards; include/vnav.h, DESIGN.md "Visit
counts and novelty bonus"): the table, the per-env episode record and seen-set as plain Python
loops, and the bonus in float32, operation for operation. Shared by test_visit_refs.py (CPU) and
the GPU visit tests."""
import numpy as np

from expert_ref import anneal_weight  # noqa: F401  (both weights anneal as the expert's)


def clamp(x, lo, hi):
    return min(max(int(x), lo), hi)


class VisitState:
    """count [C] uint32 over the scenes' states laid end to end, and per env the running
    episode's scene, its number of distinct states and its seen-set."""

    def __init__(self, scene_n, num_envs):
        self.scene_n = [int(n) for n in scene_n]
        self.cell_off = np.concatenate([[0], np.cumsum(self.scene_n)]).astype(np.int64)
        self.C = int(self.cell_off[-1])
        self.W = (max(self.scene_n) + 31) // 32
        self.E = int(num_envs)
        self.count = np.zeros(self.C, dtype=np.uint32)
        self.ep_scene = np.zeros(self.E, dtype=np.int32)
        self.ep_distinct = np.zeros(self.E, dtype=np.int32)
        self.seen = [set() for _ in range(self.E)]

    def cell(self, scene, state):
        """(cell, state) of a (scene, state) pair, both clamped into the tables."""
        k = clamp(scene, 0, len(self.scene_n) - 1)
        s = clamp(state, 0, self.scene_n[k] - 1)
        return int(self.cell_off[k]) + s, s, k

    def packed(self):
        """The layout of vn_visit_get_state: count, the [2, E] record, the [E, W] bitmaps."""
        bits = np.zeros((self.E, self.W), dtype=np.uint32)
        for e, states in enumerate(self.seen):
            for s in states:
                bits[e, s >> 5] |= np.uint32(1 << (s & 31))
        return np.concatenate([self.count.view(np.int32), self.ep_scene, self.ep_distinct,
                               bits.reshape(-1).view(np.int32)])

    def stats(self, scene=None):
        """[cells with count > 0, sum of the counts] of a scene, or of all."""
        lo, hi = (0, self.C) if scene is None else (int(self.cell_off[scene]), int(self.cell_off[scene + 1]))
        c = self.count[lo:hi].astype(np.int64)
        return np.array([(c > 0).sum(), c.sum()], dtype=np.int64)


def visit_start(vs, scene, state, mask=None, add=True):
    """The refresh form (vn_visit_enable(1), vn_visit_clear and vn_reset with add, vn_set_state
    without): the envs whose mask word is not 0 start an episode at their (scene, state)."""
    for e in range(vs.E):
        if mask is not None and mask[e] == 0:
            continue
        cell, s, k = vs.cell(scene[e], state[e])
        vs.seen[e] = {s}
        vs.ep_scene[e] = k
        vs.ep_distinct[e] = 1
        if add:
            vs.count[cell] += np.uint32(1)


def visit_clear(vs, scene, state):
    vs.count[:] = 0
    visit_start(vs, scene, state)


def visit_step(vs, scene, state, done, terminal_state, autoreset=True):
    """One step's (cell int32, first uint8, ep_distinct int32), [E] each. scene / state describe
    the env after the step (get_state(): after an auto-reset the new episode); done and
    terminal_state are the step's. With autoreset off a done env's episode goes on."""
    cell_o = np.zeros(vs.E, np.int32)
    first_o = np.zeros(vs.E, np.uint8)
    dist_o = np.zeros(vs.E, np.int32)
    for e in range(vs.E):
        if done[e]:
            cell, s, _ = vs.cell(vs.ep_scene[e], terminal_state[e])
        else:
            cell, s, _ = vs.cell(scene[e], state[e])
        vs.count[cell] += np.uint32(1)
        first = s not in vs.seen[e]
        vs.seen[e].add(s)
        vs.ep_distinct[e] += int(first)
        cell_o[e], first_o[e] = cell, int(first)
        dist_o[e] = vs.ep_distinct[e] if done[e] else 0
        if done[e] and autoreset:
            c2, s2, k2 = vs.cell(scene[e], state[e])
            vs.seen[e] = {s2}
            vs.ep_scene[e] = k2
            vs.ep_distinct[e] = 1
            vs.count[c2] += np.uint32(1)
    return cell_o, first_o, dist_o


def novelty_rewards32(rewards, cell, first, count, w_count, w_first, steps=0, anneal_steps=0):
    """vn_a2c_novelty_rewards in float32, one correctly rounded operation at a time:
    b = wc / sqrt(float32(N)) (0 where the cell is outside the table or N == 0), f = wf where
    first, out = r + (b + f). Returns (out float32, dict(added, firsts, inv float64 sums, wc))."""
    f = np.float32
    wc = f(anneal_weight(w_count, steps, anneal_steps))
    wf = f(anneal_weight(w_first, steps, anneal_steps))
    r = np.asarray(rewards, dtype=f)
    cell = np.asarray(cell).astype(np.int64)
    count = np.asarray(count, dtype=np.uint32)
    inside = (cell >= 0) & (cell < len(count))
    N = np.where(inside, count[np.clip(cell, 0, max(len(count) - 1, 0))] if len(count) else 0, 0).astype(np.uint32)
    q = np.sqrt(np.where(N > 0, N, 1).astype(f)).astype(f)
    b = np.where(N > 0, (wc / q).astype(f), f(0.0)).astype(f)
    inv = np.where(N > 0, (f(1.0) / q).astype(f), f(0.0)).astype(f)
    fv = np.asarray(first) != 0
    add = (b + np.where(fv, wf, f(0.0)).astype(f)).astype(f)
    out = (r + add).astype(f)
    return out, dict(added=float(add.astype(np.float64).sum()), firsts=float(fv.sum()),
                     inv=float(inv.astype(np.float64).sum()), wc=wc)
