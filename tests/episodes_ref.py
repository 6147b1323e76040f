"""numpy restatement of the fixed-episode evaluation (include/vnav.h, vn_nav_sample_episodes and
vn_nav_set_episode_log; DESIGN.md "Fixed-episode evaluation"): the episode sampler, the
per-episode log rule, the static episode -> env assignment and a CPU walk of a constant-action
policy. Built on oracle.philox and tests/nav_ref.py; shared by test_episodes_refs.py (CPU) and
the GPU tests."""
import numpy as np

import nav_ref
from oracle import philox

STREAM_EPISODES = 5
MAX_DISTANCE = 32767


def qualifying(geo, lo, hi):
    """Q = {(g, s) : lo <= geo[g][s] <= hi} as (goal, state) arrays, ordered by g, then by s."""
    hi = MAX_DISTANCE if hi is None else min(int(hi), MAX_DISTANCE)
    g, s = np.nonzero((geo >= lo) & (geo <= hi))  # row-major: by g, then by s
    return g, s


def draw_u64(count, seed, salt):
    """u of draws 0..count-1 as Python ints: r.x * 2^32 + r.y of Philox((j, 0, salt, 5), seed)."""
    k0, k1 = philox.seed_key(seed)
    x, y, _, _ = philox.philox4x32_10(np.arange(count), 0, int(salt) & 0xFFFFFFFF, STREAM_EPISODES, k0, k1)
    return [(int(a) << 32) | int(b) for a, b in zip(x, y)]


def index_of(u, total):
    """(u * total) >> 64 in exact integers."""
    return (int(u) * int(total)) >> 64


def sample_episodes(geo, lo, hi, count, seed, salt, u=None):
    """(pairs int32 [count, 2] = (start, goal), distance int32 [count], total). ``u`` forces
    the 64-bit draws (a list of ints) instead of the Philox ones."""
    g, s = qualifying(geo, lo, hi)
    total = len(g)
    pairs = np.full((count, 2), -1, dtype=np.int32)
    dist = np.full(count, -1, dtype=np.int32)
    if total == 0:
        return pairs, dist, 0
    u = draw_u64(count, seed, salt) if u is None else u
    idx = np.array([index_of(v, total) for v in u], dtype=np.int64)
    pairs[:, 0], pairs[:, 1] = s[idx], g[idx]
    dist[:] = geo[g[idx], s[idx]]
    return pairs, dist, total


def assign(scene, num_envs, num_scenes):
    """The static placement, restated with plain loops: one env per scene that holds episodes,
    every further env to the scene with the most episodes per env (lowest scene on a tie);
    a scene's envs consecutive in scene order; its j-th episode on its (j mod m)-th env, slot
    j div m. Returns (env_scenes, env, slot, want, slots)."""
    counts = [0] * num_scenes
    for k in scene:
        counts[int(k)] += 1
    m = [1 if c else 0 for c in counts]
    for _ in range(num_envs - sum(m)):
        best, best_k = -1.0, -1
        for k in range(num_scenes):
            if m[k] and counts[k] / m[k] > best:
                best, best_k = counts[k] / m[k], k
        m[best_k] += 1
    first, env_scenes = [], []
    for k in range(num_scenes):
        first.append(len(env_scenes))
        env_scenes += [k] * m[k]
    seen = [0] * num_scenes
    env, slot = [], []
    for k in scene:
        k = int(k)
        env.append(first[k] + seen[k] % m[k])
        slot.append(seen[k] // m[k])
        seen[k] += 1
    want = [0] * num_envs
    for e in env:
        want[e] += 1
    return (np.array(env_scenes, np.int32), np.array(env, np.int64), np.array(slot, np.int64),
            np.array(want, np.int32), max(slot) + 1)


class EpisodeLogRef:
    """The log rule of the nav step: for an env with done, slot count[e] is written while
    count[e] < want[e], then count[e] += 1."""
    FIELDS = ("success", "length", "start_distance", "spl", "ep_return")

    def __init__(self, capacity, want):
        E = len(want)
        self.want = np.asarray(want, dtype=np.int64)
        self.count = np.zeros(E, dtype=np.int64)
        self.written = np.zeros((capacity, E), dtype=bool)
        self.success = np.zeros((capacity, E), dtype=np.uint8)
        self.length = np.zeros((capacity, E), dtype=np.int32)
        self.start_distance = np.zeros((capacity, E), dtype=np.int32)
        self.spl = np.zeros((capacity, E), dtype=np.float32)
        self.ep_return = np.zeros((capacity, E), dtype=np.float32)

    def step(self, done, success, spl, start_distance, length, ep_return):
        for e in np.nonzero(np.asarray(done))[0]:
            k = self.count[e]
            if k < self.want[e]:
                self.written[k, e] = True
                self.success[k, e] = success[e]
                self.length[k, e] = length[e]
                self.start_distance[k, e] = start_distance[e]
                self.spl[k, e] = spl[e]
                self.ep_return[k, e] = ep_return[e]
            self.count[e] = k + 1


def walk_constant(graph, geo, start, goal, action, limit):
    """One episode of the policy that always takes ``action``: (success, length, spl float32).
    A move along a missing edge leaves the state; the episode ends on the goal (success) or
    after ``limit`` steps."""
    s, l = int(start), int(geo[goal, start])
    for p in range(1, limit + 1):
        nxt = int(graph[s, action])
        if nxt >= 0:
            s = nxt
        if s == goal:
            return True, p, nav_ref.spl_value(True, l, p)
    return False, limit, np.float32(0.0)
