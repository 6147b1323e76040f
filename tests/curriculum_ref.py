"""numpy restatement of the geodesic start curriculum (include/vnav.h, vn_nav_curriculum): the
per-goal start tables, the draw and the level controller. Shared by test_curriculum_refs.py
(CPU) and the GPU curriculum tests."""
import numpy as np

from oracle import philox
from oracle.envs import VectorEnvOracle


def scene_D(geo):
    """The scene's largest geodesic entry (0 when nothing is reachable)."""
    return max(int(np.asarray(geo).max()), 0)


def keys(geo):
    geo = np.asarray(geo).astype(np.int64)
    return np.clip(geo, -1, scene_D(geo)) + 1


def tables(geo):
    """(order int32 [N, N], count int32 [N, D + 2], D) of a [goal, state] geodesic table:
    order[g] = the states sorted stably by key(g, .), count[g][b] = #states with key <= b."""
    key = keys(geo)
    D = scene_D(geo)
    order = np.argsort(key, axis=1, kind="stable").astype(np.int32)
    count = np.stack([(key <= b).sum(axis=1) for b in range(D + 2)], axis=1).astype(np.int32)
    return order, count, D


def clamp_level(level, level_min, D):
    return min(max(int(level), min(int(level_min), D)), D)


class GeoCurriculumOracle(VectorEnvOracle):
    """VectorEnvOracle whose curriculum draw ranks starts by the scenes' geodesic tables
    (scene dicts carry "geo", [goal, state]) and a per-scene level instead of spd and a
    complexity. Only _curriculum_start is overridden: the rejection path keeps the true spd."""

    def __init__(self, scenes, *args, **kw):
        self.geo_levels = None
        self.geo_mode = 0
        self._geo_cache = {}
        super().__init__(scenes, *args, **kw)

    def set_geo_curriculum(self, mode, levels):
        """levels: one per scene, already clamped (None switches back to the spd draw)."""
        self.geo_levels = None if levels is None else [int(v) for v in levels]
        self.geo_mode = int(mode)
        if levels is not None:
            self.cur_mode = 1
        else:
            self.cur_mode = int(any(getattr(self, "cur_modes", [0])))

    def _geo_row(self, sc, g):
        if (sc, g) not in self._geo_cache:
            geo = np.asarray(self.scenes[sc]["geo"]).astype(np.int64)
            col = np.clip(geo[g], -1, scene_D(geo))
            self._geo_cache[(sc, g)] = (col, np.argsort(col, kind="stable"))
        return self._geo_cache[(sc, g)]

    def _curriculum_start(self, e, k, sc, g):
        if self.geo_levels is None:
            return super()._curriculum_start(e, k, sc, g)
        col, order = self._geo_row(sc, g)
        n = len(col)
        oi = self.geo_levels[sc]
        lo = int((col <= 0).sum())
        hi = int((col <= oi).sum())
        rx, ry, _, _ = philox.philox4x32_10(e, k, 0, philox.STREAM_START, self.k0, self.k1)
        use_far = (self.geo_mode == 2 and int(ry) >= 3865470566 and hi < n) or hi <= lo
        b0, b1 = (hi, n) if use_far else (lo, hi)
        if b1 <= b0:
            return None
        return int(order[b0 + int(philox.uniform_below(rx, b1 - b0))])


class Controller:
    """The per-scene counters and levels: count() is the launch behind every step (while
    window > 0), advance() is vn_nav_curriculum_advance."""

    def __init__(self, Ds, scene, level=1, mode=1, window=0, up=0.8, down=0.3, step=1, level_min=1):
        self.D = np.asarray(Ds, dtype=np.int64)
        S = len(self.D)
        self.window, self.step, self.level_min = int(window), int(step), int(level_min)
        self.up, self.down = np.float32(up), np.float32(down)
        self.level = np.array([clamp_level(level, level_min, D) for D in self.D], dtype=np.int64)
        self.done = np.zeros(S, dtype=np.int64)
        self.succ = np.zeros(S, dtype=np.int64)
        self.ep_scene = np.asarray(scene, dtype=np.int64).copy()

    def count(self, done, truncated, scene):
        """done / truncated: the step's; scene: every env's scene after the step."""
        if self.window <= 0:
            return
        for e in np.nonzero(np.asarray(done))[0]:
            self.done[self.ep_scene[e]] += 1
            if not truncated[e]:
                self.succ[self.ep_scene[e]] += 1
        self.ep_scene = np.asarray(scene, dtype=np.int64).copy()

    def refresh(self, scene):
        self.ep_scene = np.asarray(scene, dtype=np.int64).copy()

    def advance(self):
        if self.window <= 0:
            return
        for k in range(len(self.D)):
            if self.done[k] < self.window:
                continue
            r = np.float32(self.succ[k]) / np.float32(self.done[k])  # one fp32 division
            D = int(self.D[k])
            if r >= self.up:
                self.level[k] = min(self.level[k] + self.step, D)
            elif r <= self.down:
                self.level[k] = max(self.level[k] - self.step, min(self.level_min, D))
            self.done[k] = self.succ[k] = 0

    def state(self):
        return np.stack([self.level, self.done, self.succ, self.D]).astype(np.int32)
