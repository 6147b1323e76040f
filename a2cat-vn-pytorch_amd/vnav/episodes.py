"""Fixed episode sets for evaluation (DESIGN.md "Fixed-episode evaluation").

An ``EpisodeSet`` is a list of (scene, start, goal) episodes with their action-graph geodesic
distance and distance bucket: sampled on the device, stratified by distance
(``VectorEnv.sample_episodes``), or given explicitly. ``A2CTrainer.evaluate_episodes`` runs every
episode of a set exactly once. The helpers that place episodes on envs and split a set between
ranks are pure numpy, so they are tested without a GPU.
"""
import warnings

import numpy as np

DEFAULT_BUCKETS = ((1, 3), (4, 8), (9, None))
MAX_DISTANCE = 32767


def parse_buckets(text):
    """"1-3,4-8,9-" -> ((1, 3), (4, 8), (9, None))."""
    out = []
    for part in text.split(","):
        lo, _, hi = part.strip().partition("-")
        out.append((int(lo), int(hi) if hi.strip() else None))
    return tuple(out)


def bucket_of(distance, buckets):
    """Index of the first bucket holding each distance, -1 where none does."""
    d = np.asarray(distance, dtype=np.int64)
    out = np.full(d.shape, -1, dtype=np.int32)
    for b in reversed(range(len(buckets))):
        lo, hi = buckets[b]
        out[(d >= lo) & (d <= (MAX_DISTANCE if hi is None else hi))] = b
    return out


def world_slice(num_episodes, rank, world):
    """The episodes rank ``rank`` of ``world`` evaluates: j = rank (mod world), ascending."""
    return np.arange(int(rank), int(num_episodes), int(world), dtype=np.int64)


def assign_episodes(scene, num_envs, num_scenes):
    """Static placement of the episodes on the envs. Scenes that hold episodes get envs in
    proportion to their episode counts, at least one each: after one env per such scene every
    further env goes to the scene with the most episodes per env (the lowest scene on a tie).
    A scene's envs are consecutive, scenes in ascending order; episode j of a scene (in the
    set's order) goes to the scene's (j mod m)-th env, slot j div m.
    Returns (env_scenes int32 [E], env int64 [M], slot int64 [M], want int32 [E], slots)."""
    scene = np.asarray(scene, dtype=np.int64)
    E = int(num_envs)
    counts = np.bincount(scene, minlength=int(num_scenes)) if len(scene) else np.zeros(int(num_scenes), np.int64)
    present = np.nonzero(counts)[0]
    if len(present) == 0:
        raise ValueError("the episode set is empty")
    if len(present) > E:
        raise ValueError("%d scenes hold episodes but there are only %d envs" % (len(present), E))
    m = np.zeros(len(counts), dtype=np.int64)
    m[present] = 1
    for _ in range(E - len(present)):
        load = np.where(m > 0, counts / np.maximum(m, 1), -1.0)
        m[int(np.argmax(load))] += 1
    first = np.concatenate([[0], np.cumsum(m)[:-1]])
    env_scenes = np.repeat(np.arange(len(counts)), m).astype(np.int32)
    env = np.zeros(len(scene), dtype=np.int64)
    slot = np.zeros(len(scene), dtype=np.int64)
    for k in present:
        idx = np.nonzero(scene == k)[0]
        j = np.arange(len(idx))
        env[idx] = first[k] + j % m[k]
        slot[idx] = j // m[k]
    want = np.bincount(env, minlength=E).astype(np.int32)
    return env_scenes, env, slot, want, int(slot.max()) + 1


class EpisodeSet:
    """M episodes: int32 arrays ``scene``, ``start``, ``goal``, ``distance`` (geo[goal][start]),
    ``bucket`` (index into ``buckets``, -1 = in none) and the bucket edges ((lo, hi), hi None =
    open)."""

    def __init__(self, scene, start, goal, distance=None, buckets=DEFAULT_BUCKETS, env=None):
        self.scene = np.atleast_1d(np.asarray(scene, dtype=np.int32))
        self.start = np.atleast_1d(np.asarray(start, dtype=np.int32))
        self.goal = np.atleast_1d(np.asarray(goal, dtype=np.int32))
        if not (self.scene.shape == self.start.shape == self.goal.shape) or self.scene.ndim != 1:
            raise ValueError("scene, start and goal must be 1-d arrays of one length")
        self.buckets = tuple((int(lo), None if hi is None else int(hi)) for lo, hi in buckets)
        if distance is None:
            if env is None:
                raise ValueError("an explicit EpisodeSet needs distance= or env= (distances from env.geodesic)")
            distance = self._distances(env)
        self.distance = np.atleast_1d(np.asarray(distance, dtype=np.int32))
        if self.distance.shape != self.scene.shape:
            raise ValueError("distance must have one entry per episode")
        self.bucket = bucket_of(self.distance, self.buckets)

    def __len__(self):
        return len(self.scene)

    def _check_ranges(self, env):
        n_scenes = len(env.scenes)
        if len(self) and (self.scene.min() < 0 or self.scene.max() >= n_scenes):
            raise ValueError("episode set: a scene index outside 0..%d" % (n_scenes - 1))
        for k in np.unique(self.scene):
            n = env.scenes[int(k)].n_states
            sel = self.scene == k
            if min(self.start[sel].min(), self.goal[sel].min()) < 0 or \
                    max(self.start[sel].max(), self.goal[sel].max()) >= n:
                raise ValueError("episode set: a start or goal outside scene %d's %d states" % (k, n))

    def _distances(self, env):
        self._check_ranges(env)
        out = np.zeros(len(self), dtype=np.int32)
        for k in np.unique(self.scene):
            geo = env.geodesic(int(k)).cpu().numpy()
            sel = self.scene == k
            out[sel] = geo[self.goal[sel], self.start[sel]]
        return out

    def validate(self, env):
        """Every index inside the env's tables, every goal reachable from its start and not the
        start itself, and the stored distances equal to the env's."""
        if len(self) == 0:
            raise ValueError("the episode set is empty")
        d = self._distances(env)
        if (d < 1).any():  # -1: unreachable; 0: the start is the goal, no episode to run
            j = int(np.nonzero(d < 1)[0][0])
            raise ValueError("episode %d: goal %d %s start %d in scene %d"
                             % (j, self.goal[j], "is the" if d[j] == 0 else "cannot be reached from", self.start[j],
                                self.scene[j]))
        if not np.array_equal(d, self.distance):
            raise ValueError("episode set: the stored distances are not this env's (other scenes?)")
        return self

    @classmethod
    def sample(cls, env, per_bucket, buckets=DEFAULT_BUCKETS, seed=0):
        """``per_bucket`` episodes per scene and bucket, drawn on the device with
        salt = scene * 65536 + bucket. A bucket without a pair in a scene is left out with a
        warning."""
        sc, st, gl, ds = [], [], [], []
        for k in range(len(env.scenes)):
            for b, (lo, hi) in enumerate(buckets):
                pairs, dist, total = env.sample_episodes(k, per_bucket, lo, hi, seed=seed, salt=k * 65536 + b)
                if total == 0:
                    warnings.warn("scene %d has no pair at distance %s-%s: bucket left out"
                                  % (k, lo, "" if hi is None else hi))
                    continue
                pairs = pairs.cpu().numpy()
                sc.append(np.full(len(pairs), k, dtype=np.int32))
                st.append(pairs[:, 0])
                gl.append(pairs[:, 1])
                ds.append(dist.cpu().numpy())
        if not sc:
            return cls(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32),
                       distance=np.zeros(0, np.int32), buckets=buckets)
        return cls(np.concatenate(sc), np.concatenate(st), np.concatenate(gl), distance=np.concatenate(ds),
                   buckets=buckets)

    def subset(self, index):
        index = np.asarray(index, dtype=np.int64)
        return EpisodeSet(self.scene[index], self.start[index], self.goal[index], distance=self.distance[index],
                          buckets=self.buckets)

    def save(self, path):
        edges = np.array([[lo, -1 if hi is None else hi] for lo, hi in self.buckets], dtype=np.int32).reshape(-1, 2)
        with open(path, "wb") as f:
            np.savez(f, scene=self.scene, start=self.start, goal=self.goal, distance=self.distance, buckets=edges)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as d:
            buckets = tuple((int(lo), None if hi < 0 else int(hi)) for lo, hi in d["buckets"])
            return cls(d["scene"], d["start"], d["goal"], distance=d["distance"], buckets=buckets)
