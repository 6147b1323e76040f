"""numpy / scipy restatement of the navigation info of vn_step (include/vnav.h, vn_nav_enable):
the action-graph geodesic table and the six per-step outputs. Shared by test_nav_refs.py (CPU)
and the GPU nav tests, with the three small scenes they use."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import shortest_path

from vnav.scenes import Scene, maze_scene, synthetic_scene

FRAME = (16, 16, 3)


def geodesic(graph):
    """int16 [N, N] indexed [goal, state]: least number of actions from state to goal along
    graph[.][0..3] (-1 = no edge); 0 on the diagonal, -1 where the goal cannot be reached."""
    graph = np.asarray(graph)
    n = len(graph)
    src, act = np.nonzero(graph >= 0)
    dst = graph[src, act]
    adj = csr_matrix((np.ones(len(src)), (src, dst)), shape=(n, n))
    d = shortest_path(adj, method="D", directed=True, unweighted=True)  # [state, goal]
    d = np.where(np.isinf(d), -1, d)
    return np.ascontiguousarray(d.T).astype(np.int16)


def distance_mask_action(graph, geo, state, goal):
    """(distance, optimal mask, optimal action) of one (state, goal)."""
    d = int(geo[goal, state])
    mask = 0
    if d > 0:
        for a in range(4):
            nxt = int(graph[state, a])
            if nxt != -1 and int(geo[goal, nxt]) == d - 1:
                mask |= 1 << a
    action = -1 if mask == 0 else (mask & -mask).bit_length() - 1
    return d, mask, action


def spl_value(success, l, p):
    """float32 SPL of one finished episode: start distance l, path length p."""
    if not success or l < 0:
        return np.float32(0.0)
    if l == 0:
        return np.float32(1.0)
    return np.float32(l) / np.float32(max(p, l))


class NavRecord:
    """The per-env nav record: start distance and length offset."""

    def __init__(self, num_envs):
        self.start = np.zeros(num_envs, dtype=np.int64)
        self.offset = np.zeros(num_envs, dtype=np.int64)

    def copy(self):
        r = NavRecord(len(self.start))
        r.start, r.offset = self.start.copy(), self.offset.copy()
        return r


def nav_refresh(graphs, geos, scene, state, goal, elapsed, record, enable=False):
    """vn_reset's refresh form (enable=True: vn_nav_enable's): distance, mask and action of
    every env; the record of the envs at elapsed == 0 (every env when enabling, a running
    episode being measured from here on)."""
    E = len(state)
    out = dict(distance_to_goal=np.zeros(E, np.int32), optimal_mask=np.zeros(E, np.uint8),
               optimal_action=np.zeros(E, np.int32))
    for e in range(E):
        k = int(scene[e])
        d, m, a = distance_mask_action(graphs[k], geos[k], int(state[e]), int(goal[e]))
        out["distance_to_goal"][e], out["optimal_mask"][e], out["optimal_action"][e] = d, m, a
        if enable or elapsed[e] == 0:
            record.start[e], record.offset[e] = d, elapsed[e]
    return out


def nav_outputs(graphs, geos, scene, state, goal, elapsed, done, truncated, ep_length, record):
    """The six outputs of one step from what the step itself reports. scene / state / goal /
    elapsed describe the env after the step (get_state()); done / truncated / ep_length are the
    step's. `record` is read for the episode the step belonged to and restarted for the envs
    that were just reset (elapsed == 0)."""
    E = len(state)
    out = dict(distance_to_goal=np.zeros(E, np.int32), optimal_mask=np.zeros(E, np.uint8),
               optimal_action=np.zeros(E, np.int32), success=np.zeros(E, bool),
               spl=np.zeros(E, np.float32), start_distance=np.zeros(E, np.int32))
    for e in range(E):
        k = int(scene[e])
        d, m, a = distance_mask_action(graphs[k], geos[k], int(state[e]), int(goal[e]))
        out["distance_to_goal"][e], out["optimal_mask"][e], out["optimal_action"][e] = d, m, a
        l = int(record.start[e])
        ok = bool(done[e]) and not bool(truncated[e])
        out["start_distance"][e] = l
        out["success"][e] = ok
        out["spl"][e] = spl_value(ok, l, int(ep_length[e]) - int(record.offset[e]))
        if elapsed[e] == 0:
            record.start[e], record.offset[e] = d, 0
    return out


# ---- the three scenes the nav tests share (one frame shape, synthetic frames) ---------------
MAZE_A = np.ones((5, 5), dtype=bool)
for _c in ((1, 1), (3, 2), (1, 3)):
    MAZE_A[_c] = False

# (c): one-way ring 0->1->2->3->0 on action 0, 1->0 on action 3, spur 3->4 on action 1 with no
# way back, self loop 4->4 on action 2, island 5<->6 on action 0
GRAPH_C = np.full((7, 4), -1, dtype=np.int64)
GRAPH_C[0, 0], GRAPH_C[1, 0], GRAPH_C[2, 0], GRAPH_C[3, 0] = 1, 2, 3, 0
GRAPH_C[1, 3] = 0
GRAPH_C[3, 1] = 4
GRAPH_C[4, 2] = 4
GRAPH_C[5, 0], GRAPH_C[6, 0] = 6, 5
# rows = state, columns = goal (the transpose of the [goal, state] layout)
TABLE_C = np.array([[0, 1, 2, 3, 4, -1, -1], [1, 0, 1, 2, 3, -1, -1], [2, 3, 0, 1, 2, -1, -1],
                    [1, 2, 3, 0, 1, -1, -1], [-1, -1, -1, -1, 0, -1, -1], [-1, -1, -1, -1, -1, 0, 1],
                    [-1, -1, -1, -1, -1, 1, 0]], dtype=np.int16)


def scene_a():
    m = maze_scene(MAZE_A, (4, 4))
    return Scene(graph=m.graph, spd=m.spd, frame_shape=FRAME, observations=None, synth_id=0,
                 rewards=m.rewards, terminal_obs=1, name="nav-a")


def scene_b():
    s = synthetic_scene(0, grid=6)
    return Scene(graph=s.graph, spd=s.spd, frame_shape=FRAME, observations=None, synth_id=1,
                 rewards=s.rewards, terminal_obs=0, name="nav-b")


def scene_c():
    spd = np.ones((7, 7), dtype=np.int64) - np.eye(7, dtype=np.int64)
    return Scene(graph=GRAPH_C, spd=spd, frame_shape=FRAME, observations=None, synth_id=2, terminal_obs=0,
                 name="nav-c")


def shared_scenes():
    return [scene_a(), scene_b(), scene_c()]
