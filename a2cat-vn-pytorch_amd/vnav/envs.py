"""VectorEnv — the batched cached-scene environment on one GPU.

Drop-in for the deep_rl ``SubprocVecEnv`` of THORDiscreteCachedEnv / THORCachedEnv
processes (experiments/thor_cached_auxiliary.py:58-71): ``reset()``, ``step(actions)``
with baselines-style auto-reset, ``call_unwrapped('set_complexity', x)`` and
``set_hardness``. Every env lives on the device; a step is one HIP launch
(``vn_step`` in libvnav.so) — there is no per-env process, pipe or host copy.

Observations are the tuple ``(image, goal)`` of uint8 ``[E,H,W,C]`` device tensors (the
raw cached frames, cached.py:59-60 / gym_thor_cached.py:52-53). The reference
wrapper chain TransposeImage + ScaledFloatFrame is ``obs_format="f32_chw"``: the step
itself then emits float32 ``[E,C,H,W]`` in [0, 1] (``vn_step_f32``), with the wrappers'
arithmetic bit for bit. ``to_float_chw`` below is the same chain in torch, for frames that
are already out of the env; the policy kernels consume the uint8 frames directly and fuse
that conversion.

``aux_observations=True`` (AuxiliaryGraph-v0) makes the observation the reference's five-tuple
``(image, goal, depth, segmentation, goal segmentation)``; with the aux frames in the format of
the image frames all five leave the scene cache in the step's own launch (``vn_step_aux``).

``nav_info=True`` adds the navigation info to every step's ``info``: the geodesic distance to the
goal on the scene's action graph, the optimal action(s), and per finished episode success, SPL
and start distance (``vn_nav_enable``; tables built on the device, one small launch per step).
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from .scenes import Scene, resize_scene

OBS_FORMATS = ("u8_hwc", "f32_chw")
AUX_KEYS = ("depth", "segmentation", "goal_segmentation")
ST_FIELDS = ("scene", "state", "goal", "obs_state", "elapsed", "episode", "sched_pos")
# info keys of nav_info=True, in vn_set_nav_buffers' order, with their dtypes
NAV_KEYS = (("distance_to_goal", torch.int32), ("optimal_action", torch.int32), ("optimal_mask", torch.uint8),
            ("success", torch.bool), ("spl", torch.float32), ("start_distance", torch.int32))
# info keys of nav_progress=True (set_nav_progress), both int32
PROGRESS_KEYS = ("distance_before", "progress")
# info keys of visit_counts=True (set_visit_counts), in vn_set_visit_outputs' order
VISIT_KEYS = (("visit_cell", torch.int32), ("first_visit", torch.bool), ("coverage", torch.int32))


class _DeviceWords:
    """A span of 32-bit words in device memory the library owns, for torch.as_tensor."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(int(n),), typestr="<i4", data=(int(ptr), False), version=2)


def to_float_chw(frames):
    """TransposeImage + ScaledFloatFrame: uint8 [...,H,W,C] -> float32 [...,C,H,W] / 255."""
    return frames.permute(*range(frames.dim() - 3), -1, -3, -2).to(torch.float32) / 255.0


class EpisodeLog:
    """The per-episode log's device tensors (VectorEnv.set_episode_log): slot k of env e is
    element [k, e]; only slots k < min(count[e], want[e]) hold an episode."""
    FIELDS = (("success", torch.uint8), ("length", torch.int32), ("start_distance", torch.int32),
              ("spl", torch.float32), ("ep_return", torch.float32))

    def __init__(self, capacity, want, num_envs, device):
        self.capacity = capacity
        self.want = want
        self.count = torch.zeros(num_envs, dtype=torch.int32, device=device)
        for k, dt in self.FIELDS:
            setattr(self, k, torch.zeros((capacity, num_envs), dtype=dt, device=device))

    def _struct(self):
        return _lib.EpisodeLog(self.capacity, *[t.data_ptr() for t in (
            self.want, self.count, self.success, self.length, self.start_distance, self.spl, self.ep_return)])

    def remaining(self):
        """Episodes still to record, summed over envs (a device scalar)."""
        return (self.want - self.count).clamp(min=0).sum()


class VectorEnv:
    num_actions = 4  # THORDiscreteCachedEnv.get_action_size (cached.py:66-68)

    def __init__(self, scenes, num_envs, seed=0, device=None, max_episode_steps=900, tasks=None,
                 env_scenes=None, autoreset=True, aux_observations=False, reuse_outputs=True,
                 obs_format="u8_hwc", aux_format=None, nav_info=False, image_size=None, nav_progress=False,
                 visit_counts=False):
        """obs_format: "u8_hwc" (default) returns and takes uint8 [E,H,W,C] frames; "f32_chw"
        returns and takes float32 [E,C,H,W] frames in [0, 1], every value float(u8) / 255 as
        fp32 division (ScaledFloatFrame's), converted in the step's own launch with the same
        ``out=`` fast path and reuse contract. ``obs_shape`` is the shape of one returned frame.
        aux_format: the format of the extra depth / segmentation frames of
        ``aux_observations=True``. None or "u8_hwc" (default): uint8 [E,H,W,1] / [E,H,W,3] in
        either obs_format; "f32_chw": float32 [E,1,H,W] / [E,3,H,W], only together with
        ``obs_format="f32_chw"``. When both formats are equal the five frames are written by one
        launch (vn_step_aux) and ``out=`` may carry the three aux buffers (``step``).
        nav_info: every step's info also carries ``distance_to_goal`` (least number of actions
        to the goal on the scene's action graph, -1 = unreachable), ``optimal_action`` /
        ``optimal_mask`` (a / all first actions of a shortest path, -1 / 0 if none), and the
        episode's ``success``, ``spl`` and ``start_distance``.
        nav_progress: with nav_info, every step's info also carries ``distance_before`` (the
        distance to the goal before the step) and ``progress`` (how many actions closer the step
        brought the env, 0 where the goal is unreachable; ``set_nav_progress``). ``reward`` stays
        the environment's own.
        visit_counts: keep a visit count per (scene, state) and the running episode's set of
        seen states on the device (``set_visit_counts``; needs no nav_info): every step's info
        also carries ``visit_cell``, ``first_visit`` and, per finished episode, ``coverage``.
        image_size: (height, width) of the frames the env emits, the reference cached env's
        ``image_size`` (cached.py:19,62-64). Every scene whose frames have another size is
        resized on the device before the scene cache is built (``scenes.resize_scene``); None
        (default) and scenes already of that size are left untouched."""
        if obs_format not in OBS_FORMATS:
            raise ValueError("obs_format must be one of %s, got %r" % (OBS_FORMATS, obs_format))
        if aux_format is not None and aux_format not in OBS_FORMATS:
            raise ValueError("aux_format must be None or one of %s, got %r" % (OBS_FORMATS, aux_format))
        if aux_format == "f32_chw" and obs_format != "f32_chw":
            raise ValueError('aux_format="f32_chw" needs obs_format="f32_chw" (got %r)' % (obs_format,))
        if isinstance(scenes, Scene):
            scenes = [scenes]
        if not scenes:
            raise ValueError("VectorEnv needs at least one scene")
        if not torch.cuda.is_available():
            raise _lib.VnavError("VectorEnv requires a ROCm GPU (no CPU fallback)")
        self.lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   torch.device(device).index or 0)
        self.scenes = list(scenes)
        if image_size is not None:
            hw = tuple(int(v) for v in image_size)
            self.scenes = [s if tuple(s.frame_shape[:2]) == hw else resize_scene(s, hw, device=self.device)
                           for s in self.scenes]
        self.num_envs = int(num_envs)
        self.seed = int(seed)
        self.frame_shape = tuple(self.scenes[0].frame_shape)
        self.obs_format = obs_format
        if obs_format == "f32_chw":
            self.obs_shape = (self.frame_shape[2],) + self.frame_shape[:2]
            self._obs_dtype = torch.float32
            self._vn_step, self._vn_observe = self.lib.vn_step_f32, self.lib.vn_observe_f32
        else:
            self.obs_shape = self.frame_shape
            self._obs_dtype = torch.uint8
            self._vn_step, self._vn_observe = self.lib.vn_step, self.lib.vn_observe
        descs = (_lib.SceneDesc * len(self.scenes))()
        self._keep = []
        for i, s in enumerate(self.scenes):
            d = descs[i]
            d.n_states = s.n_states
            d.height, d.width, d.channels = s.frame_shape
            d.graph = s.graph.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
            d.spd = s.spd.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
            if s.observations is not None:
                d.observations = s.observations.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
            d.reward_goal, d.reward_step, d.reward_collision = s.rewards
            d.terminal_obs = s.terminal_obs
            if s.companion is not None:
                d.companion = s.companion.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
            d.synth_id = s.synth_id
            self._keep.append(s)
        handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vn_create(descs, len(self.scenes), self.num_envs,
                                          ctypes.c_uint64(self.seed & (2**64 - 1)),
                                          self.device.index, ctypes.byref(handle)), "vn_create")
        self._ctx = handle
        self.nav_info = False
        self.nav_progress = False
        self._progress_home = (None, None)
        self.visit_counts = False
        self._visit_home = (None, None, None)
        self.episode_log = None
        self.geo_curriculum = None  # set_geodesic_curriculum's configuration while it is on
        # the env -> scene assignment (vn_set_env_scenes; the native default)
        self.env_scenes = np.arange(self.num_envs, dtype=np.int32) % len(self.scenes)
        # bumped by every call that replaces the kernels' per-ctx configuration (tables,
        # schedules, limits): a captured hipGraph holds the old launch arguments and must be
        # recaptured (A2CTrainer checks it before each replay)
        self.config_generation = 0
        self._out_cache = None
        self._aux_cache = None
        # output reuse (vn_set_output_reuse): armed only while the caller
        # steps into its own buffers; _reuse_on mirrors the native switch
        self.reuse_outputs = bool(reuse_outputs)
        self._reuse_on = False
        E = self.num_envs
        kw = dict(device=self.device)
        self._info = dict(
            ep_return=torch.zeros(E, dtype=torch.float32, **kw),
            ep_length=torch.zeros(E, dtype=torch.int32, **kw),
            terminal_state=torch.zeros(E, dtype=torch.int32, **kw),
            truncated=torch.zeros(E, dtype=torch.uint8, **kw),
            img_row=torch.zeros(E, dtype=torch.int32, **kw),
            goal_row=torch.zeros(E, dtype=torch.int32, **kw),
        )
        self.set_row_outputs(None, None)
        self.set_max_episode_steps(max_episode_steps)
        if not autoreset:
            _lib.check(self.lib.vn_set_autoreset(self._ctx, 0), "vn_set_autoreset")
        if env_scenes is not None:
            self.set_env_scenes(env_scenes)
        if tasks is None and all(s.goals for s in self.scenes):
            # the scenes' own fixed goal lists (OrientedGraphEnv goals, MazeGraph goal)
            tasks = [(i, g) for i, s in enumerate(self.scenes) for g in s.goals]
        if tasks:
            self.set_tasks(tasks)
        self.complexity = None
        self._schedule = None
        self.aux_arena = None
        if all(s.depth is not None and s.segmentation is not None for s in self.scenes):
            self.aux_arena = self._build_aux_arena()
        self.aux_observations = bool(aux_observations)
        if self.aux_observations and self.aux_arena is None:
            raise ValueError("aux_observations needs depth + segmentation on every scene")
        self.aux_format = aux_format or "u8_hwc"
        self._aux_dtype = torch.float32 if self.aux_format == "f32_chw" else torch.uint8
        # all five frames in one format: the five-frame entry points (vn_step_aux). The mixed
        # pair (float image / goal, uint8 aux frames) stays vn_step_f32 + three row gathers
        self._aux_fused = self.aux_observations and self.aux_format == self.obs_format
        H, W = self.frame_shape[:2]
        if self.aux_arena is not None:
            dc, sc = int(self.aux_arena[0].shape[3]), int(self.aux_arena[1].shape[3])
            chw = self.aux_format == "f32_chw"
            self.aux_shapes = tuple((c, H, W) if chw else (H, W, c) for c in (dc, sc, sc))
        if nav_info:
            self.set_nav_info(True)
        if nav_progress:
            if not nav_info:
                raise ValueError("nav_progress=True needs nav_info=True")
            self.set_nav_progress(True)
        if visit_counts:
            self.set_visit_counts(True)

    def _build_aux_arena(self):
        """Depth [rows,H,W,1] and segmentation [rows,H,W,3] uint8 on the device, indexed by
        the frame arena's rows (so info img_row / goal_row address them too)."""
        _, _, rows, bases = self.frame_arena()
        H, W = self.frame_shape[:2]
        depth = torch.zeros((rows, H, W, 1), dtype=torch.uint8, device=self.device)
        seg = torch.zeros((rows, H, W, 3), dtype=torch.uint8, device=self.device)
        for s, b in zip(self.scenes, bases):
            depth[b:b + s.n_states].copy_(torch.from_numpy(s.depth))
            seg[b:b + s.n_states].copy_(torch.from_numpy(s.segmentation))
        # the context borrows both tensors (kept alive as self.aux_arena) for vn_step_aux
        torch.cuda.synchronize(self.device)
        self.config_generation += 1
        _lib.check(self.lib.vn_set_aux_arena(self._ctx, _lib.ptr(depth), int(depth.shape[3]), _lib.ptr(seg),
                                             int(seg.shape[3])), "vn_set_aux_arena")
        return depth, seg

    def _gather_aux(self):
        """(depth, segmentation, goal segmentation) of the current observation by row."""
        depth, seg = self.aux_arena
        E = self.num_envs
        out = []
        for src, rows in ((depth, self._info["img_row"]), (seg, self._info["img_row"]), (seg, self._info["goal_row"])):
            dst = torch.empty((E,) + tuple(src.shape[1:]), dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.vn_gather_rows(_lib.ptr(src), int(src[0].numel()), _lib.ptr(rows), E, _lib.ptr(dst),
                                               self._stream()), "vn_gather_rows")
            out.append(dst)
        return tuple(out)

    # -- navigation info -----------------------------------------------------
    def set_nav_info(self, on, buffers=None):
        """Enable / disable the navigation info (vn_nav_enable): builds the scenes' geodesic
        tables on the device and adds NAV_KEYS to info. Episodes already running are measured
        from here. ``buffers``: the caller's own [E] output tensors in NAV_KEYS' order (any may
        be None: not written), e.g. a trainer's rollout slots; default the env's own."""
        if on:
            if buffers is None:
                buffers = [torch.zeros(self.num_envs, dtype=dt, device=self.device) for _, dt in NAV_KEYS]
            buffers = list(buffers)
            if len(buffers) != len(NAV_KEYS):
                raise ValueError("nav buffers: one per key of %s" % ([k for k, _ in NAV_KEYS],))
            for (k, dt), t in zip(NAV_KEYS, buffers):
                self._check_out(k, t, dt, self.num_envs)
        self.config_generation += 1
        for k, _ in NAV_KEYS:
            self._info.pop(k, None)
        self.nav_info = False
        self._drop_progress()  # vn_nav_enable switches progress off first
        self.episode_log = None  # the log lives in the nav state
        self.geo_curriculum = None  # vn_nav_enable switches the geodesic curriculum off first
        _lib.check(self.lib.vn_nav_enable(self._ctx, 1 if on else 0), "vn_nav_enable")
        if not on:
            return
        torch.cuda.synchronize(self.device)  # the buffers' zero fill precedes the call's own write
        _lib.check(self.lib.vn_set_nav_buffers(self._ctx, *[_lib.ptr(t) for t in buffers]), "vn_set_nav_buffers")
        self.nav_info = True
        for (k, _), t in zip(NAV_KEYS, buffers):
            if t is not None:
                self._info[k] = t

    def nav_outputs(self):
        """The env's own navigation buffers by info key (no copies): after reset() the first
        three hold the new episodes' values, after a step all six hold the step's."""
        self._need_nav()
        return {k: self._info[k] for k, _ in NAV_KEYS if k in self._info}

    def set_nav_mask_output(self, mask):
        """Where the next steps write ``optimal_mask``: a uint8 [E] device tensor (e.g. a
        trainer's per-step slot, so no copy follows each step), or None for the buffer
        set_nav_info() was given (vn_set_nav_mask_output: a pointer swap, no launch, no sync).
        The other navigation outputs stay where they are. The caller keeps the tensor alive."""
        self._need_nav()
        self._check_out("optimal_mask", mask, torch.uint8, self.num_envs)
        _lib.check(self.lib.vn_set_nav_mask_output(self._ctx, _lib.ptr(mask)), "vn_set_nav_mask_output")

    def refresh_nav_outputs(self):
        """Rewrite distance, mask and action of every env's current state into the env's
        navigation buffers (vn_set_nav_buffers with the same buffers: synchronises). For use
        after set_state() + set_nav_state(), which leave them at the states before."""
        self._need_nav()
        bufs = [self._info.get(k) for k, _ in NAV_KEYS]
        torch.cuda.synchronize(self.device)
        _lib.check(self.lib.vn_set_nav_buffers(self._ctx, *[_lib.ptr(t) for t in bufs]), "vn_set_nav_buffers")

    def _need_nav(self):
        if not self.nav_info:
            raise _lib.VnavError("navigation info is off: VectorEnv(..., nav_info=True)")

    def geodesic(self, scene_index):
        """The scene's action-graph geodesic table: int16 [N, N] device tensor indexed
        [goal, state] (a copy; -1 = the goal cannot be reached from the state)."""
        self._need_nav()
        p, n = ctypes.c_void_p(), ctypes.c_int32()
        _lib.check(self.lib.vn_nav_table(self._ctx, int(scene_index), ctypes.byref(p), ctypes.byref(n)),
                   "vn_nav_table")
        out = torch.empty((n.value, n.value), dtype=torch.int16, device=self.device)
        rows = torch.arange(n.value, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.vn_gather_rows(p, 2 * n.value, _lib.ptr(rows), n.value, _lib.ptr(out), self._stream()),
                   "vn_gather_rows")
        rows.record_stream(torch.cuda.current_stream(self.device))
        return out

    def nav_episode_stats(self, out=None):
        """float32 [4]: finished episodes, successes, SPL sum, start-distance sum over all envs
        since the last call (vn_nav_episode_stats: fixed-order sums, then zeroed)."""
        self._need_nav()
        if out is None:
            out = torch.empty(4, dtype=torch.float32, device=self.device)
        else:
            self._check_out("nav stats", out, torch.float32, 4)
        _lib.check(self.lib.vn_nav_episode_stats(self._ctx, _lib.ptr(out), self._stream()), "vn_nav_episode_stats")
        return out

    def get_nav_state(self):
        """The nav record a checkpoint needs: int32 [2, E] (start distance, length offset)."""
        self._need_nav()
        buf = torch.empty((2, self.num_envs), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.vn_get_nav_state(self._ctx, _lib.ptr(buf), self._stream()), "vn_get_nav_state")
        return buf

    def set_nav_state(self, buf):
        """Restore get_nav_state()'s table; call it right after set_state()."""
        self._need_nav()
        buf = torch.as_tensor(buf)
        if tuple(buf.shape) != (2, self.num_envs):
            raise ValueError("nav state must be [2, %d] (this env), got %s" % (self.num_envs, tuple(buf.shape)))
        buf = buf.to(device=self.device, dtype=torch.int32).contiguous()
        _lib.check(self.lib.vn_set_nav_state(self._ctx, _lib.ptr(buf), self._stream()), "vn_set_nav_state")
        # the copy is stream-ordered: keep the source alive until it has run
        buf.record_stream(torch.cuda.current_stream(self.device))

    # -- geodesic progress (DESIGN.md "Reward shaping and GAE") ------------------
    def _drop_progress(self):
        self.nav_progress = False
        self._progress_home = (None, None)
        for k in PROGRESS_KEYS:
            self._info.pop(k, None)

    def _need_progress(self):
        if not self.nav_progress:
            raise _lib.VnavError("progress is off: VectorEnv(..., nav_info=True, nav_progress=True)")

    def set_nav_progress(self, on, buffers=None):
        """Enable / disable the per-step geodesic progress (vn_nav_progress; needs nav_info):
        info gains ``distance_before`` and ``progress``, int32 [E]. Episodes already running are
        measured from their current state. ``buffers``: the caller's own (distance_before,
        progress) tensors, either may be None (not written); default the env's own. The step's
        ``reward``, ``ep_return`` and every other output are unchanged: a shaped reward is formed
        by the trainer from these distances (A2CTrainer(shaping_weight=...))."""
        if on:
            self._need_nav()
            if buffers is None:
                buffers = [torch.zeros(self.num_envs, dtype=torch.int32, device=self.device) for _ in PROGRESS_KEYS]
            buffers = list(buffers)
            if len(buffers) != len(PROGRESS_KEYS):
                raise ValueError("progress buffers: one per key of %s" % (PROGRESS_KEYS,))
            for k, t in zip(PROGRESS_KEYS, buffers):
                self._check_out(k, t, torch.int32, self.num_envs)
        elif not self.nav_info:
            self._drop_progress()
            return
        self.config_generation += 1
        self._drop_progress()
        _lib.check(self.lib.vn_nav_progress(self._ctx, 1 if on else 0), "vn_nav_progress")
        if not on:
            return
        self.nav_progress = True
        self._progress_home = tuple(buffers)
        for k, t in zip(PROGRESS_KEYS, buffers):
            if t is not None:
                self._info[k] = t
        self.set_nav_progress_outputs(None, None, None)

    def set_nav_progress_outputs(self, before, after, progress=None):
        """Where the next steps write the distance before the step, the distance after it and
        the progress: int32 [E] device tensors, e.g. a trainer's per-step slots (any None: not
        written). All three None: back to the buffers set_nav_progress() was given
        (vn_set_nav_progress_outputs: a pointer swap, no launch, no sync). The caller keeps the
        tensors alive while steps may write them."""
        self._need_progress()
        if before is None and after is None and progress is None:
            before, progress = self._progress_home
        for k, t in (("distance_before", before), ("distance_after", after), ("progress", progress)):
            self._check_out(k, t, torch.int32, self.num_envs)
        _lib.check(self.lib.vn_set_nav_progress_outputs(self._ctx, _lib.ptr(before), _lib.ptr(after),
                                                        _lib.ptr(progress)), "vn_set_nav_progress_outputs")

    def get_nav_progress_state(self):
        """The progress record a checkpoint needs: int32 [3, E] (scene, goal, distance)."""
        self._need_progress()
        buf = torch.empty((3, self.num_envs), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.vn_get_nav_progress_state(self._ctx, _lib.ptr(buf), self._stream()),
                   "vn_get_nav_progress_state")
        return buf

    def set_nav_progress_state(self, buf):
        """Restore get_nav_progress_state()'s table; call it after set_state(), which starts the
        record again from the states it sets."""
        self._need_progress()
        buf = torch.as_tensor(buf)
        if tuple(buf.shape) != (3, self.num_envs):
            raise ValueError("progress state must be [3, %d] (this env), got %s" % (self.num_envs, tuple(buf.shape)))
        buf = buf.to(device=self.device, dtype=torch.int32).contiguous()
        _lib.check(self.lib.vn_set_nav_progress_state(self._ctx, _lib.ptr(buf), self._stream()),
                   "vn_set_nav_progress_state")
        buf.record_stream(torch.cuda.current_stream(self.device))

    # -- visit counts (DESIGN.md "Visit counts and novelty bonus") ----------------
    def _drop_visits(self):
        self.visit_counts = False
        self._visit_home = (None, None, None)
        for k, _ in VISIT_KEYS:
            self._info.pop(k, None)

    def _need_visits(self):
        if not self.visit_counts:
            raise _lib.VnavError("visit counts are off: VectorEnv(..., visit_counts=True)")

    def set_visit_counts(self, on, buffers=None):
        """Enable / disable the visit counts (vn_visit_enable; independent of nav_info): the
        device keeps a count per (scene, state) of how often an env arrived there, and per env
        the set of states its running episode has seen. info gains ``visit_cell`` (int32: the
        arrival state's index in the table of all scenes, ``visit_cells()``), ``first_visit``
        (bool: the episode had not been there) and ``coverage`` (int32: the finished episode's
        number of distinct states where ``done``, else 0). Episodes already running are covered
        from their current state, which is counted once. ``buffers``: the caller's own tensors
        in VISIT_KEYS' order, any may be None (not written); default the env's own. Replaces
        launch arguments: a captured graph must be recaptured."""
        if on:
            if buffers is None:
                buffers = [torch.zeros(self.num_envs, dtype=dt, device=self.device) for _, dt in VISIT_KEYS]
            buffers = list(buffers)
            if len(buffers) != len(VISIT_KEYS):
                raise ValueError("visit buffers: one per key of %s" % ([k for k, _ in VISIT_KEYS],))
            for (k, dt), t in zip(VISIT_KEYS, buffers):
                self._check_out(k, t, dt, self.num_envs)
        self.config_generation += 1
        _lib.check(self.lib.vn_visit_enable(self._ctx, 1 if on else 0), "vn_visit_enable")
        self._drop_visits()
        if not on:
            return
        self.visit_counts = True
        self._visit_home = tuple(buffers)
        for (k, _), t in zip(VISIT_KEYS, buffers):
            if t is not None:
                self._info[k] = t
        self.set_visit_outputs(None, None, None)

    def set_visit_outputs(self, cell, first, coverage=None):
        """Where the next steps write the visit outputs: [E] device tensors (int32, bool, int32),
        e.g. a trainer's per-step slots (any None: not written). All three None: back to the
        buffers set_visit_counts() was given (vn_set_visit_outputs: a pointer swap, no launch,
        no sync). The caller keeps the tensors alive while steps may write them."""
        self._need_visits()
        if cell is None and first is None and coverage is None:
            cell, first, coverage = self._visit_home
        for (k, dt), t in zip(VISIT_KEYS, (cell, first, coverage)):
            self._check_out(k, t, dt, self.num_envs)
        _lib.check(self.lib.vn_set_visit_outputs(self._ctx, _lib.ptr(cell), _lib.ptr(first), _lib.ptr(coverage)),
                   "vn_set_visit_outputs")

    def visit_cells(self):
        """(count pointer, cell_off pointer, C) of the table of all scenes (vn_visit_cells): raw
        device addresses for the kernels, valid until the next set_visit_counts()."""
        self._need_visits()
        p, q, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        _lib.check(self.lib.vn_visit_cells(self._ctx, ctypes.byref(p), ctypes.byref(q), ctypes.byref(n)),
                   "vn_visit_cells")
        return p.value, q.value, n.value

    def visit_table(self, scene_index):
        """The live visit table of a scene: an int32 [n_states] view of the device memory the
        steps count into (no copy; the table's words are unsigned, so a count of 2^31 or more
        reads negative). Valid until the next set_visit_counts()."""
        self._need_visits()
        p, n = ctypes.c_void_p(), ctypes.c_int32()
        _lib.check(self.lib.vn_visit_table(self._ctx, int(scene_index), ctypes.byref(p), ctypes.byref(n)),
                   "vn_visit_table")
        return torch.as_tensor(_DeviceWords(p.value, n.value), device=self.device)

    def visit_stats(self, scene=None, out=None):
        """int64 [2] device tensor: the number of states with a count > 0 and the sum of the
        counts, of one scene or (None) of all (vn_visit_stats: exact integer sums)."""
        self._need_visits()
        if out is None:
            out = torch.empty(2, dtype=torch.int64, device=self.device)
        else:
            self._check_out("visit stats", out, torch.int64, 2)
        _lib.check(self.lib.vn_visit_stats(self._ctx, -1 if scene is None else int(scene), _lib.ptr(out),
                                           self._stream()), "vn_visit_stats")
        return out

    def clear_visits(self):
        """Zero the table and start every env's episode record from its current state
        (vn_visit_clear: on the current stream, no host value, so it may be captured)."""
        self._need_visits()
        _lib.check(self.lib.vn_visit_clear(self._ctx, self._stream()), "vn_visit_clear")

    def _visit_words(self):
        W = (max(s.n_states for s in self.scenes) + 31) // 32
        return sum(s.n_states for s in self.scenes) + self.num_envs * (2 + W)

    def get_visit_state(self):
        """The visit state a checkpoint needs, one flat int32 tensor: the counts of all scenes,
        the [2, E] record (episode scene, distinct states) and the [E, W] seen bitmaps."""
        self._need_visits()
        buf = torch.empty(self._visit_words(), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.vn_visit_get_state(self._ctx, _lib.ptr(buf), self._stream()), "vn_visit_get_state")
        return buf

    def set_visit_state(self, buf):
        """Restore get_visit_state()'s tensor; call it after set_state(), which starts every
        env's episode record again from the states it sets."""
        self._need_visits()
        buf = torch.as_tensor(buf)
        if tuple(buf.shape) != (self._visit_words(),):
            raise ValueError("visit state must be [%d] (this env), got %s" % (self._visit_words(), tuple(buf.shape)))
        buf = buf.to(device=self.device, dtype=torch.int32).contiguous()
        _lib.check(self.lib.vn_visit_set_state(self._ctx, _lib.ptr(buf), self._stream()), "vn_visit_set_state")
        buf.record_stream(torch.cuda.current_stream(self.device))

    # -- fixed-episode evaluation (DESIGN.md "Fixed-episode evaluation") -------
    def sample_episodes(self, scene_index, count, min_distance=1, max_distance=None, seed=0, salt=0):
        """Draw ``count`` (start, goal) pairs of a scene, with replacement, uniformly among the
        pairs whose action-graph geodesic distance lies in [min_distance, max_distance]
        (vn_nav_sample_episodes: on the device, exact, reproducible from seed and salt).
        Returns (pairs int32 [count, 2] = (start, goal), distance int32 [count], total) with
        total the number of qualifying pairs; total == 0 leaves both tensors at -1."""
        self._need_nav()
        count = int(count)
        hi = 32767 if max_distance is None else int(max_distance)
        pairs = torch.full((max(count, 0), 2), -1, dtype=torch.int32, device=self.device)
        dist = torch.full((max(count, 0),), -1, dtype=torch.int32, device=self.device)
        total = ctypes.c_int64(0)
        _lib.check(self.lib.vn_nav_sample_episodes(self._ctx, int(scene_index), int(min_distance), hi, count,
                                                   ctypes.c_uint64(int(seed) & (2**64 - 1)),
                                                   ctypes.c_uint32(int(salt) & 0xFFFFFFFF), _lib.ptr(pairs),
                                                   _lib.ptr(dist), ctypes.byref(total), self._stream()),
                   "vn_nav_sample_episodes")
        return pairs, dist, total.value

    def set_episode_log(self, capacity, want=None):
        """Record every env's first ``want[e]`` (<= capacity) finished episodes, one slot each
        (vn_nav_set_episode_log). Returns the EpisodeLog holding the device tensors: ``count``
        int32 [E] (episodes finished since the call) and, [capacity, E] each, ``success``,
        ``length``, ``start_distance``, ``spl``, ``ep_return``. ``set_episode_log(None)``
        switches the log off. Replaces launch arguments: a captured graph must be recaptured."""
        self._need_nav()
        self.config_generation += 1
        if capacity is None:
            _lib.check(self.lib.vn_nav_set_episode_log(self._ctx, None), "vn_nav_set_episode_log")
            self.episode_log = None
            return None
        capacity = int(capacity)
        if capacity <= 0:
            raise ValueError("episode log: capacity must be positive")
        want = torch.as_tensor(want).to(device=self.device, dtype=torch.int32).contiguous()
        if want.shape != (self.num_envs,):
            raise ValueError("episode log: want must have one entry per env")
        if int(want.min()) < 0 or int(want.max()) > capacity:
            raise ValueError("episode log: want must lie in 0..capacity")
        log = EpisodeLog(capacity, want, self.num_envs, self.device)
        torch.cuda.synchronize(self.device)  # the buffers' fill precedes the call's own write
        _lib.check(self.lib.vn_nav_set_episode_log(self._ctx, ctypes.byref(log._struct())), "vn_nav_set_episode_log")
        self.episode_log = log
        return log

    # -- geodesic curriculum (DESIGN.md "Geodesic curriculum") ------------------
    def set_geodesic_curriculum(self, level=1, mode=1, window=0, up=0.8, down=0.3, step=1, level_min=1):
        """Draw every reset's start among the states within ``level`` actions of the goal
        (0 < distance_to_goal <= level; vn_nav_curriculum), the unit of ``distance_to_goal``,
        SPL and the EpisodeSet buckets. mode 1: uniform over them; mode 2: with probability 0.9
        among them and 0.1 among the farther states. ``window`` > 0 makes the level adaptive, per
        scene and on the device: once ``window`` episodes of a scene have finished,
        ``curriculum_advance()`` raises its level by ``step`` if their success rate is >= ``up``
        and lowers it (not below ``level_min``) if it is <= ``down``; levels stay within the
        scene's largest distance. ``level=None`` switches it off and restores the starts there
        were before (a ``set_complexity`` curriculum included). Turns ``nav_info`` on if it was
        off; a captured graph must be recaptured after this call, but not when the level moves.
        Costs N^2 int32 of device memory per scene, as ``set_complexity``'s table does."""
        self.config_generation += 1
        if level is None:
            if self.geo_curriculum is not None:
                _lib.check(self.lib.vn_nav_curriculum(self._ctx, None), "vn_nav_curriculum")
            self.geo_curriculum = None
            return
        cfg = dict(mode=int(mode), level=int(level), level_min=int(level_min), step=int(step), window=int(window),
                   up=float(up), down=float(down))
        if not self.nav_info:
            self.set_nav_info(True)
        c = _lib.GeoCurriculum(**cfg)
        _lib.check(self.lib.vn_nav_curriculum(self._ctx, ctypes.byref(c)), "vn_nav_curriculum")
        self.geo_curriculum = cfg

    def _need_curriculum(self):
        if self.geo_curriculum is None:
            raise _lib.VnavError("the geodesic curriculum is off: set_geodesic_curriculum(level, ...)")

    def curriculum_advance(self):
        """One level decision per scene whose window is full (vn_nav_curriculum_advance): one
        small launch on the current stream, no host value, so it may be captured in a graph.
        Nothing is launched with ``window=0``."""
        self._need_curriculum()
        _lib.check(self.lib.vn_nav_curriculum_advance(self._ctx, self._stream()), "vn_nav_curriculum_advance")

    def curriculum_state(self, out=None):
        """int32 [4, S] device tensor: per scene the level, the finished episodes and successes
        of the running window, and the scene's largest distance D."""
        self._need_curriculum()
        S = len(self.scenes)
        if out is None:
            out = torch.empty((4, S), dtype=torch.int32, device=self.device)
        else:
            self._check_out("curriculum state", out, torch.int32, 4 * S)
        _lib.check(self.lib.vn_nav_curriculum_get_state(self._ctx, _lib.ptr(out), self._stream()),
                   "vn_nav_curriculum_get_state")
        return out

    def set_curriculum_state(self, t):
        """Restore curriculum_state()'s table (rows level, done, succ; D is the scenes' own):
        an int32 [4, S] tensor on the env's device. Call it after set_state()."""
        self._need_curriculum()
        S = len(self.scenes)
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise ValueError("curriculum state must be a tensor on %s" % (self.device,))
        if t.dtype != torch.int32 or tuple(t.shape) != (4, S):
            raise ValueError("curriculum state must be int32 [4, %d], got %s %s" % (S, t.dtype, tuple(t.shape)))
        t = t.contiguous()
        _lib.check(self.lib.vn_nav_curriculum_set_state(self._ctx, _lib.ptr(t), self._stream()),
                   "vn_nav_curriculum_set_state")
        t.record_stream(torch.cuda.current_stream(self.device))

    def curriculum_tables(self, scene_index):
        """(order int32 [N, N], count int32 [N, D + 2]) of a scene, indexed by goal (copies):
        the states sorted stably by distance to the goal, and the number of states per goal with
        clamp(distance, -1, D) + 1 <= b."""
        self._need_curriculum()
        po, pc, n, D = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self.lib.vn_nav_curriculum_tables(self._ctx, int(scene_index), ctypes.byref(po), ctypes.byref(pc),
                                                     ctypes.byref(n), ctypes.byref(D)), "vn_nav_curriculum_tables")
        out = []
        for p, cols in ((po, n.value), (pc, D.value + 2)):
            t = torch.empty((n.value, cols), dtype=torch.int32, device=self.device)
            # a scene's block is only 4-byte aligned: rows the copy would move as 16-byte
            # lanes from such a base go element by element instead
            per = cols if (p.value % 16 == 0 or (4 * cols) % 16 != 0) else 1
            rows = torch.arange(n.value * cols // per, dtype=torch.int32, device=self.device)
            _lib.check(self.lib.vn_gather_rows(p, 4 * per, _lib.ptr(rows), rows.numel(), _lib.ptr(t), self._stream()),
                       "vn_gather_rows")
            rows.record_stream(torch.cuda.current_stream(self.device))
            out.append(t)
        return tuple(out)

    # -- configuration -------------------------------------------------------
    def set_max_episode_steps(self, n):
        self.max_episode_steps = int(n or 0)
        self.config_generation += 1
        _lib.check(self.lib.vn_set_max_episode_steps(self._ctx, int(n or 0)), "vn_set_max_episode_steps")

    def set_tasks(self, tasks):
        """tasks: [(scene_index, goal_state or -1)] sampled uniformly at each reset."""
        arr = np.ascontiguousarray(np.asarray(tasks, dtype=np.int32).reshape(-1, 2))
        self.config_generation += 1
        _lib.check(self.lib.vn_set_tasks(self._ctx, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(arr)),
                   "vn_set_tasks")

    def set_env_scenes(self, env_scenes):
        arr = np.ascontiguousarray(np.asarray(env_scenes, dtype=np.int32))
        if arr.shape != (self.num_envs,):
            raise ValueError("env_scenes must have one entry per env")
        self.config_generation += 1
        _lib.check(self.lib.vn_set_env_scenes(self._ctx, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
                   "vn_set_env_scenes")
        self.env_scenes = arr.copy()

    def set_schedule(self, schedule):
        """Exact-replay test mode: schedule [E, L, 2] int32 (start, goal) per reset."""
        self.config_generation += 1
        if schedule is None:
            _lib.check(self.lib.vn_set_schedule(self._ctx, None, 0), "vn_set_schedule")
            self._schedule = None
            return
        sched = torch.as_tensor(schedule, dtype=torch.int32).to(self.device).contiguous()
        if sched.dim() != 3 or sched.shape[0] != self.num_envs or sched.shape[2] != 2:
            raise ValueError("schedule must be [num_envs, L, 2]")
        torch.cuda.synchronize(self.device)
        _lib.check(self.lib.vn_set_schedule(self._ctx, _lib.ptr(sched), sched.shape[1]), "vn_set_schedule")
        self._schedule = sched

    def set_complexity(self, complexity=None, mode=None, offset=None):
        """Curriculum hook (graph/env.py:98-99, environments/gym_graph/graph.py:40-52,
        experiments/thor_cached_auxiliary.py:68-70): subsequent resets draw starts near the
        goal on the device (vn_set_curriculum); None switches back to uniform starts.
        mode/offset default to each scene's own semantics (Scene.curriculum)."""
        if self.geo_curriculum is not None:
            raise _lib.VnavError("set_complexity: the geodesic curriculum is on (set_geodesic_curriculum(None) first)")
        self.complexity = complexity
        self.config_generation += 1
        if complexity is None:
            _lib.check(self.lib.vn_set_curriculum(self._ctx, 0.0, 0, 0.0), "vn_set_curriculum")
            return
        modes = np.array([s.curriculum[0] if mode is None else int(mode) for s in self.scenes], dtype=np.int32)
        offs = np.array([s.curriculum[1] if offset is None else float(offset) for s in self.scenes], dtype=np.float64)
        _lib.check(self.lib.vn_set_curriculum_scenes(self._ctx, float(complexity), modes.ctypes.data_as(ctypes.c_void_p),
                                                     offs.ctypes.data_as(ctypes.c_void_p)), "vn_set_curriculum_scenes")

    set_hardness = set_complexity

    def call_unwrapped(self, name, *args, **kwargs):
        return getattr(self, name)(*args, **kwargs)

    # -- gym VecEnv API -------------------------------------------------------
    def _stream(self):
        return _lib.stream_ptr(self.device)

    def set_row_outputs(self, img_rows, goal_rows):
        """Where the next steps write the arena rows of the frames they emit: int32 [E] device
        tensors (e.g. the trainer's per-step rollout slots, so no copy follows each step), or
        None for this env's own info["img_row"] / info["goal_row"]."""
        i = self._info
        if img_rows is None:
            img_rows, goal_rows = i["img_row"], i["goal_row"]
        self._check_out("img_rows", img_rows, torch.int32, self.num_envs)
        self._check_out("goal_rows", goal_rows, torch.int32, self.num_envs)
        _lib.check(self.lib.vn_set_info_buffers(self._ctx, _lib.ptr(i["ep_return"]), _lib.ptr(i["ep_length"]),
                                                _lib.ptr(i["terminal_state"]), _lib.ptr(i["truncated"]),
                                                _lib.ptr(img_rows), _lib.ptr(goal_rows)), "vn_set_info_buffers")

    def _check_out(self, name, t, dtype, numel):
        """Caller-owned output buffers are written by the kernel through raw pointers: refuse
        anything the launch would write past or misread (wrong device, dtype, size, layout)."""
        if t is None:
            return
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise ValueError("%s must be a tensor on %s" % (name, self.device))
        if t.dtype != dtype or not t.is_contiguous() or t.numel() != numel:
            raise ValueError("%s must be a contiguous %s tensor of %d elements (got %s, %d, contiguous=%s)"
                             % (name, dtype, numel, t.dtype, t.numel(), t.is_contiguous()))

    def _check_frames_out(self, img, goal):
        F = int(np.prod(self.frame_shape))
        self._check_out("image", img, self._obs_dtype, self.num_envs * F)
        self._check_out("goal", goal, self._obs_dtype, self.num_envs * F)

    def _frames(self):
        shape = (self.num_envs,) + self.obs_shape
        return (torch.empty(shape, dtype=self._obs_dtype, device=self.device),
                torch.empty(shape, dtype=self._obs_dtype, device=self.device))

    def _arm_reuse(self):
        """The caller's own buffers were (re)validated: the next launch writes every row, later
        ones may skip rows that already hold their frame. Also called for buffers seen before:
        a new tensor at a recycled address must not inherit the old one's record."""
        if self.reuse_outputs:
            _lib.check(self.lib.vn_set_output_reuse(self._ctx, 1), "vn_set_output_reuse")
            self._reuse_on = True

    def _disarm_reuse(self):
        """Fresh output tensors: the allocator may hand back an address whose record still
        matches but whose bytes are someone else's, so every row is written. The cached
        buffers are dropped with it, so the next step(out=...) arms again."""
        if self._reuse_on:
            _lib.check(self.lib.vn_set_output_reuse(self._ctx, 0), "vn_set_output_reuse")
            self._reuse_on = False
            self._out_cache = None
            self._aux_cache = None

    def reset(self, mask=None):
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.int32).contiguous()
            if m.shape != (self.num_envs,):
                raise ValueError("reset mask must have shape [num_envs]")
        _lib.check(self.lib.vn_reset(self._ctx, _lib.ptr(m), self._stream()), "vn_reset")
        return self.observe()

    def observe(self, out=None, gather=True):
        """Current (image, goal) frames in the env's obs_format; gather=False only refreshes
        info img_row/goal_row. With ``aux_observations=True`` the five-tuple, and ``out`` may be
        the five buffers (image, goal, depth, segmentation, goal segmentation)."""
        if not gather:
            _lib.check(self._vn_observe(self._ctx, None, None, None, self._stream()), "vn_observe")
            return None, None
        if self._aux_fused and self._fused(out is not None, out is not None and len(out) > 2):
            return self._observe_aux(out)
        img, goal = out if out is not None else self._frames()
        self._check_frames_out(img, goal)
        if out is None:
            self._disarm_reuse()
        else:
            self._arm_reuse()
        _lib.check(self._vn_observe(self._ctx, _lib.ptr(img), _lib.ptr(goal), None, self._stream()), "vn_observe")
        if self.aux_observations:
            return (img, goal) + self._gather_aux()
        return img, goal

    def step(self, actions, out=None, gather=True):
        """actions: int32 [E] device tensor (other integer dtypes are converted).
        Returns ((image, goal), reward f32 [E], done bool [E], info dict of [E] tensors); the
        frames are uint8 [E,H,W,C], or float32 [E,C,H,W] with ``obs_format="f32_chw"`` (the
        ``out`` image / goal buffers then are float32 too).
        Without ``out`` every returned tensor is fresh, info included (a caller may keep step
        t's results while stepping on). ``out`` = dict of preallocated outputs (image, goal,
        reward, done, state) to write in place: the fast path, where nothing is allocated or
        copied per step and info's tensors (ep_return, ep_length, terminal_state, truncated,
        img_row, goal_row) are the env's own buffers, overwritten by the next step like the
        ``out`` buffers. ``gather=False`` skips the frame copy
        (index-only step: info img_row / goal_row address the frames in the scene cache).
        Contract of ``out`` with ``reuse_outputs=True`` (the default): the step does not copy a
        frame whose row of ``out["image"]`` / ``out["goal"]`` already holds it from this env's
        previous step (the goal between resets, the image on a blocked move), so the image and
        goal rows must be left as the env wrote them until the next step. Rows that are edited
        in place, shared between two envs or written by anything else need
        ``VectorEnv(..., reuse_outputs=False)``, which writes every row on every step.
        With ``aux_observations=True`` and the aux frames in the image frames' format, ``out``
        may also carry ``depth``, ``segmentation`` and ``goal_segmentation`` (all three or none):
        the five frames returned are then the caller's own tensors, under the same contract
        (depth and segmentation are skipped with the image, goal segmentation with the goal),
        and no two of the five may overlap."""
        if type(actions) is torch.Tensor and actions.dtype == torch.int32 and actions.device == self.device \
                and actions.shape == (self.num_envs,) and actions.is_contiguous():
            a = actions
        else:
            a = torch.as_tensor(actions, device=self.device)
            if a.dtype != torch.int32:
                a = a.to(torch.int32)
            a = a.contiguous()
            if a.shape != (self.num_envs,):
                raise ValueError("actions must have shape [num_envs]")
        if self._aux_fused and gather and \
                self._fused(out is not None, out is not None and any(out.get(k) is not None for k in AUX_KEYS)):
            return self._step_aux(a, out)
        if out is not None and gather:
            # the same caller-owned buffers as the previous call: validated then, pointers cached.
            # The key also holds each buffer's current data_ptr and size, so a tensor that was
            # resize_()d or set_() to other storage since is validated again
            bufs = (out["image"], out["goal"], out.get("reward"), out.get("done"), out.get("state"))
            c = self._out_cache
            if c is not None and all(x is y for x, y in zip(bufs, c[0])) and \
                    c[2] == tuple((t.data_ptr(), t.numel()) if t is not None else None for t in bufs):
                P = c[1]
                _lib.check(self._vn_step(self._ctx, _lib.ptr(a), P[0], P[1], P[2], P[3], P[4], self._stream()),
                           "vn_step")
                info = dict(self._info)
                info["state"] = bufs[4]
                if self.aux_observations:
                    return (bufs[0], bufs[1]) + self._gather_aux(), bufs[2], bufs[3], info
                return (bufs[0], bufs[1]), bufs[2], bufs[3], info
        if out is None:
            if gather:
                self._disarm_reuse()
            img, goal = self._frames() if gather else (None, None)
            reward = torch.empty(self.num_envs, dtype=torch.float32, device=self.device)
            done = torch.empty(self.num_envs, dtype=torch.bool, device=self.device)
            state = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        else:
            img, goal = (out["image"], out["goal"]) if gather else (None, None)
            reward, done, state = out.get("reward"), out.get("done"), out.get("state")
            self._check_frames_out(img, goal)
            self._check_out("reward", reward, torch.float32, self.num_envs)
            self._check_out("done", done, torch.bool, self.num_envs)
            self._check_out("state", state, torch.int32, self.num_envs)
            if gather:
                bufs = (img, goal, reward, done, state)
                self._out_cache = (bufs, tuple(_lib.ptr(t) for t in bufs),
                                   tuple((t.data_ptr(), t.numel()) if t is not None else None for t in bufs))
                self._aux_cache = None
                self._arm_reuse()
        _lib.check(self._vn_step(self._ctx, _lib.ptr(a), _lib.ptr(img), _lib.ptr(goal), _lib.ptr(reward),
                                 _lib.ptr(done), _lib.ptr(state), self._stream()), "vn_step")
        # fresh info tensors unless the caller chose the in-place path (out=...)
        info = {k: v.clone() for k, v in self._info.items()} if out is None else dict(self._info)
        info["state"] = state
        if self.aux_observations and gather:
            return (img, goal) + self._gather_aux(), reward, done, info
        return (img, goal), reward, done, info

    # -- the five-frame observation in one launch (vn_step_aux / vn_observe_aux) ------------
    def _fused(self, has_out, has_aux_bufs):
        """Whether this call takes the five-frame entry points. Not with VN_AUX_OBS_GATHER=1
        (read per call: the former step + three vn_gather_rows, for the A/B test and the
        measurement; uint8 aux frames only, float ones have no former form), and not when the
        caller gives image / goal buffers but no uint8 aux buffers: then the aux frames are
        fresh tensors gathered after the two-frame step, which keeps its output reuse."""
        if not self._aux_fused:
            return False
        if self.aux_format == "u8_hwc":
            if os.environ.get("VN_AUX_OBS_GATHER", "0") not in ("", "0"):
                return False
            if has_out and not has_aux_bufs:
                return False
        return True

    def _aux_frames(self):
        return tuple(torch.empty((self.num_envs,) + s, dtype=self._aux_dtype, device=self.device)
                     for s in self.aux_shapes)

    def _check_five(self, frames):
        """The caller's five frame buffers: each as _check_out wants it, no two overlapping."""
        self._check_frames_out(frames[0], frames[1])
        if any(t is None for t in frames[2:]):
            raise ValueError("out needs all of %s or none of them" % (AUX_KEYS,))
        for name, t, shape in zip(AUX_KEYS, frames[2:], self.aux_shapes):
            self._check_out(name, t, self._aux_dtype, self.num_envs * int(np.prod(shape)))
        spans = sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in frames)
        for (_, end), (start, _) in zip(spans, spans[1:]):
            if start < end:
                raise ValueError("the five frame buffers must not overlap")

    def _obs_set(self, frames):
        return _lib.ObsSet(*[t.data_ptr() for t in frames],
                           _lib.OBS_F32_CHW if self.aux_format == "f32_chw" else _lib.OBS_U8_HWC)

    def _aux_out_frames(self, given):
        """The five frames of a call with caller-owned buffers: `given` holds image, goal and
        either the three aux buffers or None x 3 (fresh aux tensors: the float form only, and
        every such call writes all five, since a fresh tensor may lie at a recorded address)."""
        if all(t is None for t in given[2:]):
            self._check_frames_out(given[0], given[1])
            self._aux_cache = None
            return tuple(given[:2]) + self._aux_frames()
        self._check_five(given)
        return tuple(given)

    def _observe_aux(self, out):
        if out is None:
            self._disarm_reuse()
            frames = self._frames() + self._aux_frames()
        else:
            out = tuple(out)
            if len(out) not in (2, 5):
                raise ValueError("observe(out=...) takes (image, goal) or the five frame buffers")
            frames = self._aux_out_frames(out + (None,) * (5 - len(out)))
            self._arm_reuse()
        o = self._obs_set(frames)
        _lib.check(self.lib.vn_observe_aux(self._ctx, ctypes.byref(o), None, self._stream()), "vn_observe_aux")
        return frames

    def _step_aux(self, a, out):
        E = self.num_envs
        if out is not None:
            bufs = (out["image"], out["goal"], out.get("reward"), out.get("done"), out.get("state")) + \
                tuple(out.get(k) for k in AUX_KEYS)
            c = self._aux_cache
            if c is not None and all(x is y for x, y in zip(bufs, c[0])) and \
                    c[2] == tuple((t.data_ptr(), t.numel()) if t is not None else None for t in bufs):
                P = c[1]
                _lib.check(self.lib.vn_step_aux(self._ctx, _lib.ptr(a), c[3], P[2], P[3], P[4], self._stream()),
                           "vn_step_aux")
                info = dict(self._info)
                info["state"] = bufs[4]
                return (bufs[0], bufs[1]) + bufs[5:], bufs[2], bufs[3], info
        if out is None:
            self._disarm_reuse()
            frames = self._frames() + self._aux_frames()
            reward = torch.empty(E, dtype=torch.float32, device=self.device)
            done = torch.empty(E, dtype=torch.bool, device=self.device)
            state = torch.empty(E, dtype=torch.int32, device=self.device)
            o = self._obs_set(frames)
        else:
            reward, done, state = bufs[2:5]
            frames = self._aux_out_frames(bufs[:2] + bufs[5:])
            self._check_out("reward", reward, torch.float32, E)
            self._check_out("done", done, torch.bool, E)
            self._check_out("state", state, torch.int32, E)
            o = self._obs_set(frames)
            if bufs[5] is not None:
                self._aux_cache = (bufs, tuple(_lib.ptr(t) for t in bufs),
                                   tuple((t.data_ptr(), t.numel()) if t is not None else None for t in bufs),
                                   ctypes.byref(o), o)
                self._out_cache = None
            self._arm_reuse()
        _lib.check(self.lib.vn_step_aux(self._ctx, _lib.ptr(a), ctypes.byref(o), _lib.ptr(reward), _lib.ptr(done),
                                        _lib.ptr(state), self._stream()), "vn_step_aux")
        info = {k: v.clone() for k, v in self._info.items()} if out is None else dict(self._info)
        info["state"] = state
        return frames, reward, done, info

    def step_a2c(self, a2c, reward, done, state):
        """The trainer's rollout step (vn_step_a2c): the actions are sampled in the step from
        the policy outputs named by ``a2c`` (a prepared _lib.A2CStep whose buffers the caller
        keeps alive), index-only, with the per-step bookkeeping fused. reward / done / state
        are the caller's [E] buffers (checked once by the caller)."""
        _lib.check(self.lib.vn_step_a2c(self._ctx, ctypes.byref(a2c), _lib.ptr(reward), _lib.ptr(done),
                                        _lib.ptr(state), self._stream()), "vn_step_a2c")

    def random_actions(self, step, out=None):
        out = torch.empty(self.num_envs, dtype=torch.int32, device=self.device) if out is None else out
        _lib.check(self.lib.vn_random_actions(self._ctx, _lib.ptr(out), ctypes.c_uint64(int(step)), self._stream()),
                   "vn_random_actions")
        return out

    # -- state / checkpoint ----------------------------------------------------
    def get_state(self):
        buf = torch.empty((len(ST_FIELDS), self.num_envs), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.vn_get_state(self._ctx, _lib.ptr(buf), self._stream()), "vn_get_state")
        return buf

    def set_state(self, buf):
        """Restore get_state()'s [len(ST_FIELDS), num_envs] int32 table (checked before the
        device copy: a table of another env count would be read past or misaligned)."""
        buf = torch.as_tensor(buf)
        if tuple(buf.shape) != (len(ST_FIELDS), self.num_envs):
            raise ValueError("env state must be [%d, %d] (this env), got %s"
                             % (len(ST_FIELDS), self.num_envs, tuple(buf.shape)))
        buf = buf.to(device=self.device, dtype=torch.int32).contiguous()
        _lib.check(self.lib.vn_set_state(self._ctx, _lib.ptr(buf), self._stream()), "vn_set_state")

    def get_episode_returns(self):
        """Running return of every env's unfinished episode ([E] f32, device)."""
        buf = torch.empty(self.num_envs, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.vn_get_episode_returns(self._ctx, _lib.ptr(buf), self._stream()),
                   "vn_get_episode_returns")
        return buf

    def set_episode_returns(self, buf):
        buf = torch.as_tensor(buf)
        if tuple(buf.shape) != (self.num_envs,):
            raise ValueError("episode returns must be [%d] (this env), got %s" % (self.num_envs, tuple(buf.shape)))
        buf = buf.to(device=self.device, dtype=torch.float32).contiguous()
        _lib.check(self.lib.vn_set_episode_returns(self._ctx, _lib.ptr(buf), self._stream()),
                   "vn_set_episode_returns")

    def frame_arena(self):
        """(arena uint8 tensor view [rows, H, W, C] over the scene cache, row bases per scene)."""
        p, fb, rows = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        _lib.check(self.lib.vn_frame_arena(self._ctx, ctypes.byref(p), ctypes.byref(fb), ctypes.byref(rows)),
                   "vn_frame_arena")
        bases = []
        for k in range(len(self.scenes)):
            b = ctypes.c_int64()
            _lib.check(self.lib.vn_scene_row_base(self._ctx, k, ctypes.byref(b)), "vn_scene_row_base")
            bases.append(b.value)
        return p.value, fb.value, rows.value, bases

    def error_flags(self, clear=True):
        f = ctypes.c_uint32()
        _lib.check(self.lib.vn_error_flags_sync(self._ctx, ctypes.byref(f), int(clear)), "vn_error_flags_sync")
        return f.value

    def close(self):
        if getattr(self, "_ctx", None):
            self.lib.vn_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# gym-style registry mirroring environments.make ids (environments/__init__.py:2,
# environments/gym_ai2thor/__init__.py:45-49, environments/gym_graph/__init__.py:18-27)
REGISTRY = {
    "CachedThor-v0": dict(max_episode_steps=900),
    "AuxiliaryGraph-v0": dict(max_episode_steps=900, aux_observations=True),
    "OrientedGraph-v0": dict(max_episode_steps=900),
}


def make(id, scenes, num_envs, **kwargs):
    if id not in REGISTRY:
        raise KeyError("unknown env id %r (known: %s)" % (id, sorted(REGISTRY)))
    opts = dict(REGISTRY[id])
    opts.update(kwargs)  # obs_format, aux_format, ... pass through
    return VectorEnv(scenes, num_envs, **opts)


class CachedThorEnv:
    """One gym-style env over the same kernel: the single-env surface of
    THORDiscreteCachedEnv (environments/gym_ai2thor/envs/cached.py:10-99) under gym's
    TimeLimit, for callers that drive one env at a time (gym.make + a hand-written loop,
    test-time episodes). ``reset() -> (image, goal)``; ``step(a) -> (obs, reward, done,
    info)`` with no auto-reset: on a terminal step the previous observation is returned
    (cached.py:90-96) and the caller resets, as with the reference. Frames are float64 in
    [0, 1], HWC, as ``_preprocess_frame`` returns (cached.py:62-64): at the scene's own size,
    or with ``image_size=(H, W)`` resized once on the device when the env is built, each value
    then byte / 255 with the byte round(255 x) of the reference's float x. Every call
    synchronises with the device; the batched ``VectorEnv`` is the fast path."""

    def __init__(self, scene, seed=0, device=None, max_episode_steps=900, float_frames=True, nav_info=False,
                 image_size=None):
        self._env = VectorEnv([scene], 1, seed=seed, device=device, max_episode_steps=max_episode_steps,
                              autoreset=False, nav_info=nav_info, image_size=image_size)
        self.float_frames = bool(float_frames)
        self.action_size = VectorEnv.num_actions  # get_action_size (cached.py:66-68)
        self.max_episode_steps = max_episode_steps

    def _obs(self, img, goal):
        img, goal = img[0].cpu().numpy(), goal[0].cpu().numpy()
        if self.float_frames:
            return img.astype(np.float64) / 255.0, goal.astype(np.float64) / 255.0
        return img, goal

    def reset(self):
        return self._obs(*self._env.reset())

    def step(self, action):
        (img, goal), reward, done, info = self._env.step(torch.tensor([int(action)], dtype=torch.int32))
        info_out = {}
        if bool(info["truncated"][0].item()):
            info_out["TimeLimit.truncated"] = True  # gym's TimeLimit (environments/gym_ai2thor/__init__.py:48)
        for k, _ in NAV_KEYS:  # nav_info=True: the navigation keys as Python scalars
            if k in info:
                info_out[k] = info[k][0].item()
        return self._obs(img, goal), float(reward[0].item()), bool(done[0].item()), info_out

    @property
    def state(self):
        """(state, goal) indices of the env (cached.py: self.state, self.goal)."""
        st = self._env.get_state().cpu().numpy()
        return int(st[ST_FIELDS.index("state"), 0]), int(st[ST_FIELDS.index("goal"), 0])

    def set_schedule(self, starts_goals):
        """Exact replay: the (start, goal) pairs the following resets take, in order."""
        self._env.set_schedule(np.asarray(starts_goals, dtype=np.int32)[None])

    def set_complexity(self, complexity=None):
        self._env.set_complexity(complexity)

    def close(self):
        self._env.close()
