"""bench.py's plain run: only the headline figure (no CPU baseline, PMC pass or training leg
unless --full), and --dump-outputs writes what the last timed VectorEnv.step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (7, 3)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    """One plain run at 300 envs (more than the 256 whose frames are kept), 2 scenes, 2 warmup
    + 3 timed steps: the line has the headline keys and none of --full's parts; the dumped
    arrays are float32 / float64 and equal, value for value, what a VectorEnv built and
    stepped the same way returns from its fifth step."""
    import torch
    import vnav
    import bench
    E, W, K = 300, 2, 3
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
           "--envs", str(E), "--scenes", "2", "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-4000:]
    line = json.loads(lines[0])
    assert line["steps"] == K and line["warmup"] == W and line["unit"] == "env-steps/s" and line["dtype"] == "u8"
    assert line["higher_is_better"] is True and line["error_flags"] == 0
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(E * 1e3 / line["ms_per_step"], rel=1e-9)
    assert line["cpu_baseline"] is None and line["roofline"]["traffic"] is None
    assert not [k for k in line if k.startswith("train") and line[k] is not None]

    dev = torch.device("cuda", 0)
    ve = vnav.VectorEnv([vnav.synthetic_scene(k) for k in range(2)], E, seed=1000, device=dev)
    for t in range(W + K):
        (img, goal), reward, done, info = ve.step(ve.random_actions(t))
    pick = np.load(dump / "sample_envs.npy").astype(np.int64)
    assert len(pick) == bench.DUMP_SAMPLE_ENVS and np.all(np.diff(pick) > 0) and 0 <= pick[0] and pick[-1] < E
    want = {"image": img.cpu().numpy()[pick], "goal": goal.cpu().numpy()[pick], "reward": reward.cpu().numpy(),
            "done": done.cpu().numpy(), **{k: v.cpu().numpy() for k, v in info.items()}}
    got = {p.stem: np.load(p) for p in dump.glob("*.npy")}
    assert set(got) == set(want) | {"sample_envs"}
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    for k, v in want.items():
        assert got[k].dtype in (np.float32, np.float64), k
        assert got[k].shape == v.shape and np.array_equal(got[k], v.astype(got[k].dtype)), k
    assert got["image"].std() > 0 and not np.array_equal(got["image"], got["goal"])
