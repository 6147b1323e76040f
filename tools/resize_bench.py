"""Measure vn_resize_frames against the upload of its own input (DESIGN.md "Scene ingest:
resize on the device").

    python tools/resize_bench.py [--frames 1000] [--rounds 5] [--out bench_out/resize_bench.json]

One process, two shapes (300x400x3 -> 84x84 and 300x300x3 -> 174x174, the cached-THOR dump
sizes and the policies' inputs). Per shape, on --frames frames resident on the device:
  device_ms          one vn_resize_frames call between one event pair, --rounds rounds after a
                     warm-up: min / median / max
  upload_ms          the same frames host -> device, from pageable memory (what resize_frames
                     does) and from pinned memory, event-timed the same way
  input_gb_s         input bytes over the median device time
  cpu_ref_ms_per_frame   tests/resize_ref.py (numpy) on 20 frames, for scale only
The first two frames are also compared with tests/resize_ref.py bit for bit. Needs a GPU.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "a2cat-vn-pytorch_amd"), os.path.join(REPO, "tests")]

SHAPES = (((300, 400, 3), (84, 84)), ((300, 300, 3), (174, 174)))


def timed(fn, rounds):
    import torch
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return dict(min=min(out), median=statistics.median(out), max=max(out), rounds=out)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--frames", type=int, default=1000)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--cpu-frames", type=int, default=20)
    p.add_argument("--out", default=os.path.join("bench_out", "resize_bench.json"))
    a = p.parse_args(argv)
    import torch

    import resize_ref
    from vnav import _lib, scenes
    if not torch.cuda.is_available():
        raise SystemExit("resize_bench needs a GPU")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    results = []
    for (h, w, c), (oh, ow) in SHAPES:
        n = a.frames
        rng = np.random.default_rng(h * w)
        host = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        pinned = torch.from_numpy(host).pin_memory()
        src = torch.empty((n, h, w, c), dtype=torch.uint8, device=dev)
        dst = torch.empty((n, oh, ow, c), dtype=torch.uint8, device=dev)
        _, rr, tr = scenes.resize_taps(h, oh)
        _, rc, tc = scenes.resize_taps(w, ow)
        dp = ctypes.POINTER(ctypes.c_double)

        def run():
            _lib.check(lib.vn_resize_frames(_lib.ptr(src), n, h, w, c, oh, ow, tr.ctypes.data_as(dp), rr,
                                            tc.ctypes.data_as(dp), rc, _lib.ptr(dst), _lib.stream_ptr(dev)),
                       "vn_resize_frames")

        src.copy_(pinned)
        run()  # warm-up: loads the code object
        torch.cuda.synchronize()
        dev_ms = timed(run, a.rounds)
        up_pageable = timed(lambda: src.copy_(torch.from_numpy(host)), a.rounds)
        up_pinned = timed(lambda: src.copy_(pinned, non_blocking=True), a.rounds)
        torch.cuda.synchronize()
        got = dst[:2].cpu().numpy()
        exact = bool(np.array_equal(got, resize_ref.resize(host[:2], (oh, ow))))
        k = min(a.cpu_frames, n)
        t0 = time.perf_counter()
        resize_ref.resize(host[:k], (oh, ow))
        cpu_ms = (time.perf_counter() - t0) * 1e3 / k
        in_bytes = host.nbytes
        results.append(dict(shape=[h, w, c], image_size=[oh, ow], frames=n, input_bytes=in_bytes, radius=[rr, rc],
                            device_ms=dev_ms, upload_ms_pageable=up_pageable, upload_ms_pinned=up_pinned,
                            input_gb_s=in_bytes / dev_ms["median"] / 1e6,
                            resize_over_pinned_upload=dev_ms["median"] / up_pinned["median"],
                            bitwise_equal_to_resize_ref=exact, cpu_ref_ms_per_frame=cpu_ms, cpu_ref_frames=k))
        print(json.dumps(results[-1]))
        del src, dst, pinned, host
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), results=results), f, indent=1)
    return 0 if all(r["bitwise_equal_to_resize_ref"] for r in results) else 1


if __name__ == "__main__":
    raise SystemExit(main())
