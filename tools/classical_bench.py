"""Classical restorers (elvis_amd/classical.py) at 1080p: 30 frames, block 8, levels spread over 0-4.

    python tools/classical_bench.py [--frames 30] [--reps 10] [--out FILE]

For the Lanczos restorer, the unsharp mask at halo 0 and at halo 8, and the temporal blend, prints:
  * device-resident frames/s: one launch over the clip already in HBM, HIP events, after a warm-up;
  * host-to-host frames/s: pinned host clip -> device -> restorer -> pinned host clip, synchronised;
  * the numpy restatement (tests/_classical_ref.py) on one frame, in seconds - context next to BASELINE.md's
    CPU OpenCV numbers (6.08 / 5.27 frames/s at 720p), not a like-for-like comparison.
One JSON line with every number closes the output (and goes to --out when given).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from elvis_amd import classical, synth  # noqa: E402


def _levels(n, by, bx, seed=3):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 5, size=(n, by, bx)).astype(np.int32)    # levels 0..4, uniform


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("classical_bench needs a GPU")
    dev = torch.device("cuda:0")
    n, h, w, b = args.frames, 1080, 1920, 8
    clip = synth.synth_clip(11, n, h, w)
    lv = _levels(n, h // b, w // b)
    fd = torch.from_numpy(clip).to(dev)
    ld = torch.from_numpy(lv).to(dev)
    out_d = torch.empty_like(fd)
    pin_in = torch.from_numpy(clip).pin_memory()
    pin_out = torch.empty_like(pin_in).pin_memory()

    cases = {
        "lanczos": lambda src, maps, out: classical.lanczos_restore_device(src, maps, b, out=out),
        "unsharp_halo0": lambda src, maps, out: classical.unsharp_restore_device(src, maps, b, halo=0, out=out),
        "unsharp_halo8": lambda src, maps, out: classical.unsharp_restore_device(src, maps, b, halo=8, out=out),
        "temporal_blend": lambda src, maps, out: classical.temporal_blend_device(src, 0.1, out=out),
    }
    result = {"frames": n, "height": h, "width": w, "block": b, "levels": "0-4 uniform"}
    for name, fn in cases.items():
        for _ in range(3):
            fn(fd, ld, out_d)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn(fd, ld, out_d)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.reps
        # host to host: pinned upload, one launch, pinned download, synchronised
        t0 = time.perf_counter()
        for _ in range(args.reps):
            src = pin_in.to(dev, non_blocking=True)
            maps = ld if name != "temporal_blend" else None
            res = fn(src, maps, None if name == "temporal_blend" else torch.empty_like(src))
            pin_out.copy_(res, non_blocking=True)
            torch.cuda.synchronize()
        h2h = (time.perf_counter() - t0) / args.reps
        result[name] = {"device_ms_per_clip": round(ms, 3), "device_us_per_frame": round(ms * 1e3 / n, 1),
                        "device_fps": round(n / (ms / 1e3), 1), "host_to_host_fps": round(n / h2h, 1)}
        print(f"{name:15s} device {ms * 1e3 / n:8.1f} us/frame = {n / (ms / 1e3):9.1f} frames/s   "
              f"host to host {n / h2h:7.1f} frames/s")
    assert np.array_equal(pin_out.numpy()[0], clip[0])     # the blend leaves frame 0 as it is

    import _classical_ref as R
    f0, l0 = clip[:1], lv[:1]
    for name, fn in (("lanczos", lambda: R.lanczos_restore(f0, l0, b)),
                     ("unsharp_halo0", lambda: R.unsharp_restore(f0, l0, b, 0)),
                     ("unsharp_halo8", lambda: R.unsharp_restore(f0, l0, b, 8))):
        t0 = time.perf_counter()
        fn()
        result[name]["numpy_restatement_s_per_frame"] = round(time.perf_counter() - t0, 3)
        print(f"{name:15s} numpy restatement {result[name]['numpy_restatement_s_per_frame']:.3f} s per 1080p frame")
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
