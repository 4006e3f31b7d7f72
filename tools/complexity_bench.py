"""Time of the block-complexity analysis on a 30-frame 1080p clip, with its numpy statement on this host as context.

    python tools/complexity_bench.py [--frames 30] [--repeats 20] [--cpu-frames 2] [--out FILE]

`block_complexity_device` on a resident RGB clip at block 8 and 16: device events around the call, median and minimum
over the repeats after warm-up; `hbm_fraction` is the bytes the kernel reads - the whole blocks of every frame once,
6.2 MB per 1080p RGB frame; the two float64 maps it writes are 0.5 MB (block 8) or 0.13 MB (block 16) per frame and
are counted too - over the device-event median, as a fraction of the 8 TB/s HBM peak.  `analyze_frames` host to host
(upload in chunks, launches, the two maps read back) beside tests/_complexity_ref.py on the same host (timed on
`--cpu-frames` frames and scaled to the clip): context, not a target.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from elvis_amd import complexity, synth  # noqa: E402
from elvis_amd.recompose import frames_to_device  # noqa: E402
import _complexity_ref as R  # noqa: E402

HBM_PEAK = 8.0e12


def device_ms(call, repeats: int, warmup: int = 2):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    t = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        stop.record()
        stop.synchronize()
        t.append(start.elapsed_time(stop))
    return float(np.median(t)), float(np.min(t))


def host_ms(call, repeats: int, warmup: int = 1):
    for _ in range(warmup):
        call()
    t = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--cpu-frames", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("complexity_bench needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    h, w, n = 1080, 1920, args.frames
    frames = list(synth.synth_clip(21, n, h, w))
    host_clip = np.stack(frames)
    lines = []

    def report(name, kind, med_min, count, **extra):
        line = dict(call=name, clock=kind, frames=count, ms_median=round(med_min[0], 4), ms_min=round(med_min[1], 4),
                    ms_per_frame=round(med_min[0] / count, 4), **extra)
        lines.append(line)
        print(json.dumps(line), flush=True)

    clip = frames_to_device(frames, dev)
    few = max(2, args.repeats // 4)
    k = max(2, min(args.cpu_frames, n))
    for block in (8, 16):
        by, bx = h // block, w // block
        out = tuple(torch.empty((n, by, bx), dtype=torch.float64, device=dev) for _ in range(2))
        traffic = n * by * block * bx * block * 3 + 2 * out[0].numel() * 8
        t = device_ms(lambda: complexity.block_complexity_device(clip, block, "rgb", out=out), args.repeats)
        report(f"block_complexity_device (block {block})", "device events", t, n, bytes_per_frame=traffic // n,
               tb_per_s=round(traffic / (t[0] * 1e-3) / 1e12, 3), hbm_fraction=round(traffic / (t[0] * 1e-3) / HBM_PEAK, 4))
        cfg = complexity.EVCAConfig(block_size=block)
        report(f"analyze_frames (block {block})", "host to host", host_ms(lambda: complexity.analyze_frames(host_clip, cfg, dev), few), n)
        t0 = time.perf_counter()
        R.complexity(host_clip[:k], block, "rgb")
        cpu = (time.perf_counter() - t0) * 1e3
        report(f"_complexity_ref.complexity (block {block})", "cpu", (cpu,) * 2, k)
        report(f"_complexity_ref.complexity (block {block}), scaled to the clip", "cpu (scaled)", (cpu / k * n,) * 2, n)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=lines), f, indent=1)


if __name__ == "__main__":
    main()
