"""Time of the on-device quality report on a 30-frame 1080p clip, with the numpy / scipy restatement as context.

    python tools/quality_bench.py [--frames 30] [--repeats 10] [--cpu-frames 2] [--out FILE]

Per call - `masked_ssim_device` (bounding boxes + luma SSIM of the whole clip, resident tensors), `calculate_ssim` and
`evaluate_fg_bg_metrics` (host numpy in, host numbers out): device events around the call where it runs on resident
tensors, and host-to-host wall time (upload, launches, read-back) for the public functions; median and minimum over
the repeats after warm-up, one JSON line per measurement.  `hbm_fraction` is the SSIM kernel's algorithmic traffic -
two frame reads plus the mask - over the device-event median, as a fraction of the 8 TB/s HBM peak.  The CPU lines
time tests/_quality_ref.py (scipy's Gaussian filter) on `--cpu-frames` frames of the same clip on this host.
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

from elvis_amd import metrics, synth  # noqa: E402
from elvis_amd.recompose import frames_to_device  # noqa: E402
import _quality_ref as Q  # noqa: E402

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
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--cpu-frames", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quality_bench needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    h, w, n = 1080, 1920, args.frames
    refs = list(synth.synth_clip(11, n, h, w))
    rng = np.random.default_rng(12)
    decs = [np.clip(f.astype(np.int16) + rng.integers(-8, 9, f.shape), 0, 255).astype(np.uint8) for f in refs]
    yy, xx = np.mgrid[:h, :w]
    fg = [((yy - 500 - 3 * i) ** 2 + (xx - 800 - 8 * i) ** 2) < 300 ** 2 for i in range(n)]
    lines = []

    def report(name, kind, med_min, frames, **extra):
        line = dict(call=name, clock=kind, frames=frames, ms_median=round(med_min[0], 4), ms_min=round(med_min[1], 4),
                    ms_per_frame=round(med_min[0] / frames, 4), **extra)
        lines.append(line)
        print(json.dumps(line), flush=True)

    a, b = frames_to_device(refs, dev), frames_to_device(decs, dev)
    m = metrics.masks_to_device(fg, (h, w), dev)
    algorithmic = 2 * a.numel() + m.numel()
    t = device_ms(lambda: metrics.masked_ssim_device(a, b, m), args.repeats)
    report("masked_ssim_device (foreground boxes)", "device events", t, n, hbm_fraction=round(algorithmic / (t[0] * 1e-3) / HBM_PEAK, 4))
    t = device_ms(lambda: metrics.masked_ssim_device(a, b, None), args.repeats)
    report("masked_ssim_device (whole frames)", "device events", t, n, hbm_fraction=round(2 * a.numel() / (t[0] * 1e-3) / HBM_PEAK, 4))
    t = device_ms(lambda: metrics.calculate_ssim_device(a, b), args.repeats)
    report("calculate_ssim_device", "device events", t, n, hbm_fraction=round(2 * a.numel() / (t[0] * 1e-3) / HBM_PEAK, 4))
    report("masked_ssim_device (foreground boxes)", "host to host", host_ms(lambda: metrics.masked_ssim_device(a, b, m).cpu(), args.repeats), n)
    report("calculate_ssim", "host to host", host_ms(lambda: metrics.calculate_ssim(refs, decs, device=dev), max(2, args.repeats // 3)), n)
    report("evaluate_fg_bg_metrics", "host to host", host_ms(lambda: metrics.evaluate_fg_bg_metrics(refs, decs, fg, 1, dev), max(2, args.repeats // 3)), n)

    k = max(1, min(args.cpu_frames, n))
    t0 = time.perf_counter()
    for i in range(k):
        Q.masked_ssim(refs[i], decs[i], fg[i])
        Q.masked_ssim(refs[i], decs[i], ~fg[i])
    report("_quality_ref.masked_ssim (foreground + background)", "cpu", ((time.perf_counter() - t0) * 1e3,) * 2, k)
    t0 = time.perf_counter()
    for i in range(k):
        Q.msssim_ssim(refs[i], decs[i])
    report("_quality_ref.msssim_ssim", "cpu", ((time.perf_counter() - t0) * 1e3,) * 2, k)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=lines), f, indent=1)


if __name__ == "__main__":
    main()
