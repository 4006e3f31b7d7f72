"""Time of the encoder hand-off on a 30-frame 1080p clip, with the host conversion it replaces as context.

    python tools/handoff_bench.py [--frames 30] [--repeats 20] [--cpu-frames 2] [--out FILE]

`rgb_to_i420_device` on a resident clip: device events around the call, median and minimum over the repeats after
warm-up; `hbm_fraction` is the kernel's traffic - 6.22 MB of RGB read and 3.11 MB of I420 written per 1080p frame,
9.33 MB - over the device-event median, as a fraction of the 8 TB/s HBM peak.  `convert_frames_to_yuv420p` host to host
(upload, launches, read-back in chunks, the bytes object) against what a caller does without it: download the resident
RGB clip and convert it on this host with the numpy restatement (tests/_handoff_ref.py, timed on `--cpu-frames` frames
and scaled to the clip; the download is timed on the whole clip).  One JSON line per measurement.
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

from elvis_amd import handoff, synth  # noqa: E402
from elvis_amd.recompose import frames_to_device  # noqa: E402
import _handoff_ref as R  # noqa: E402

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
        raise SystemExit("handoff_bench needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    h, w, n = 1080, 1920, args.frames
    frames = list(synth.synth_clip(21, n, h, w))
    lines = []

    def report(name, kind, med_min, count, **extra):
        line = dict(call=name, clock=kind, frames=count, ms_median=round(med_min[0], 4), ms_min=round(med_min[1], 4),
                    ms_per_frame=round(med_min[0] / count, 4), **extra)
        lines.append(line)
        print(json.dumps(line), flush=True)

    clip = frames_to_device(frames, dev)
    out = torch.empty((n, h * 3 // 2, w), dtype=torch.uint8, device=dev)
    traffic = clip.numel() + out.numel()
    for order in ("rgb", "bgr"):
        t = device_ms(lambda: handoff.rgb_to_i420_device(clip, order, out=out), args.repeats)
        report(f"rgb_to_i420_device ({order})", "device events", t, n, bytes_per_frame=traffic // n,
               tb_per_s=round(traffic / (t[0] * 1e-3) / 1e12, 3), hbm_fraction=round(traffic / (t[0] * 1e-3) / HBM_PEAK, 4))
    few = max(2, args.repeats // 4)
    report("convert_frames_to_yuv420p", "host to host", host_ms(lambda: handoff.convert_frames_to_yuv420p(frames, dev), few), n)
    report("download of the I420 clip", "host to host", host_ms(lambda: out.cpu(), few), n)
    download = host_ms(lambda: clip.cpu(), few)
    report("download of the RGB clip", "host to host", download, n)
    k = max(1, min(args.cpu_frames, n))
    t0 = time.perf_counter()
    R.yuv420p_bytes(frames[:k])
    cpu = (time.perf_counter() - t0) * 1e3 / k
    report("_handoff_ref.yuv420p_bytes", "cpu", (cpu * k,) * 2, k)
    report("download of the RGB clip + _handoff_ref on the host", "host to host (cpu part scaled)", (download[0] + cpu * n,) * 2, n)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=lines), f, indent=1)


if __name__ == "__main__":
    main()
