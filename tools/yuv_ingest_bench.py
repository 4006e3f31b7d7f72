"""Time of the decoder hand-off on the seeded 30-frame 1080p `synth` clip, against the PNG paths it stands beside.

    python tools/yuv_ingest_bench.py [--frames 30] [--repeats 10] [--e2e-repeats 3] [--out FILE]

Every pair runs in this one process, arms alternating, after a warm-up of each arm; a time is the median (and minimum)
over the repeats of a host clock around a call that ends in a device synchronise, except the kernel's, which is device
events around `i420_to_rgb_device` on a resident clip.  `hbm_fraction` is the kernel's traffic - 1.5 bytes read and 3
written per pixel, 4.5 - over the device-event median, as a fraction of the 8 TB/s HBM peak.

  in    A  `frameio.load_frame` over a directory of PNGs, then `frames_to_device`   (what every client entry point does)
        B  `handoff.load_y4m_device` of the same pixels as one .y4m file
  out   A  `frameio.save_frame` per frame into a directory
        B  `handoff.write_y4m`
  e2e   A  `drivers.restore_blur_adaptive` on a PNG directory (rewritten before every repeat, outside the clock)
        B  `drivers.restore_yuv_clip("blur")` from a .y4m to a .y4m
        one blur round on every block, `--e2e-repeats` repeats: the model dominates both arms

The pixels of the B arms are the A arms' after one trip through I420 (the .y4m is written from the PNG frames), so
the two arms do not hold the same bytes - 4:2:0 is lossy - but the same picture at the same size.  One JSON line per
measurement.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elvis_amd import drivers, frameio, handoff, synth  # noqa: E402
from elvis_amd.recompose import frames_to_device  # noqa: E402

HBM_PEAK = 8.0e12


def device_ms(call, repeats: int, warmup: int = 3):
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


def alternate_ms(arms, repeats: int, before=None):
    """Median and minimum host time of each arm, the arms taking turns; `before[i]` runs outside the clock."""
    before = before or [None] * len(arms)
    for prep, arm in zip(before, arms):                      # warm-up: code objects, the page cache, pinned pools
        if prep:
            prep()
        arm()
    times = [[] for _ in arms]
    for _ in range(repeats):
        for i, arm in enumerate(arms):
            if before[i]:
                before[i]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arm()
            torch.cuda.synchronize()
            times[i].append((time.perf_counter() - t0) * 1e3)
    return [(float(np.median(t)), float(np.min(t))) for t in times]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--e2e-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("yuv_ingest_bench needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    h, w, n = args.height, args.width, args.frames
    frames = list(synth.synth_clip(21, n, h, w))
    lines = []

    def report(name, clock, med_min, **extra):
        line = dict(call=name, clock=clock, frames=n, ms_median=round(med_min[0], 4), ms_min=round(med_min[1], 4),
                    ms_per_frame=round(med_min[0] / n, 4), **extra)
        lines.append(line)
        print(json.dumps(line), flush=True)

    def pair(name, a, b, results):
        report(f"{name} A: {a}", "host, synchronised", results[0])
        report(f"{name} B: {b}", "host, synchronised", results[1], a_over_b=round(results[0][0] / results[1][0], 3))

    with tempfile.TemporaryDirectory(prefix="yuv_ingest_") as d:
        png_dir, out_dir = os.path.join(d, "png"), os.path.join(d, "png_out")
        os.makedirs(png_dir)
        os.makedirs(out_dir)
        names = [f"{i + 1:05d}.png" for i in range(n)]

        def write_pngs():
            for name, f in zip(names, frames):
                frameio.save_frame(f, os.path.join(png_dir, name))

        write_pngs()
        y4m, y4m_out = os.path.join(d, "clip.y4m"), os.path.join(d, "out.y4m")
        handoff.write_y4m(frames, y4m, 30.0, dev)

        # the kernel alone
        planes = handoff.rgb_to_i420_device(frames_to_device(frames, dev))
        clip = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
        traffic = planes.numel() + clip.numel()
        for order in ("rgb", "bgr"):
            t = device_ms(lambda: handoff.i420_to_rgb_device(planes, order, out=clip), max(args.repeats, 20))
            report(f"i420_to_rgb_device ({order})", "device events", t, bytes_per_pixel=traffic / (n * h * w),
                   tb_per_s=round(traffic / (t[0] * 1e-3) / 1e12, 3), hbm_fraction=round(traffic / (t[0] * 1e-3) / HBM_PEAK, 4))
        del planes, clip

        # the way in
        results = alternate_ms([lambda: frames_to_device([frameio.load_frame(os.path.join(png_dir, name)) for name in names], dev),
                                lambda: handoff.load_y4m_device(y4m, dev)], args.repeats)
        pair("in", "load_frame x n + frames_to_device", "load_y4m_device", results)

        # the way out
        def save_pngs():
            for name, f in zip(names, frames):
                frameio.save_frame(f, os.path.join(out_dir, name))

        results = alternate_ms([save_pngs, lambda: handoff.write_y4m(frames, y4m_out, 30.0, dev)], args.repeats)
        pair("out", "save_frame x n", "write_y4m", results)

        # end to end, the Blur slot
        b = 8
        rounds = np.ones((n, h // b, w // b), np.int32)
        results = alternate_ms([lambda: drivers.restore_blur_adaptive(png_dir, rounds, b, devices=[dev]),
                                lambda: drivers.restore_yuv_clip("blur", y4m, y4m_out, rounds, b, devices=[dev])],
                               args.e2e_repeats, before=[write_pngs, None])
        pair("e2e blur", "restore_blur_adaptive on a PNG directory", "restore_yuv_clip .y4m -> .y4m", results)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=lines), f, indent=1)


if __name__ == "__main__":
    main()
