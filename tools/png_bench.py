"""The device PNG writer (csrc/png.hip, elvis_amd/png.py) on a 30-frame 1080p clip of restored content, or of masks.

    python tools/png_bench.py [--frames 30] [--reps 20] [--clip restored_frames.npy] [--out DIR]
                              [--deflate literal|rle] [--content synth|mask]

`--deflate` picks the stream of every device measurement: "literal" (the default) or "rle" (runs of equal filtered bytes
as distance-1 matches).  `--content mask` replaces the clip by gray 0 / 255 masks [n,1080,1920,1] with one rectangle that
moves from frame to frame: what the v1 drivers write as full-resolution hole masks.

The clip is `--clip` where that file holds whole uint8-valued frames [n,H,W,3] (what `bench.py --dump-outputs` writes
for a clip of at most 8 Mi elements; a larger clip is dumped as a sample and cannot be used), else `synth.synth_clip`.
Prints one JSON line per measurement:

  phases      device time between events on the stream, median of `reps` after a warm-up: phase 1 (`elvis_png_stats`)
              and phase 2 (`elvis_png_pack`: pack and CRC kernels) apart, with their algorithmic bytes - the clip read
              once by each phase, the files written once by phase 2 - as a fraction of the HBM peak
  writers     host to host on the same frames and the same disk: `png.save_frames` (upload, encode, download, write)
              against the `frameio.save_frame` loop it stands in for; frames per second of both and their ratio
  sizes       bytes per frame of the device files against PIL at compress_level 6 (its default) and 1
"""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elvis_amd import frameio, png, synth  # noqa: E402
from elvis_amd._lib import check, lib, ptr  # noqa: E402
from elvis_amd.ops import _s  # noqa: E402

HBM_PEAK_GBS = 8000.0


def device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def report(**kw):
    print(json.dumps(kw), flush=True)


def mask_clip(frames, h=1080, w=1920):
    a = np.zeros((frames, h, w, 1), dtype=np.uint8)
    for f in range(frames):
        a[f, h // 4 + 4 * f:3 * h // 4 + 4 * f, w // 3 + 8 * f:2 * w // 3 + 8 * f] = 255
    return a, "rectangle masks"


def save_pil(frame, path):
    if frame.shape[2] == 1:
        frameio.save_mask(frame[:, :, 0], path)
    else:
        frameio.save_frame(frame, path)


def load_clip(path, frames):
    if path and os.path.exists(path):
        a = np.load(path)
        if a.ndim == 4 and a.shape[3] == 3:
            return np.ascontiguousarray(a[:frames]).astype(np.uint8), "dumped restored frames"
    return synth.synth_clip(7, frames, 1080, 1920), "synth.synth_clip"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--clip", default=None)
    ap.add_argument("--out", default=None, help="directory for the written files (default: a temporary one)")
    ap.add_argument("--segment-rows", type=int, default=16)
    ap.add_argument("--deflate", choices=png.DEFLATES, default="literal")
    ap.add_argument("--content", choices=("synth", "mask"), default="synth")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    clip, source = mask_clip(args.frames) if args.content == "mask" else load_clip(args.clip, args.frames)
    rle = args.deflate == "rle"
    stride = png.RLE_STATS_STRIDE if rle else png.STATS_STRIDE
    stats_fn, pack_fn = (lib().elvis_png_stats_rle, lib().elvis_png_pack_rle) if rle else (lib().elvis_png_stats, lib().elvis_png_pack)
    plan_fn = png.plan_layout_rle if rle else png.plan_layout
    n, h, w, c = clip.shape
    rows = args.segment_rows
    nseg = (h + rows - 1) // rows
    d = torch.from_numpy(clip).to(dev)

    # the two phases apart, on the resident clip
    types = torch.empty(n * h, dtype=torch.uint8, device=dev)
    stats_d = torch.empty(n * nseg * stride, dtype=torch.int32, device=dev)

    def phase1():
        check(stats_fn(ptr(d), ptr(types), ptr(stats_d), n, h, w, c, 1, -1, rows, _s(d)), dev)
    phase1()
    t0 = time.perf_counter()
    plan = plan_fn(stats_d.cpu().numpy().view(np.uint32).reshape(n, nseg, stride))
    plan_ms = (time.perf_counter() - t0) * 1e3
    total = int(plan.file_offsets[-1])
    chunks_d = torch.from_numpy(plan.chunks).to(dev)
    tab_d = torch.from_numpy(plan.frame_tab.view(np.int32)).to(dev)
    out = torch.empty(total, dtype=torch.uint8, device=dev)

    def phase2():
        check(pack_fn(ptr(d), ptr(types), ptr(chunks_d), ptr(tab_d), ptr(out), total, n, h, w, c, 1, rows, _s(d)), dev)
    t1, t2 = device_ms(phase1, args.reps), device_ms(phase2, args.reps)
    raw = clip.size
    report(what="phases", source=source, deflate=args.deflate, file_bytes=total, frames=n, shape=[h, w, c], segment_rows=rows, phase1_ms=round(t1, 3), phase2_ms=round(t2, 3),
           download_and_plan_ms=round(plan_ms, 3), device_ms_per_frame=round((t1 + t2) / n, 4),
           phase1_hbm_fraction=round(raw / (t1 * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
           phase2_hbm_fraction=round((raw + total) / (t2 * 1e-3) / 1e9 / HBM_PEAK_GBS, 4))
    del out, chunks_d, tab_d, stats_d, types

    # host to host, same frames, same disk
    frames = [np.ascontiguousarray(f) for f in clip]
    with tempfile.TemporaryDirectory(dir=args.out) as root:
        dev_paths = [os.path.join(root, "device", f"{i + 1:05d}.png") for i in range(n)]
        pil_paths = [os.path.join(root, "pil", f"{i + 1:05d}.png") for i in range(n)]
        png.save_frames(frames[:2], dev_paths[:2], dev, deflate=args.deflate)   # warm-up
        t0 = time.perf_counter()
        png.save_frames(frames, dev_paths, dev, deflate=args.deflate)
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        for f, p in zip(frames, pil_paths):
            save_pil(f, p)
        t_pil = time.perf_counter() - t0
        for f, p in zip(frames[:3], dev_paths[:3]):
            with Image.open(p) as im:
                back = np.asarray(im)
            assert np.array_equal(back.reshape(h, w, -1)[:, :, ::-1], f), "the device file does not decode to the frame"
        report(what="writers", frames=n, device_fps=round(n / t_dev, 2), pil_fps=round(n / t_pil, 2), ratio=round(t_pil / t_dev, 2),
               device_ms_per_frame=round(t_dev / n * 1e3, 2), pil_ms_per_frame=round(t_pil / n * 1e3, 2))
        size_dev = sum(os.path.getsize(p) for p in dev_paths) / n
        size_pil6 = sum(os.path.getsize(p) for p in pil_paths) / n

    sample = frames[:min(n, 5)]
    size1 = 0
    for f in sample:
        buf = io.BytesIO()
        (Image.fromarray(f[:, :, 0], "L") if c == 1 else Image.fromarray(np.ascontiguousarray(f[:, :, ::-1]), "RGB")).save(
            buf, format="PNG", compress_level=1)
        size1 += buf.tell()
    report(what="sizes", deflate=args.deflate, raw_bytes_per_frame=h * w * c, device_bytes_per_frame=round(size_dev), pil_level6_bytes_per_frame=round(size_pil6),
           pil_level1_bytes_per_frame=round(size1 / len(sample)), device_over_level6=round(size_dev / size_pil6, 4),
           device_over_level1=round(size_dev / (size1 / len(sample)), 4))


if __name__ == "__main__":
    main()
