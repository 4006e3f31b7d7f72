"""JPEG reading: files on disk to a resident [n,1080,1920,3] clip through the device reader
(jpeg.load_jpeg_frames_device) against the PIL path (frameio.load_frame per file, then recompose.frames_to_device), on
one seeded synthetic clip written by PIL at quality 90, 4:2:0, once without restart markers (a file is one serial
segment: one lane) and once with `restart_marker_rows=1` (a segment per MCU row).

    python tools/jpeg_read_bench.py [--frames 30] [--height 1080] [--width 1920] [--runs 10] [--out DIR]

Both paths run in the same call, alternating, after a warm-up; the host clock is read around a final synchronise and the
median is reported.  In the same run device events are taken around each of the three C-ABI calls, and the statement
(tests/_jpeg_ref.py) counts one frame's Huffman symbols for the entropy kernel's rate.  `--kernels-only` runs just the
device path a few times, for a `rocprofv3 --kernel-trace --stats` run of its own.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from elvis_amd import frameio, jpeg, synth  # noqa: E402
from elvis_amd.recompose import frames_to_device  # noqa: E402


def _time(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def _kernel_events(paths, dev):
    """Device events around each C-ABI call of one decode of the whole clip: ms for tables + entropy, IDCT, colour."""
    from elvis_amd import _lib
    files = [open(p, "rb").read() for p in paths]
    infos = [jpeg.parse_jpeg(d, p) for d, p in zip(files, paths)]
    out = torch.empty((len(files), infos[0].height, infos[0].width, 3), dtype=torch.uint8, device=dev)
    handle = _lib.lib()
    names = ("elvis_jpeg_entropy", "elvis_jpeg_idct", "elvis_jpeg_colour")
    marks = []

    class Timed:
        def __getattr__(self, name):
            fn = getattr(handle, name)
            if name not in names:
                return fn

            def call(*args):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                rc = fn(*args)
                b.record()
                marks.append((name, a, b))
                return rc
            return call

    real = jpeg.lib
    jpeg.lib = lambda: Timed()
    try:
        jpeg._launch_decode(files, infos, out, "bgr", 3)
    finally:
        jpeg.lib = real
    torch.cuda.synchronize(dev)
    ms = {}
    for name, a, b in marks:
        ms[name] = ms.get(name, 0.0) + a.elapsed_time(b)
    return ms, files, infos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--no-symbols", action="store_true", help="skip the statement's symbol count (seconds of Python a frame)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    clip = np.ascontiguousarray(synth.synth_clip(7, args.frames, args.height, args.width))
    result = {"frames": args.frames, "height": args.height, "width": args.width, "runs": args.runs}
    with tempfile.TemporaryDirectory(prefix="jpeg_read_bench_") as tmp:
        from PIL import Image
        sets = {}
        for name, save in (("no_restart", {}), ("restart_rows_1", {"restart_marker_rows": 1})):
            d = os.path.join(tmp, name)
            os.makedirs(d)
            sets[name] = [os.path.join(d, f"{i + 1:05d}.jpg") for i in range(args.frames)]
            for p, f in zip(sets[name], clip):
                Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(p, quality=90, subsampling=2, **save)
        for name, paths in sets.items():
            device_path = lambda: jpeg.load_jpeg_frames_device(paths, dev)                                # noqa: E731
            pil_path = lambda: frames_to_device([frameio.load_frame(p) for p in paths], dev)              # noqa: E731
            assert torch.equal(device_path(), pil_path()), name
            if args.kernels_only:
                for _ in range(3):
                    device_path()
                torch.cuda.synchronize(dev)
                continue
            for _ in range(args.warmup):
                _time(device_path, dev)
            _time(pil_path, dev)
            dev_ms, pil_ms = [], []
            for _ in range(args.runs):
                dev_ms.append(_time(device_path, dev))
                pil_ms.append(_time(pil_path, dev))
            events, files, infos = _kernel_events(paths, dev)
            entry = {
                "file_bytes_mean": int(np.mean([os.path.getsize(p) for p in paths])),
                "segments_per_frame": len(infos[0].segments),
                "device_ms_median": round(statistics.median(dev_ms), 2), "pil_ms_median": round(statistics.median(pil_ms), 2),
                "pil_over_device": round(statistics.median(pil_ms) / statistics.median(dev_ms), 3),
                "kernel_ms": {k: round(v, 3) for k, v in events.items()},
            }
            if not args.no_symbols:
                import _jpeg_ref as R
                nsym = [0]
                R.entropy_decode(R.walk(files[0]), symbols=nsym)
                lanes = len(infos[0].segments)
                entry["symbols_frame0"] = nsym[0]
                # the frames run side by side and so do a frame's segments, a lane each: the call lasts as long as the
                # slowest lane, which decodes about a frame's symbols over its segments
                entry["symbols_per_second_per_lane"] = round(nsym[0] / lanes / (events["elvis_jpeg_entropy"] * 1e-3))
                entry["symbols_per_second_clip"] = round(nsym[0] * args.frames / (events["elvis_jpeg_entropy"] * 1e-3))
            result[name] = entry
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "jpeg_read_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
