"""PNG reading: files on disk to a resident [n,1080,1920,3] clip through the device reader (png.load_frames_device) against
the PIL path (frameio.load_frame per file, then recompose.frames_to_device), on one seeded synthetic clip written once by
PIL at compress_level 6 and once by the device writer.

    python tools/png_read_bench.py [--frames 30] [--height 1080] [--width 1920] [--runs 10] [--out DIR]

Both paths run in the same call, alternating, after a warm-up; the host clock is read around a final synchronise and the
median is reported.  In the same run device events are taken around each of the three C-ABI calls, and the statement
(tests/_png_read_ref.py) counts one frame's tokens for the inflater's serial rate.  `--kernels-only` runs just the device
path a few times, for a `rocprofv3 --kernel-trace --stats` run of its own.  Prints one JSON line.
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

from elvis_amd import frameio, png, synth  # noqa: E402
from elvis_amd.recompose import frames_to_device  # noqa: E402


def _clip(n, h, w, seed=7):
    """The seeded synthetic clip of synth.py: a smooth field panning over time, gratings and sensor noise."""
    return np.ascontiguousarray(synth.synth_clip(seed, n, h, w))


def _time(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def _kernel_events(paths, dev):
    """Device events around each C-ABI call of one decode of the whole clip: ms for gather + CRC, inflate, unfilter."""
    from elvis_amd import _lib
    files = [open(p, "rb").read() for p in paths]
    infos = [png.parse_png(d, p) for d, p in zip(files, paths)]
    h, w = infos[0].height, infos[0].width
    out = torch.empty((len(files), h, w, 3), dtype=torch.uint8, device=dev)
    handle = _lib.lib()
    names = ("elvis_png_gather", "elvis_png_inflate", "elvis_png_unfilter")
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

    real = png.lib
    png.lib = lambda: Timed()
    try:
        png._launch_decode(files, infos, out, "bgr", 3)
    finally:
        png.lib = real
    torch.cuda.synchronize(dev)
    ms = {}
    for name, a, b in marks:
        ms[name] = ms.get(name, 0.0) + a.elapsed_time(b)
    return ms, files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    clip = _clip(args.frames, args.height, args.width)
    result = {"frames": args.frames, "height": args.height, "width": args.width, "runs": args.runs}
    with tempfile.TemporaryDirectory(prefix="png_read_bench_") as tmp:
        from PIL import Image
        sets = {}
        pil_dir, dev_dir = os.path.join(tmp, "pil"), os.path.join(tmp, "device")
        os.makedirs(pil_dir)
        sets["pil6"] = [os.path.join(pil_dir, f"{i + 1:05d}.png") for i in range(args.frames)]
        for p, f in zip(sets["pil6"], clip):
            Image.fromarray(np.ascontiguousarray(f[:, :, ::-1]), "RGB").save(p, compress_level=6)
        sets["device_writer"] = [os.path.join(dev_dir, f"{i + 1:05d}.png") for i in range(args.frames)]
        at = 0
        while at < args.frames:                                  # in parts: the writer's own size limit
            png.save_frames_device(torch.from_numpy(clip[at:at + 8]).to(dev), sets["device_writer"][at:at + 8])
            at += 8
        want = torch.from_numpy(clip).to(dev)
        for name, paths in sets.items():
            device_path = lambda: png.load_frames_device(paths, dev)                                      # noqa: E731
            pil_path = lambda: frames_to_device([frameio.load_frame(p) for p in paths], dev)              # noqa: E731
            assert torch.equal(device_path(), want) and torch.equal(pil_path(), want), name
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
            events, files = _kernel_events(paths, dev)
            import _png_read_ref as R
            wk = R.walk(files[0])
            cap = wk.height * (1 + wk.width * wk.bpp)
            # the device writer's stream is literals only: a token a byte; PIL's is counted by the statement
            tokens = cap if name == "device_writer" else R.inflate(wk.stream, cap).tokens
            result[name] = {
                "file_bytes_mean": int(np.mean([os.path.getsize(p) for p in paths])),
                "device_ms_median": round(statistics.median(dev_ms), 2), "pil_ms_median": round(statistics.median(pil_ms), 2),
                "pil_over_device": round(statistics.median(pil_ms) / statistics.median(dev_ms), 3),
                "kernel_ms": {k: round(v, 3) for k, v in events.items()},
                "tokens_frame0": tokens,
                # the streams run side by side, one wave each: the call lasts as long as one stream
                "tokens_per_second_per_stream": round(tokens / (events["elvis_png_inflate"] * 1e-3)),
            }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "png_read_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
