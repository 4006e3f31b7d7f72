"""The device JPEG writer (csrc/jpeg_write.hip, elvis_amd/jpeg_write.py) on a resident 1080p clip.

    python tools/jpeg_write_bench.py [--frames 30] [--reps 10] [--height 1080] [--width 1920] [--out DIR]

The clip is `synth.synth_clip`.  Prints one JSON line per measurement:

  encode      device time between events on the stream around `jpeg_write._encode_clip` - the four calls with their two
              small downloads in between - median of `reps` after a warm-up, per frame, with the bytes the algorithm
              needs (the clip read once, the scans written once) as a fraction of the HBM peak
  writers     a host clock from the resident clip to the files on disk: `jpeg_write.save_jpeg_frames_device` (encode, one
              download, write) against the path it replaces, the clip brought down and `frameio.save_frame` to `.jpg`
              per frame (PIL at its own quality 75); and PIL asked for the device writer's settings, quality 95 and
              4:2:0, for the like-for-like cost
  sizes       bytes per frame of the three
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
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elvis_amd import frameio, jpeg_write, recompose, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0


def report(**kw):
    print(json.dumps(kw), flush=True)


def host_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    n, h, w = args.frames, args.height, args.width
    clip = torch.from_numpy(np.ascontiguousarray(synth.synth_clip(7, n, h, w)[..., ::-1])).to(dev)     # BGR, as the drivers hold it
    out = args.out or tempfile.mkdtemp(prefix="jpeg_write_bench_")
    dirs = {k: os.path.join(out, k) for k in ("device", "pil75", "pil95")}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
    paths = {k: [os.path.join(d, f"{i + 1:05d}.jpg") for i in range(n)] for k, d in dirs.items()}

    times = []
    jpeg_write._encode_clip(clip, "bgr", 95, "420", "bench")
    torch.cuda.synchronize()
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        got = jpeg_write._encode_clip(clip, "bgr", 95, "420", "bench")
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    scan_bytes = int(got["out_off"][-1])
    ms = statistics.median(times)
    report(measurement="encode", frames=n, height=h, width=w, ms_per_clip=round(ms, 3), ms_per_frame=round(ms / n, 4),
           ms_min=round(min(times), 3), ms_max=round(max(times), 3), algorithmic_bytes=clip.numel() + scan_bytes,
           fraction_of_hbm_peak=round((clip.numel() + scan_bytes) / (ms * 1e-3) / (HBM_PEAK_GBS * 1e9), 5))

    def device_writer():
        jpeg_write.save_jpeg_frames_device(clip, paths["device"])

    def pil_path():
        for f, p in zip(recompose.frames_to_host(clip), paths["pil75"]):
            frameio.save_frame(f, p)

    def pil_95():
        for f, p in zip(recompose.frames_to_host(clip), paths["pil95"]):
            Image.fromarray(np.ascontiguousarray(f[:, :, ::-1]), "RGB").save(p, quality=95, subsampling=2)

    rows = {}
    for name, fn in (("device", device_writer), ("pil75", pil_path), ("pil95", pil_95)):
        med, lo, hi = host_ms(fn, max(3, args.reps // 2))
        rows[name] = med
        report(measurement="writers", writer=name, ms_per_clip=round(med, 2), ms_min=round(lo, 2), ms_max=round(hi, 2),
               frames_per_second=round(n / (med * 1e-3), 1))
    report(measurement="writers", device_over_pil75=round(rows["pil75"] / rows["device"], 2), device_over_pil95=round(rows["pil95"] / rows["device"], 2))
    report(measurement="sizes", **{k: round(sum(os.path.getsize(p) for p in ps) / n) for k, ps in paths.items()})
    same = all(open(a, "rb").read().split(b"\xff\xda", 1)[1] == open(b, "rb").read().split(b"\xff\xda", 1)[1]
               for a, b in zip(paths["device"], paths["pil95"]))
    report(measurement="sizes", device_scan_equals_pil95=same)


if __name__ == "__main__":
    main()
