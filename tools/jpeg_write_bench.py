"""The device JPEG writer (csrc/jpeg_write.hip, elvis_amd/jpeg_write.py) on a resident 1080p clip.

    python tools/jpeg_write_bench.py [--frames 30] [--reps 10] [--height 1080] [--width 1920] [--out DIR]
                                     [--restart-rows R | --restart-mcus K] [--measure encode,roundtrip,writers,sizes]

The clip is `synth.synth_clip`.  `--restart-rows` / `--restart-mcus` give the device writer a restart interval (PIL's
files of the comparison get the same one).  `ELVIS_AMD_LIB` names another build of the library, for a comparison in one
session.  Prints one JSON line per measurement:

  encode      device time between events on the stream around `jpeg_write._encode_clip` - the four calls with their two
              small downloads in between - median of `reps` after a warm-up, per frame, with the bytes the algorithm
              needs (the clip read once, the scans written once) as a fraction of the HBM peak
  roundtrip   `jpeg_write.jpeg_roundtrip_device` - encode, the files down, the device reader's decode of them: a host clock
              around the call and a final synchronise (median, min, max), and in one more run device events around
              each C-ABI call of the writer and of the reader (the reader's entropy launch decodes a segment per lane)
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

from elvis_amd import frameio, jpeg, jpeg_write, recompose, synth  # noqa: E402

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


def call_events(fn):
    """Device events around every `elvis_jpeg_*` call that `fn` makes through jpeg_write.py and jpeg.py: {name: ms}."""
    from elvis_amd import _lib
    handle, marks = _lib.lib(), []

    class Timed:
        def __getattr__(self, name):
            real = getattr(handle, name)
            if not name.startswith("elvis_jpeg_") or name in ("elvis_jpeg_frame_blocks", "elvis_jpeg_segments"):
                return real

            def call(*args):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                rc = real(*args)
                b.record()
                marks.append((name, a, b))
                return rc
            return call

    saved = jpeg_write.lib, jpeg.lib
    jpeg_write.lib = jpeg.lib = lambda: Timed()
    try:
        fn()
    finally:
        jpeg_write.lib, jpeg.lib = saved
    torch.cuda.synchronize()
    ms = {}
    for name, a, b in marks:
        ms[name] = round(ms.get(name, 0.0) + a.elapsed_time(b), 4)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--out", default=None)
    ap.add_argument("--restart-rows", type=int, default=0)
    ap.add_argument("--restart-mcus", type=int, default=0)
    ap.add_argument("--measure", default="encode,roundtrip,writers,sizes")
    args = ap.parse_args()
    measure = set(args.measure.split(","))
    restart = (args.restart_rows, args.restart_mcus)
    restart_kw = {k: v for k, v in (("restart_rows", args.restart_rows), ("restart_mcus", args.restart_mcus)) if v}
    pil_kw = {k: v for k, v in (("restart_marker_rows", args.restart_rows), ("restart_marker_blocks", args.restart_mcus)) if v}
    setting = dict(restart_kw, library=os.environ.get("ELVIS_AMD_LIB") or "built")
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

    encode = (lambda: jpeg_write._encode_clip(clip, "bgr", 95, "420", "bench", restart=restart)) if any(restart) else \
        (lambda: jpeg_write._encode_clip(clip, "bgr", 95, "420", "bench"))
    if "encode" in measure:
        times = []
        encode()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            got = encode()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        scan_bytes = int(got["out_off"][-1])
        ms = statistics.median(times)
        report(measurement="encode", **setting, frames=n, height=h, width=w, ms_per_clip=round(ms, 3), ms_per_frame=round(ms / n, 4),
               ms_min=round(min(times), 3), ms_max=round(max(times), 3), segments_per_frame=got.get("segments", 1),
               bytes_per_frame=round((len(got["header"]) * n + scan_bytes) / n), algorithmic_bytes=clip.numel() + scan_bytes,
               fraction_of_hbm_peak=round((clip.numel() + scan_bytes) / (ms * 1e-3) / (HBM_PEAK_GBS * 1e9), 5), calls_ms=call_events(encode))

    if "roundtrip" in measure:
        def roundtrip():
            return jpeg_write.jpeg_roundtrip_device(clip, 95, "420", **restart_kw)

        med, lo, hi = host_ms(roundtrip, args.reps)
        calls = call_events(roundtrip)
        report(measurement="roundtrip", **setting, frames=n, ms_per_clip=round(med, 2), ms_min=round(lo, 2), ms_max=round(hi, 2), calls_ms=calls,
               encode_calls_ms=round(sum(v for k, v in calls.items() if k in ("elvis_jpeg_fdct", "elvis_jpeg_bits", "elvis_jpeg_pack", "elvis_jpeg_stuff",
                                                                             "elvis_jpeg_bits_rst", "elvis_jpeg_pack_rst", "elvis_jpeg_stuff_rst")), 3),
               reader_entropy_ms=calls.get("elvis_jpeg_entropy"), bytes_per_frame=round(float(roundtrip()[1].mean())))

    if not measure & {"writers", "sizes"}:
        return

    def device_writer():
        jpeg_write.save_jpeg_frames_device(clip, paths["device"], **restart_kw)

    def pil_path():
        for f, p in zip(recompose.frames_to_host(clip), paths["pil75"]):
            frameio.save_frame(f, p)

    def pil_95():
        for f, p in zip(recompose.frames_to_host(clip), paths["pil95"]):
            Image.fromarray(np.ascontiguousarray(f[:, :, ::-1]), "RGB").save(p, quality=95, subsampling=2, **pil_kw)

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
