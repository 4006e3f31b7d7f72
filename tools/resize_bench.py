"""Device time of the intake's INTER_AREA resize (`intake.resize_area_device`) on a 30-frame clip at the size pairs a
working resolution is reached by, with `enhance.resize_lanczos4_device` at the same sizes (the nearest kernel the
package had before) and the numpy statement (tests/_resize_ref.py, one frame, on this box's CPU share) as context.

    python tools/resize_bench.py [--frames 30] [--reps 20] [--no-cpu]

Prints one JSON line per measurement.  GB/s are algorithmic - the source read once plus the result written once - next to
the 8 TB/s HBM peak; device time is by events around `reps` launches after a warm-up launch.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from elvis_amd import enhance, intake  # noqa: E402

HBM_PEAK_GBS = 8000.0
PAIRS = (("2160p->1080p", (2160, 3840), (1080, 1920)), ("1080p->720p", (1080, 1920), (720, 1280)),
         ("1080p->640x360", (1080, 1920), (360, 640)), ("2160p->720p", (2160, 3840), (720, 1280)))


def device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def report(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.frames
    for name, (hs, ws), (hd, wd) in PAIRS:
        frames = torch.randint(0, 256, (n, hs, ws, 3), dtype=torch.uint8, device=dev)
        out = torch.zeros((n, hd, wd, 3), dtype=torch.uint8, device=dev)
        alg = n * 3 * (hs * ws + hd * wd)
        th, tw, lds = intake.resize_area_plan(hs, ws, hd, wd, 3)
        t = device_ms(lambda: intake.resize_area_device(frames, hd, wd, out=out), args.reps)
        report(what="resize_area", pair=name, frames=n, tile=[th, tw], lds_bytes=lds, ms_per_clip=round(t, 4),
               gbs=round(alg / t / 1e6, 1), frac_hbm=round(alg / t / 1e6 / HBM_PEAK_GBS, 3))
        t = device_ms(lambda: enhance.resize_lanczos4_device(frames, hd, wd), max(2, args.reps // 4))
        report(what="resize_lanczos4", pair=name, frames=n, ms_per_clip=round(t, 4), gbs=round(alg / t / 1e6, 1),
               frac_hbm=round(alg / t / 1e6 / HBM_PEAK_GBS, 3))
        if not args.no_cpu:
            import _resize_ref as R
            one = frames[:1].cpu().numpy()
            t0 = time.perf_counter()
            want = R.resize_area_u8(one, hd, wd)
            dt = time.perf_counter() - t0
            same = bool((out[:1].cpu().numpy() == want).all())
            report(what="cpu_statement_one_frame", pair=name, threads=torch.get_num_threads(), ms=round(dt * 1e3, 1), device_equal=same)
        del frames, out


if __name__ == "__main__":
    main()
