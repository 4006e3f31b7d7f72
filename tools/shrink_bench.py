"""Device time of the ELVIS v1 shrink / stretch kernels on a 30-frame 1080p clip (block 8 and 16, 25 % removed),
host-to-host frames/s of `stretch_video_frames`, and the CPU time of the same work by the numpy restatement
(tests/_shrink_ref.py - the reference-equivalent Python, on this box's CPU share) as context.

    python tools/shrink_bench.py [--frames 30] [--reps 10] [--no-cpu]

Prints one JSON line per measurement.  GB/s are algorithmic: kept blocks read + whole output written (+ the
full-resolution mask for a stretch), next to the 8 TB/s HBM peak recompose_rows_u8_kernel is rated against.
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

from elvis_amd import shrink  # noqa: E402

HBM_PEAK_GBS = 8000.0


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, amount = args.frames, 0.25
    rng = np.random.default_rng(0)
    for h, w, b in ((1080, 1920, 8), (1072, 1920, 16)):
        by, bx = h // b, w // b
        frames = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev)
        scores = torch.from_numpy(rng.random((n, by, bx))).to(dev)
        frame_bytes = h * w * 3
        # ---- shrinks: selection and gather timed apart
        shrunk, mask, src_of = shrink.shrink_topk_device(frames, scores, b, amount)
        kept = src_of.shape[1] * src_of.shape[2] * b * b * 3
        t_sel = device_ms(lambda: shrink.shrink_topk_device(frames, scores, b, amount), args.reps)
        t_g = device_ms(lambda: shrink.block_gather_device(frames, src_of, b, (by, bx), out=shrunk), args.reps)
        alg = n * (2 * kept + src_of[0].numel() * 4)
        report(what="shrink_topk", block=b, frames=n, select_plus_gather_ms=round(t_sel, 4), gather_ms=round(t_g, 4),
               gather_gbs=round(alg / t_g / 1e6, 1), gather_frac_hbm=round(alg / t_g / 1e6 / HBM_PEAK_GBS, 3))
        for mode in ("rows", "rows_cols"):
            t = device_ms(lambda: shrink.shrink_passes_device(frames, scores, b, amount, mode), max(2, args.reps // 3))
            report(what=f"shrink_passes_{mode}", block=b, frames=n, select_plus_gather_ms=round(t, 4),
                   frames_per_s=round(n / t * 1e3, 1))
        # ---- stretch: rank map + gather with the fused full-resolution mask
        out = torch.empty_like(frames)
        t_all = device_ms(lambda: shrink.stretch_device(shrunk, mask, b, "flat", out=out, fullres_mask=True), args.reps)
        idx = shrink.stretch_index_device(mask, (by, src_of.shape[2]), "flat")
        t_g = device_ms(lambda: shrink.block_gather_device(shrunk, idx, b, out=out, fullres_mask=True), args.reps)
        t_nomask = device_ms(lambda: shrink.block_gather_device(shrunk, idx, b, out=out), args.reps)
        alg = n * (kept + frame_bytes + by * bx * 4)
        report(what="stretch", block=b, frames=n, index_plus_gather_ms=round(t_all, 4), gather_with_mask_ms=round(t_g, 4),
               gather_ms=round(t_nomask, 4), gather_gbs=round(alg / t_nomask / 1e6, 1),
               gather_frac_hbm=round(alg / t_nomask / 1e6 / HBM_PEAK_GBS, 3),
               gather_with_mask_gbs=round((alg + n * h * w) / t_g / 1e6, 1),
               gather_with_mask_frac_hbm=round((alg + n * h * w) / t_g / 1e6 / HBM_PEAK_GBS, 3))
        # ---- host to host
        shrunk_h = [a for a in shrunk.cpu().numpy()]
        mask_h = [a for a in mask.cpu().numpy()]
        shrink.stretch_video_frames(shrunk_h, mask_h, b)
        t0 = time.perf_counter()
        shrink.stretch_video_frames(shrunk_h, mask_h, b)
        dt = time.perf_counter() - t0
        report(what="stretch_video_frames_host_to_host", block=b, frames=n, seconds=round(dt, 4), frames_per_s=round(n / dt, 1))
        if not args.no_cpu:
            import _shrink_ref as R
            f0, s0 = frames[0].cpu().numpy(), scores[0].cpu().numpy()
            cpu = {}
            for name, fn in (("apply_selective_removal", lambda: R.apply_selective_removal(f0, s0, b, amount)),
                             ("shrink_frame_row_only", lambda: R.shrink_frame_row_only(f0, s0, b, amount)),
                             ("shrink_frame_position_map", lambda: R.shrink_frame_position_map(f0, s0, b, amount)),
                             ("stretch_frame", lambda: R.stretch_frame(shrunk_h[0], mask_h[0], b))):
                t0 = time.perf_counter()
                fn()
                cpu[name + "_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            report(what="cpu_restatement_one_frame", block=b, threads=torch.get_num_threads(), **cpu)


if __name__ == "__main__":
    main()
