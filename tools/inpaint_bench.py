"""Device time of the wavefront Telea inpainter (csrc/inpaint.hip) on a 30-frame 1080p clip with 25 % and 50 % of the
blocks removed by `shrink_topk_device` (block 8 and block 16): the preparation pass and the fill launches timed apart,
the deepest wave K, hole pixels per second, stretch + inpaint resident, and the host-to-host rate of
`inpaint_with_opencv`.

    python tools/inpaint_bench.py [--frames 30] [--reps 5]

Prints one JSON line per measurement.  Times are device times between events on the stream, median of `reps` after
one warm-up call; the one synchronisation of a clip (the download of the per-wave counts) is inside `inpaint_ms` and
outside `prepare_ms` / `fill_ms`.  Context only: the reference's notebook gives 5.71 frames/s for its whole
CV2-inpaint stage on unstated hardware; the numpy statement in tests/_inpaint_ref.py is a specification, not a baseline.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elvis_amd import inpaint, shrink  # noqa: E402
from elvis_amd._lib import check, lib, ptr  # noqa: E402
from elvis_amd.ops import _s  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.frames
    rng = np.random.default_rng(0)
    for h, w, b in ((1080, 1920, 8), (1072, 1920, 16)):
        by, bx = h // b, w // b
        frames = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev)
        scores = torch.from_numpy(rng.random((n, by, bx))).to(dev)
        for amount in (0.25, 0.5):
            shrunk, mask, _ = shrink.shrink_topk_device(frames, scores, b, amount)
            stretched, full = shrink.stretch_device(shrunk, mask, b, "flat", fullres_mask=True)
            holes = int((full != 0).sum().item())
            work = stretched.clone()
            ws = torch.empty(lib().elvis_inpaint_workspace_bytes(n, h, w), dtype=torch.uint8, device=dev)

            def prepare():
                check(lib().elvis_inpaint_prepare(ptr(full), 0, ptr(ws), n, h, w, _s(work)), dev)
            prepare()
            counts = ws[:(h + w + 2) * 4].view(torch.int32).cpu().numpy()
            k = int(np.flatnonzero(counts)[-1])
            assert int(counts.sum()) == holes
            host = np.ascontiguousarray(counts[:k + 1], dtype=np.int32)

            def fill():
                check(lib().elvis_inpaint_fill(ptr(work), ptr(ws), n, h, w, 3, host.ctypes.data_as(C.c_void_p), k + 1, _s(work)), dev)
            t_prep = device_ms(prepare, args.reps)
            t_fill = device_ms(fill, args.reps)
            t_all = device_ms(lambda: inpaint.inpaint_device(stretched, full, out=work), args.reps)
            t_both = device_ms(lambda: inpaint.stretch_and_inpaint_device(shrunk, mask, b), args.reps)
            report(what="inpaint", block=b, removed=amount, frames=n, hole_pixels=holes, K=k, prepare_ms=round(t_prep, 3),
                   fill_ms=round(t_fill, 3), inpaint_ms=round(t_all, 3), stretch_plus_inpaint_ms=round(t_both, 3),
                   hole_mpix_per_s=round(holes / (t_prep + t_fill) / 1e3, 1), fill_hole_mpix_per_s=round(holes / t_fill / 1e3, 1),
                   frames_per_s=round(n / t_all * 1e3, 1), workspace_mb=round(ws.numel() / 2 ** 20, 1))
            if amount == 0.25:
                frames_h, mask_h = stretched.cpu().numpy(), mask.cpu().numpy() != 0
                inpaint.inpaint_with_opencv(frames_h, mask_h)
                t0 = time.perf_counter()
                inpaint.inpaint_with_opencv(frames_h, mask_h)
                dt = time.perf_counter() - t0
                report(what="inpaint_with_opencv_host_to_host", block=b, removed=amount, frames=n, seconds=round(dt, 4),
                       frames_per_s=round(n / dt, 1))
            del ws, work, stretched, full, shrunk


if __name__ == "__main__":
    main()
