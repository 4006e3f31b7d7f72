#!/usr/bin/env python3
"""Benchmark of the Real-ESRGAN slot (csrc/rrdb.hip, elvis_amd/realesrgan.py) on one MI355X.
    python tools/rrdb_bench.py [--runs N] [--frames F] [--skip-e2e] [--json PATH]

1. Kernels: the five dense-block shapes at 270 x 480 (in place in a 192-channel buffer) and the tail convs
   (conv_up1, conv_up2, conv_hr, conv_last up to 1080p): device time by HIP events over `--inner` back-to-back launches,
   median of `--runs` timed rounds after a warm-up, and the achieved FLOP/s counted from the shapes the kernel runs
   (2 * 9 * cin * cout per output pixel, padded channels included).  Beside each, in the same process and interleaved
   round by round: `elvis_conv2d` (ops.PackedConv) on the same cin / cout and input pitch with act = 0 - the only thing the
   rest of the library can run at those shapes.  It is not the same function (no LeakyReLU, no scaled residuals, no
   channel offset, f16 output only): context, not a gate.
2. End to end, host to host: restored 1080p frames per second of `restore_frames_realesrgan` with `RealESRGAN_x4plus`
   (`schedule="single4x"`) and with `RealESRGAN_x2plus` (the staged loop), seeded synthetic weights, every block at
   level 2 (the /4 level).  Median of `--runs` calls after a warm-up call.
Random (gaussian) data throughout.  No GPU: an error, not a fallback."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from elvis_amd import _lib as L, ops, realesrgan, restore  # noqa: E402

# name: (cin, cout, h, w, upsample, lrelu, in place at channel offset cin, out_u8)
SHAPES = {
    "dense_conv1_64to32": (64, 32, 270, 480, False, True, True, False),
    "dense_conv2_96to32": (96, 32, 270, 480, False, True, True, False),
    "dense_conv3_128to32": (128, 32, 270, 480, False, True, True, False),
    "dense_conv4_160to32": (160, 32, 270, 480, False, True, True, False),
    "dense_conv5_192to64": (192, 64, 270, 480, False, False, False, False),
    "conv_up1_540p": (64, 64, 270, 480, True, True, False, False),
    "conv_up2_1080p": (64, 64, 540, 960, True, True, False, False),
    "conv_hr_1080p": (64, 64, 1080, 1920, False, True, False, False),
    "conv_last_1080p_u8": (64, 32, 1080, 1920, False, False, False, True),
}


def _time(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def bench_kernels(dev, runs, inner):
    g = torch.Generator().manual_seed(0)
    lib = L.lib()
    rows = []
    for name, (cin, cout, h, w, ups, lrelu, inplace, u8) in SHAPES.items():
        ho, wo = (2 * h, 2 * w) if ups else (h, w)
        cout_real = 3 if u8 else cout
        wt = torch.randn(cout_real, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
        bias = torch.randn(cout_real, generator=g) * 0.1
        packed, b, _, _ = realesrgan.pack_conv(wt, bias)
        wp, bd = torch.from_numpy(packed.view(np.int16)).to(dev), torch.from_numpy(b).to(dev)
        pitch = 192 if not ups and h == 270 else 64
        x = torch.randn((1, h, w, pitch), device=dev, dtype=torch.float16)
        if u8:
            out, coff = torch.empty((1, ho, wo, 3), device=dev, dtype=torch.uint8), 0
        elif inplace:
            out, coff = x, cin
        else:
            out, coff = torch.empty((1, ho, wo, cout), device=dev, dtype=torch.float16), 0
        res = x if name.startswith("dense_conv5") else None          # x5 * 0.2 + x
        stream = L.stream_handle(dev)

        def ours():
            L.check(lib.elvis_rrdb_conv3x3(x.data_ptr(), pitch, wp.data_ptr(), bd.data_ptr(), out.data_ptr(), out.shape[-1], coff,
                                           0, 0, L.ptr(res), pitch if res is not None else 0, 1, h, w, cin, cout, int(ups),
                                           int(lrelu), 0.2 if res is not None else 1.0, 0.0, int(u8), 0, stream), dev)

        conv = ops.PackedConv(wt, bias, torch.float16, dev, cin)
        xa = ops.Act(x, cin)
        oa = ops.new_act(1, ho, wo, cout_real, torch.float16, dev, zero=False)

        def theirs():
            conv(xa, upsample=bool(ups), act=0, out=oa)

        ours(), theirs()
        torch.cuda.synchronize()
        # a timed window of about 20 ms at least: a window of a few launches measures the clock and the queue
        reps = max(inner, min(4000, int(20.0 / max(_time(ours, inner), 1e-3))))
        to, tt = [], []
        for _ in range(runs):                       # interleaved: drift and neighbours hit both alike
            to.append(_time(ours, reps))
            tt.append(_time(theirs, reps))
        flop = 2.0 * 9 * cin * cout * ho * wo
        mo, mt = statistics.median(to), statistics.median(tt)
        rows.append(dict(name=name, cin=cin, cout=cout, ho=ho, wo=wo, ms=mo, ms_min=min(to), ms_max=max(to),
                         tflops=flop / mo * 1e-9, conv2d_ms=mt, conv2d_ms_min=min(tt), conv2d_ms_max=max(tt),
                         conv2d_kernel=lib.elvis_last_launch().decode()))
        print(f"{name:24s} rrdb {mo:7.3f} ms [{min(to):.3f}, {max(to):.3f}]  {flop / mo * 1e-9:6.1f} TFLOP/s   "
              f"elvis_conv2d {mt:7.3f} ms [{min(tt):.3f}, {max(tt):.3f}]  {rows[-1]['conv2d_kernel']}", flush=True)
    return rows


def bench_e2e(dev, runs, nframes):
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, size=(1080, 1920, 3), dtype=np.uint8) for _ in range(nframes)]
    maps = np.full((nframes, 1080 // 8, 1920 // 8), 2, np.int32)
    rows = []
    for model_name, schedule in (("RealESRGAN_x4plus", "single4x"), ("RealESRGAN_x2plus", "staged")):
        call = lambda: restore.restore_frames_realesrgan(frames, maps, 8, dev, model_name=model_name, schedule=schedule)
        call()
        ts = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()                                   # host to host: returns numpy frames
            ts.append(time.perf_counter() - t0)
        med = statistics.median(ts)
        rows.append(dict(model=model_name, schedule=schedule, frames=nframes, s=med, s_min=min(ts), s_max=max(ts), fps=nframes / med))
        print(f"{model_name} {schedule}: {nframes / med:.2f} restored 1080p frames/s host to host "
              f"({med:.3f} s [{min(ts):.3f}, {max(ts):.3f}] per {nframes} frames)", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")
    dev = L.resolve_device("cuda:0")
    with torch.cuda.device(dev):
        result = dict(kernels=bench_kernels(dev, a.runs, a.inner))
        if not a.skip_e2e:
            result["e2e"] = bench_e2e(dev, a.runs, a.frames)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
