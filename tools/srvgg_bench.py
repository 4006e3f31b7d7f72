#!/usr/bin/env python3
"""Benchmark of the SRVGGNetCompact models of the Real-ESRGAN slot (csrc/srvgg.hip, elvis_amd/srvgg.py) on one MI355X.
    python tools/srvgg_bench.py [--runs N] [--frames F] [--skip-e2e] [--json PATH]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o p -- python tools/srvgg_bench.py --forward-only

1. Kernels at 270 x 480 (the /4 level of a 1080p frame): the first layer (32 padded input channels), a body layer
   (64 -> 64, PReLU) and the tail (64 -> 48, pixel shuffle, base, bytes at 1080p).  Device time by HIP events over
   back-to-back launches, median of `--runs` timed rounds after a warm-up, and the achieved FLOP/s counted from the
   shapes the kernel runs (2 * 9 * cin * cout per pixel, padded channels included).  Beside each, in the same process
   and interleaved round by round: `elvis_conv2d` (ops.PackedConv) on the same cin / cout with act = 0 - the only thing
   the rest of the library can run at those shapes.  It is not the same function (no PReLU, no shuffle, no base, f16
   output only): context, not a gate.
2. Per-frame kernel time sums: the device time of one `forward` of `--frames` resident /4-level frames, HIP events
   around the whole invocation (its kernels run back to back on one stream, so this is their sum and the gaps between
   them), divided by the frames - for both SRVGG models and for `RealESRGAN_x4plus` in the same run.  For the SRVGG
   models also the sum made of part 1: first + num_conv * layer + tail.  The one condition this tool checks:
   `realesr-general-x4v3` (1/15 of the FLOPs) must take less than `RealESRGAN_x4plus`; otherwise it exits 1.
3. End to end, host to host: restored 1080p frames per second of `restore_frames_realesrgan(schedule="single4x")` for
   the same three models, seeded synthetic weights, every block at level 2.  Median of `--runs` calls after a warm-up.
`--forward-only` runs nothing but `--runs` invocations of each model's `forward` on `--frames` /4-level frames after a
warm-up one: the workload for a kernel trace in a run of its own (per-kernel times by name; the tool's own numbers are
taken with the profiler off).
Random data throughout.  No GPU: an error, not a fallback."""
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
from elvis_amd import _lib as L, ops, restore, srvgg  # noqa: E402

H, W = 270, 480
# name: (cin the kernel runs, real cin, cout, tail)
SHAPES = {"first_3to64_prelu": (32, 3, 64, False), "layer_64to64_prelu": (64, 64, 64, False),
          "tail_64to48_shuffle_u8_1080p": (64, 64, 48, True)}
MODELS = ("realesr-animevideov3", "realesr-general-x4v3", "RealESRGAN_x4plus")


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
    lib, stream = L.lib(), L.stream_handle(dev)
    rows = []
    for name, (cin, cin_real, cout, tail) in SHAPES.items():
        wt = torch.randn(cout, cin_real, 3, 3, generator=g) / math.sqrt(9 * cin_real)
        bias = torch.randn(cout, generator=g) * 0.1
        packed, b, _, _ = srvgg.pack_conv(wt, bias)
        wp, bd = torch.from_numpy(packed.view(np.int16)).to(dev), torch.from_numpy(b).to(dev)
        slope = (0.2 + 0.1 * torch.randn(64, generator=g)).to(dev)
        x = torch.randn((1, H, W, cin), device=dev, dtype=torch.float16)
        base = torch.rand((1, H, W, 32), device=dev, dtype=torch.float16)
        if tail:
            out = torch.empty((1, 4 * H, 4 * W, 3), device=dev, dtype=torch.uint8)

            def ours():
                L.check(lib.elvis_srvgg_tail(x.data_ptr(), cin, wp.data_ptr(), bd.data_ptr(), base.data_ptr(), 32,
                                             out.data_ptr(), 1, H, W, 1, 1, stream), dev)
        else:
            out = torch.empty((1, H, W, 64), device=dev, dtype=torch.float16)

            def ours():
                L.check(lib.elvis_srvgg_conv3x3(x.data_ptr(), cin, wp.data_ptr(), bd.data_ptr(), slope.data_ptr(),
                                                out.data_ptr(), 64, 1, H, W, cin, stream), dev)

        wt_run = torch.zeros(cout, cin, 3, 3)          # the shape the kernel runs: padded input channels
        wt_run[:, :cin_real] = wt
        conv = ops.PackedConv(wt_run, bias, torch.float16, dev, cin)
        xa = ops.Act(x, cin)
        oa = ops.new_act(1, H, W, cout, torch.float16, dev, zero=False)

        def theirs():
            conv(xa, act=0, out=oa)

        ours(), theirs()
        torch.cuda.synchronize()
        # a timed window of about 20 ms at least: a window of a few launches measures the clock and the queue
        reps = max(inner, min(4000, int(20.0 / max(_time(ours, inner), 1e-3))))
        to, tt = [], []
        for _ in range(runs):                       # interleaved: drift and neighbours hit both alike
            to.append(_time(ours, reps))
            tt.append(_time(theirs, reps))
        flop = 2.0 * 9 * cin * cout * H * W
        mo, mt = statistics.median(to), statistics.median(tt)
        rows.append(dict(name=name, cin=cin, cout=cout, h=H, w=W, ms=mo, ms_min=min(to), ms_max=max(to),
                         tflops=flop / mo * 1e-9, conv2d_ms=mt, conv2d_ms_min=min(tt), conv2d_ms_max=max(tt),
                         conv2d_kernel=lib.elvis_last_launch().decode()))
        print(f"{name:30s} srvgg {mo:7.4f} ms [{min(to):.4f}, {max(to):.4f}]  {flop / mo * 1e-9:6.1f} TFLOP/s   "
              f"elvis_conv2d {mt:7.4f} ms [{min(tt):.4f}, {max(tt):.4f}]  {rows[-1]['conv2d_kernel']}", flush=True)
    return rows


def bench_forward(dev, runs, nframes, kernels):
    g = torch.Generator().manual_seed(1)
    lr = torch.randint(0, 256, (nframes, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    by = {r["name"]: r["ms"] for r in kernels}
    rows = []
    for name in MODELS:
        model = restore.get_realesrgan_upsampler(dev, model_name=name)
        model.forward(lr)
        torch.cuda.synchronize()
        ts = [_time(lambda: model.forward(lr), 1) / nframes for _ in range(runs)]
        row = dict(model=name, frames=nframes, ms_per_frame=statistics.median(ts), ms_min=min(ts), ms_max=max(ts))
        if isinstance(model, srvgg.SRVGGModel):
            row["ms_from_kernels"] = by["first_3to64_prelu"] + model.cfg.num_conv * by["layer_64to64_prelu"] + \
                by["tail_64to48_shuffle_u8_1080p"]
        rows.append(row)
        extra = f", first + {model.cfg.num_conv} layers + tail = {row['ms_from_kernels']:.3f} ms" if "ms_from_kernels" in row else ""
        print(f"{name}: forward {row['ms_per_frame']:.3f} ms per /4-level frame [{min(ts):.3f}, {max(ts):.3f}] "
              f"({nframes} frames an invocation){extra}", flush=True)
    return rows


def bench_e2e(dev, runs, nframes):
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, size=(1080, 1920, 3), dtype=np.uint8) for _ in range(nframes)]
    maps = np.full((nframes, 1080 // 8, 1920 // 8), 2, np.int32)
    rows = []
    for name in MODELS:
        call = lambda: restore.restore_frames_realesrgan(frames, maps, 8, dev, model_name=name, schedule="single4x")
        call()
        ts = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()                                   # host to host: returns numpy frames
            ts.append(time.perf_counter() - t0)
        med = statistics.median(ts)
        rows.append(dict(model=name, schedule="single4x", frames=nframes, s=med, s_min=min(ts), s_max=max(ts), fps=nframes / med,
                         fps_min=nframes / max(ts), fps_max=nframes / min(ts)))
        print(f"{name} single4x: {nframes / med:.2f} restored 1080p frames/s host to host "
              f"({med:.3f} s [{min(ts):.3f}, {max(ts):.3f}] per {nframes} frames)", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--forward-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")
    dev = L.resolve_device("cuda:0")
    if a.forward_only:
        with torch.cuda.device(dev):
            lr = torch.randint(0, 256, (a.frames, H, W, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).to(dev)
            for name in MODELS:
                model = restore.get_realesrgan_upsampler(dev, model_name=name)
                for _ in range(a.runs + 1):
                    model.forward(lr)
                torch.cuda.synchronize()
                print(f"{name}: {a.runs + 1} invocations of forward on {a.frames} frames of {H} x {W}", flush=True)
        return
    with torch.cuda.device(dev):
        result = dict(kernels=bench_kernels(dev, a.runs, a.inner))
        result["forward"] = bench_forward(dev, a.runs, a.frames, result["kernels"])
        if not a.skip_e2e:
            result["e2e"] = bench_e2e(dev, a.runs, a.frames)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
    fw = {r["model"]: r["ms_per_frame"] for r in result["forward"]}
    if not fw["realesr-general-x4v3"] < fw["RealESRGAN_x4plus"]:
        print(f"INCONSISTENT: realesr-general-x4v3 takes {fw['realesr-general-x4v3']:.3f} ms a frame, RealESRGAN_x4plus "
              f"{fw['RealESRGAN_x4plus']:.3f} ms, with 1/15 of the FLOPs", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
