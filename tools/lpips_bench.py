"""Time of the LPIPS (AlexNet) score on a 30-frame 1080p pair of clips.

    python tools/lpips_bench.py [--frames 30] [--repeats 20] [--out FILE]

`lpips_device` on two resident BGR clips: device events around the call, median and minimum over the repeats after
warm-up, with the algorithmic FLOPs of the five convolutions of both clips over the median as a fraction of the 157
TFLOP/s fp32 peak.  Then one pass of four frame pairs stage by stage (stem, max-pools, 5x5 conv, the three 3x3 convs of
elvis_conv2d, the five distances), each between device events: its share of the pass and, for the convs, its own
fraction of the peak.  Last, `evaluate_fg_bg_metrics` host to host without and with the model.  One JSON line per
measurement.
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

from elvis_amd import lpips, metrics, synth  # noqa: E402
from elvis_amd.recompose import frames_to_device  # noqa: E402

FP32_PEAK = 157.0e12


def conv_flops(h: int, w: int):
    """Algorithmic FLOPs (2 per multiply-add) of the five convs for one h x w image, by layer."""
    s = lambda v: (v - 7) // 4 + 1
    p = lambda v: (v - 3) // 2 + 1
    h0, w0 = s(h), s(w)
    h1, w1 = p(h0), p(w0)
    h2, w2 = p(h1), p(w1)
    return {"stem": 2.0 * 363 * 64 * h0 * w0, "conv5": 2.0 * 1600 * 192 * h1 * w1, "conv3_192_384": 2.0 * 1728 * 384 * h2 * w2,
            "conv3_384_256": 2.0 * 3456 * 256 * h2 * w2, "conv3_256_256": 2.0 * 2304 * 256 * h2 * w2}


def device_ms(call, repeats: int, warmup: int = 2):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    t = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        stop.record()
        stop.synchronize()
        t.append(start.elapsed_time(stop))
    return float(np.median(t)), float(np.min(t))


def host_ms(call, repeats: int, warmup: int = 1):
    for _ in range(warmup):
        call()
    t = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_bench needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    h, w, n = 1080, 1920, args.frames
    refs = list(synth.synth_clip(21, n, h, w))
    rng = np.random.default_rng(5)
    decs = [np.clip(f.astype(np.int16) + rng.integers(-9, 10, f.shape), 0, 255).astype(np.uint8) for f in refs]
    model = lpips.get_lpips_model(dev)
    a, b = frames_to_device(refs, dev), frames_to_device(decs, dev)
    flops = conv_flops(h, w)
    per_image = sum(flops.values())
    lines = []

    def report(**line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    report(call="conv_flops", gflop_per_image=round(per_image / 1e9, 2), by_layer={k: round(v / 1e9, 2) for k, v in flops.items()})
    med, lo = device_ms(lambda: lpips.lpips_device(a, b, model), args.repeats)
    report(call="lpips_device", clock="device events", frames=n, ms_median=round(med, 3), ms_min=round(lo, 3), ms_per_pair=round(med / n, 3),
           tflops=round(2 * n * per_image / (med * 1e-3) / 1e12, 2), fp32_peak_fraction=round(2 * n * per_image / (med * 1e-3) / FP32_PEAK, 4))

    # ---- one pass of four pairs, stage by stage
    k = min(lpips.LPIPS_PAIRS_PER_PASS, n)
    rect = (0, h, 0, w)
    stages = []

    def timed(name, call, work=None):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = call()
        stop.record()
        stages.append((name, work, start, stop))
        return out

    def one_pass():
        del stages[:]
        feats = []
        for clip in (a[:k], b[:k]):
            t0 = timed("lpips_stem_kernel", lambda: lpips.stem_device(clip, model, None, rect, "bgr"), k * flops["stem"])
            p0 = timed("lpips_maxpool_kernel", lambda: lpips.maxpool_device(t0))
            t1 = timed("lpips_conv5_kernel", lambda: lpips.conv5_device(p0, model), k * flops["conv5"])
            p1 = timed("lpips_maxpool_kernel", lambda: lpips.maxpool_device(t1))
            t2 = timed("elvis_conv2d 3x3", lambda: model.convs3[0](p1, act=3), k * flops["conv3_192_384"])
            t3 = timed("elvis_conv2d 3x3", lambda: model.convs3[1](t2, act=3), k * flops["conv3_384_256"])
            t4 = timed("elvis_conv2d 3x3", lambda: model.convs3[2](t3, act=3), k * flops["conv3_256_256"])
            feats.append([t0, t1, t2, t3, t4])
        out = torch.empty(k, dtype=torch.float64, device=dev)
        for tap in range(5):
            timed("lpips_distance_kernel + finish", lambda: lpips.distance_device(feats[0][tap].t, feats[1][tap].t, feats[0][tap].c,
                                                                                  model.lin[tap], out, tap > 0))
        torch.cuda.synchronize()
        agg = {}
        for name, work, start, stop in stages:
            ms, fl = agg.get(name, (0.0, 0.0))
            agg[name] = (ms + start.elapsed_time(stop), fl + (work or 0.0))
        return agg

    one_pass()
    runs = [one_pass() for _ in range(max(3, args.repeats // 4))]
    total = float(np.median([sum(v[0] for v in r.values()) for r in runs]))
    for name in runs[0]:
        ms = float(np.median([r[name][0] for r in runs]))
        fl = runs[0][name][1]
        extra = dict(tflops=round(fl / (ms * 1e-3) / 1e12, 2), fp32_peak_fraction=round(fl / (ms * 1e-3) / FP32_PEAK, 4)) if fl else {}
        report(call=name, clock="device events, one pass", pairs=k, ms_median=round(ms, 3), share=round(ms / total, 4), **extra)

    # ---- the evaluator, host to host
    yy, xx = np.mgrid[:h, :w]
    fgs = [((yy - 500 - 3 * i) ** 2 + (xx - 900 - 5 * i) ** 2) < 300 ** 2 for i in range(n)]
    few = max(2, args.repeats // 5)
    t_plain = host_ms(lambda: metrics.evaluate_fg_bg_metrics(refs, decs, fgs, device=dev), few)
    t_model = host_ms(lambda: metrics.evaluate_fg_bg_metrics(refs, decs, fgs, device=dev, lpips_model=model), few)
    report(call="evaluate_fg_bg_metrics", clock="host to host", frames=n, ms_median=round(t_plain[0], 2), ms_min=round(t_plain[1], 2))
    report(call="evaluate_fg_bg_metrics (lpips_model)", clock="host to host", frames=n, ms_median=round(t_model[0], 2), ms_min=round(t_model[1], 2),
           added_ms=round(t_model[0] - t_plain[0], 2))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=lines), f, indent=1)


if __name__ == "__main__":
    main()
