"""Time of FVMD on a 30-frame and a 300-frame 1080p pair of luma clips.

    python tools/fvmd_bench.py [--frames 30 300] [--repeats 5] [--ref-segments 1] [--kernel-stats FILE.csv] [--out FILE]

`fvmd_device` on two resident luma clips and its stages (pyramid, tracks, feature rows, Frechet distance): device events
around each call, median and minimum over the repeats after warm-up, profiler off.  Then what the tracker does per call,
counted from the shapes: bilinear samples (four loads each), float64 operations, and the rates they come to at the
measured time - against the float64 vector peak that says whether the kernel is bound by FP64 issue or by the gathers.
With `--kernel-stats`, the kernel times of a SEPARATE run under `rocprofv3 --kernel-trace --stats -- python
tools/fvmd_bench.py --ref-segments 0` with the same --frames and --repeats (its `*_kernel_stats.csv`) are joined in.
Last, the numpy float64 statement (tests/_fvmd_ref.py) tracking `--ref-segments` segments of the first clip on the host's
cores.  One JSON line per measurement.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from elvis_amd import fvmd, synth, vmaf  # noqa: E402
from elvis_amd.recompose import frames_to_device  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12        # MI355X data sheet, FLOP/s
SAMPLES_PER_LEVEL = 225 * (5 + 8)  # template and four gradient taps, then one sample per iteration
FLOPS_PER_SAMPLE = 24              # clamps, floor, fractions, three blends, the residual and two products, counted as issued


def device_ms(call, repeats: int, warmup: int = 1):
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


def kernel_stats(path: str):
    """Name -> (calls, total ns) of a rocprofv3 kernel stats file."""
    stats = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("Kernel_Name") or ""
            if "fvmd_" not in name:
                continue
            name = name[name.index("fvmd_"):].split("(")[0].strip()
            calls, total = int(float(row.get("Calls", 0))), float(row.get("TotalDurationNs", 0))
            have = stats.get(name, (0, 0.0))
            stats[name] = (have[0] + calls, have[1] + total)
    return stats


def make_pair(frames: int, dev):
    """Two luma clips [frames,1080,1920]: 30 synthetic frames, repeated with a growing shift so that every frame differs,
    and the same with noise of +-9."""
    h, w = 1080, 1920
    base = vmaf.luma_device(frames_to_device(list(synth.synth_clip(21, min(frames, 30), h, w)), dev), "bgr")
    ref = torch.cat([torch.roll(base, shifts=(k, 2 * k), dims=(1, 2)) for k in range((frames + 29) // 30)])[:frames].contiguous()
    gen = torch.Generator(device=dev).manual_seed(5)
    noise = torch.randint(-9, 10, ref.shape, generator=gen, device=dev, dtype=torch.int16)
    return ref, (ref.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[30, 300])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-segments", type=int, default=1)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fvmd_bench needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    cfg = fvmd.FvmdConfig()
    lines = []

    def report(**line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    first = None
    for frames in args.frames:
        ref, dec = make_pair(frames, dev)
        first = ref if first is None else first
        s = fvmd.clip_seq_len(frames)
        b = fvmd.segment_count(frames, s, cfg.segment_step)
        med, lo = device_ms(lambda: fvmd.fvmd_device(ref, dec, cfg), args.repeats)
        report(call="fvmd_device", clock="device events", frames=frames, height=1080, width=1920, seq_len=s, segments=b,
               ms_median=round(med, 3), ms_min=round(lo, 3), value=fvmd.fvmd_device(ref, dec, cfg))
        med_p, _ = device_ms(lambda: fvmd.pyramid_device(ref), args.repeats)
        med_t, lo_t = device_ms(lambda: fvmd.track_keypoints_device(ref, s, cfg), args.repeats)
        tracks = fvmd.track_keypoints_device(ref, s, cfg)
        med_h, _ = device_ms(lambda: fvmd.motion_features_device(tracks), args.repeats)
        rows_a, rows_b = fvmd.motion_features_device(tracks), fvmd.motion_features_device(fvmd.track_keypoints_device(dec, s, cfg))
        med_f, _ = device_ms(lambda: fvmd.frechet_distance_device(rows_a, rows_b), args.repeats)
        report(stage="pyramid_device (one clip)", frames=frames, ms_median=round(med_p, 3))
        report(stage="track_keypoints_device (one clip, its pyramid included)", frames=frames, ms_median=round(med_t, 3), ms_min=round(lo_t, 3))
        report(stage="motion_features_device (one clip)", frames=frames, ms_median=round(med_h, 4))
        report(stage="frechet_distance_device", frames=frames, rows=b, row_length=rows_a.shape[1], ms_median=round(med_f, 3))
        samples = b * 400 * (s - 1) * 3 * SAMPLES_PER_LEVEL
        track_s = max(med_t - med_p, 1e-6) * 1e-3
        report(kernel="fvmd_track_kernel", frames=frames, samples_per_call=samples, loads_per_call=4 * samples,
               fp64_ops_per_call=FLOPS_PER_SAMPLE * samples, samples_per_s=round(samples / track_s, 1),
               fp64_ops_per_s=round(FLOPS_PER_SAMPLE * samples / track_s, 1),
               fp64_vector_peak_fraction=round(FLOPS_PER_SAMPLE * samples / track_s / FP64_VECTOR_PEAK, 4))
        del ref, dec, tracks, rows_a, rows_b
    if args.kernel_stats:
        for name, (calls, total) in sorted(kernel_stats(args.kernel_stats).items()):
            report(kernel=name, traced_calls=calls, traced_total_ms=round(total * 1e-6, 3), traced_ms_per_call=round(total * 1e-6 / max(calls, 1), 4))
    if args.ref_segments > 0 and first is not None:
        import _fvmd_ref as R
        s = fvmd.clip_seq_len(first.shape[0])
        clip = first[:s + args.ref_segments - 1].cpu().numpy()
        t0 = time.perf_counter()
        want = R.track(clip, s, 1)
        host_s = time.perf_counter() - t0
        got = fvmd.track_keypoints_device(first[:s + args.ref_segments - 1].contiguous(), s, cfg).cpu().numpy()
        report(call="tests/_fvmd_ref.py track", clock="host", segments=args.ref_segments, seq_len=s, s_per_segment=round(host_s / args.ref_segments, 2),
               worst_device_minus_statement=float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, results=lines), f, indent=1)


if __name__ == "__main__":
    main()
