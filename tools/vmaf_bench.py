"""Time of the VMAF features on a 30-frame 1080p pair of luma clips.

    python tools/vmaf_bench.py [--frames 30] [--repeats 10] [--ref-frames 2] [--kernel-stats FILE.csv] [--out FILE]

`vmaf_features_device` on two resident luma clips: device events around the call, median and minimum over the repeats
after warm-up, profiler off, and the ms per frame pair.  Then the bytes every kernel moves per call, counted from the
shapes (what it must read and write once; halos and re-reads through the caches are not counted).  With
`--kernel-stats`, the kernel times of a SEPARATE run under `rocprofv3 --kernel-trace --stats -- python
tools/vmaf_bench.py --ref-frames 0` with the same --frames and --repeats (its `*_kernel_stats.csv`) are joined in: each
kernel's achieved bytes/s against the 6.29 TB/s measured copy rate.  Last, the numpy float64 statement (tests/_vmaf_ref.py) on the first
`--ref-frames` frames, on the host's cores.  One JSON line per measurement.
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

from elvis_amd import synth, vmaf  # noqa: E402
from elvis_amd.recompose import frames_to_device  # noqa: E402

COPY_RATE = 6.29e12


def kernel_bytes(n: int, h: int, w: int):
    """Bytes per call and kernel, from the shapes: n frame pairs of h x w."""
    out = {}
    vh, vw = h, w
    taps = (17, 9, 5, 3)
    for s in range(4):
        if s:
            src = 1 if s == 1 else 8
            out[f"vmaf_vif_down_kernel<{taps[s]}>"] = n * 2 * (vh * vw * src + (vh // 2) * (vw // 2) * 8)
            vh, vw = vh // 2, vw // 2
        out[f"vmaf_vif_stat_kernel<{taps[s]}>"] = n * 2 * vh * vw * (8 if s else 1)
    ah, aw = h, w
    dwt = {True: 0, False: 0}
    pool = 0
    for s in range(4):
        bh, bw = (ah + 1) // 2, (aw + 1) // 2
        dwt[s == 0] += n * 2 * (ah * aw * (8 if s else 1) + 4 * bh * bw * 8)
        pool += n * 6 * bh * bw * 8
        ah, aw = bh, bw
    out["vmaf_dwt_kernel<true>"], out["vmaf_dwt_kernel<false>"] = dwt[True], dwt[False]
    out["vmaf_adm_pool_kernel"] = pool
    out["vmaf_motion_kernel"] = n * 2 * h * w
    return out


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


def kernel_stats(path: str):
    """Name -> (calls, total ns) of a rocprofv3 kernel stats file; template arguments are kept, parameter lists dropped."""
    stats = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("Kernel_Name") or ""
            if "vmaf_" not in name:
                continue
            name = name[name.index("vmaf_"):].split("(")[0].replace("void ", "").strip()
            calls, total = int(float(row.get("Calls", 0))), float(row.get("TotalDurationNs", 0))
            have = stats.get(name, (0, 0.0))
            stats[name] = (have[0] + calls, have[1] + total)
    return stats


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--ref-frames", type=int, default=2)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vmaf_bench needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    h, w, n = 1080, 1920, args.frames
    refs = list(synth.synth_clip(21, n, h, w))
    rng = np.random.default_rng(5)
    decs = [np.clip(f.astype(np.int16) + rng.integers(-9, 10, f.shape), 0, 255).astype(np.uint8) for f in refs]
    ref_y = vmaf.luma_device(frames_to_device(refs, dev), "bgr")
    dis_y = vmaf.luma_device(frames_to_device(decs, dev), "bgr")
    lines = []

    def report(**line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    calls = args.repeats + 3                                           # warm-up 2, the repeats, and the one that feeds the score
    med, lo = device_ms(lambda: vmaf.vmaf_features_device(ref_y, dis_y), args.repeats)
    report(call="vmaf_features_device", clock="device events", frames=n, height=h, width=w, ms_median=round(med, 3), ms_min=round(lo, 3),
           ms_per_pair=round(med / n, 3))
    model = vmaf.get_vmaf_model(None, dev)
    feats = vmaf.vmaf_features_device(ref_y, dis_y)
    med_p, lo_p = device_ms(lambda: vmaf.vmaf_predict_device(feats, model), args.repeats)
    report(call="vmaf_predict_device", clock="device events", frames=n, ms_median=round(med_p, 4), ms_min=round(lo_p, 4))
    by_kernel = kernel_bytes(n, h, w)
    stats = kernel_stats(args.kernel_stats) if args.kernel_stats else {}
    for name, nbytes in by_kernel.items():
        line = dict(kernel=name, bytes_per_call=nbytes)
        if name in stats and stats[name][1] > 0:
            per_call_s = stats[name][1] * 1e-9 / calls                  # the traced run made the same `calls` calls
            line.update(ms_per_call=round(per_call_s * 1e3, 3), bytes_per_s=round(nbytes / per_call_s, 1),
                        copy_rate_fraction=round(nbytes / per_call_s / COPY_RATE, 4))
        report(**line)
    if args.ref_frames > 0:
        import _vmaf_ref as R
        k = min(n, args.ref_frames)
        a, b = ref_y[:k].cpu().numpy(), dis_y[:k].cpu().numpy()
        t0 = time.perf_counter()
        want = R.features(a, b)
        host_s = time.perf_counter() - t0
        got = feats[:k].cpu().numpy()
        got[k - 1, 1] = vmaf.vmaf_features_device(ref_y[:k], dis_y[:k])[k - 1, 1].item()          # the statement saw k frames only
        report(call="tests/_vmaf_ref.py features", clock="host", frames=k, ms_per_pair=round(host_s * 1e3 / k, 1),
               worst_device_minus_statement=float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), calls_of_vmaf_features_device=calls, results=lines), f, indent=1)


if __name__ == "__main__":
    main()
