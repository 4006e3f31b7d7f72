"""Device time of Presley's two degrade kernels on a 30-frame 1080p clip, with the one-thread-per-block kernels of
`filter_frame_downsample` / `filter_frame_gaussian` on the same maps as context.

    python tools/degrade_bench.py [--frames 30] [--repeats 20] [--out FILE]

Per block size (8, 16): the scale kernel on Presley's default map (`degrade_adaptive_downsample`, max_scale 4: scales
0, 2, 3, 4), the Gaussian kernel on max_rounds 4 and 10.  The old kernels take whole-block frames, power-of-two scales
and blocks <= 16, so the old-against-new lines run on the clip cropped to whole blocks, the scale comparison on a map of
scales 0, 2, 4 only; both outputs are compared before anything is timed (equal for the scale pair; the Gaussian pair
differs by design: float32 against cv2's fixed point).  Times are device events around one launch, after warm-up, the
two kernels of a pair alternating; median and minimum over the repeats, one JSON line per measurement.  A clip is
read once and written once: `gbps` is 2 x clip bytes over the median.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from elvis_amd import degrade as D, synth  # noqa: E402


def time_alternating(calls, repeats: int, warmup: int = 3):
    """[(median ms, min ms)] of each zero-argument call, run in turn `repeats` times."""
    for _ in range(warmup):
        for call in calls:
            call()
    torch.cuda.synchronize()
    times = [[] for _ in calls]
    for _ in range(repeats):
        for k, call in enumerate(calls):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            call()
            stop.record()
            stop.synchronize()
            times[k].append(start.elapsed_time(stop))
    return [(float(np.median(t)), float(np.min(t))) for t in times]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("degrade_bench needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    h, w = 1080, 1920
    clip = torch.from_numpy(synth.synth_clip(11, args.frames, h, w)).to(dev)
    lines = []

    def report(name, block, frames_d, med_min, **extra):
        med, best = med_min
        line = dict(kernel=name, block=block, frames=int(frames_d.shape[0]), height=int(frames_d.shape[1]), width=int(frames_d.shape[2]),
                    ms_median=round(med, 4), ms_min=round(best, 4), gbps=round(2 * frames_d.numel() / med / 1e6, 1), **extra)
        lines.append(line)
        print(json.dumps(line), flush=True)

    rng = np.random.default_rng(12)
    for b in (8, 16):
        by, bx = h // b, w // b
        importance = rng.random((args.frames, by, bx))
        to_dev = lambda m: torch.from_numpy(np.ascontiguousarray(m.astype(np.int32))).to(dev)
        scales = to_dev(D._scale_map(importance, 4))
        rounds4 = to_dev(D.generate_degradation_map(importance, 4))
        rounds10 = to_dev(D.generate_degradation_map(importance, 10))
        pow2 = to_dev(np.where(D._scale_map(importance, 3) == 3, 4, D._scale_map(importance, 3)))        # scales 0, 2, 4
        levels = to_dev(np.log2(np.maximum(pow2.cpu().numpy(), 1)))
        out = torch.empty_like(clip)
        out.copy_(clip)
        t = time_alternating([lambda: D.degrade_scale_device(clip, scales, b, out=out),
                              lambda: D.degrade_gaussian_fx_device(clip, rounds4, b, out=out),
                              lambda: D.degrade_gaussian_fx_device(clip, rounds10, b, out=out)], args.repeats)
        report("degrade_scale", b, clip, t[0], map="max_scale 4")
        report("degrade_gaussian_fx", b, clip, t[1], map="max_rounds 4")
        report("degrade_gaussian_fx", b, clip, t[2], map="max_rounds 10")
        whole = clip[:, :by * b].contiguous()
        out_new, out_old = torch.empty_like(whole), torch.empty_like(whole)
        assert torch.equal(D.degrade_scale_device(whole, pow2, b), D.degrade_downsample_device(whole, levels, b))
        t = time_alternating([lambda: D.degrade_scale_device(whole, pow2, b, out=out_new),
                              lambda: D.degrade_downsample_device(whole, levels, b, out=out_old)], args.repeats)
        report("degrade_scale", b, whole, t[0], map="scales 0 2 4")
        report("degrade_downsample (old)", b, whole, t[1], map="scales 0 2 4")
        for name, rounds in (("max_rounds 4", rounds4), ("max_rounds 10", rounds10)):
            fx, f32 = D.degrade_gaussian_fx_device(whole, rounds, b), D.degrade_gaussian_device(whole, rounds, b)
            differ = float((fx != f32).float().mean())
            t = time_alternating([lambda: D.degrade_gaussian_fx_device(whole, rounds, b, out=out_new),
                                  lambda: D.degrade_gaussian_device(whole, rounds, b, out=out_old)], args.repeats)
            report("degrade_gaussian_fx", b, whole, t[0], map=name)
            report("degrade_gaussian (old, float32)", b, whole, t[1], map=name, pixels_differing_from_fx=round(differ, 4))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=lines), f, indent=1)


if __name__ == "__main__":
    main()
