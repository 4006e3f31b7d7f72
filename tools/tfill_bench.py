#!/usr/bin/env python3
"""Device time of the temporal fill (csrc/tfill.hip, elvis_amd/inpaint_temporal.py) on one MI355X.
    python tools/tfill_bench.py [--frames 30] [--runs 7] [--json PATH]

The clip: `--frames` frames of 1080p from the panning generator of tests/_tfill_ref.py (a textured scene moving (2, 3)
pixels a frame, N(0, 1) noise), 25 % of the 16 x 16 blocks removed at random in every frame, the fill's defaults.
Timed: `temporal_fill_device` (one launch a clip), and as context on the same input `inpaint_device` (the wavefront
Telea alone, with its one download) and `inpaint_temporal_device` (the fill, then Telea on what is left).  Device time
by events over back-to-back calls in a window of at least 0.2 s, median of `--runs` rounds after a warm-up, with the
smallest and the largest round.  Also reported: the share of the hole pixels the fill leaves, and the byte differences
it computes - counted from the shapes by the rule of the contract, every source of every block with a hole (the early
stop once a block is full is not counted, so the rate is an upper bound of the work done).
No GPU: an error, not a fallback."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _tfill_ref as R  # noqa: E402
from elvis_amd import _lib as L, inpaint  # noqa: E402
from elvis_amd.inpaint_temporal import DEFAULTS, inpaint_temporal_device, temporal_fill_device  # noqa: E402

H, W, B = 1080, 1920, 16


def _time(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def measure(fn, runs):
    fn()
    torch.cuda.synchronize()
    inner = max(1, min(200, int(200.0 / max(_time(fn, 1), 1e-3))))     # a window of about 0.2 s at least
    ts = [_time(fn, inner) for _ in range(runs)]
    return dict(ms=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), calls_per_round=inner)


def byte_differences(masks, p):
    """Channel differences the contract asks for: per block with a hole, per source inside the clip, (2S+1)^2
    displacements over the window's pixels, 3 channels."""
    n, h, w = masks.shape
    b, g, s = p["block"], p["margin"], p["search"]
    total = 0
    for t in range(n):
        sources = len(R.source_order(t, n, p["radius"]))
        for by in range(0, h, b):
            for bx in range(0, w, b):
                if masks[t, by:by + b, bx:bx + b].any():
                    wh = min(h, by + b + g) - max(0, by - g)
                    ww = min(w, bx + b + g) - max(0, bx - g)
                    total += sources * (2 * s + 1) ** 2 * wh * ww * 3
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")
    dev = L.resolve_device("cuda:0")
    noisy, _ = R.pan_clip(a.frames, H, W, 3, seed=0)
    masks = R.random_block_masks(a.frames, H, W, B, 0.25, seed=1)
    frames = R.holed(noisy, masks, value=0)
    p = dict(DEFAULTS)
    diffs = byte_differences(masks, p)
    with torch.cuda.device(dev):
        fd, md = torch.from_numpy(frames).to(dev), torch.from_numpy(masks).to(dev)
        out, left = temporal_fill_device(fd, md)
        holes, still = int((md != 0).sum()), int((left != 0).sum())
        work = torch.empty_like(fd)
        rows = dict(temporal_fill_device=measure(lambda: temporal_fill_device(fd, md), a.runs),
                    inpaint_device=measure(lambda: inpaint.inpaint_device(fd, md, out=work), a.runs),
                    inpaint_temporal_device=measure(lambda: inpaint_temporal_device(fd, md), a.runs))
    fill = rows["temporal_fill_device"]
    result = dict(frames=a.frames, height=H, width=W, block=B, removed=0.25, params=p, hole_pixels=holes, left_pixels=still,
                  left_share=still / max(holes, 1), byte_differences=diffs,
                  byte_differences_per_second=diffs / (fill["ms"] * 1e-3), ms_per_frame=fill["ms"] / a.frames, **rows)
    for name, r in rows.items():
        print(f"{name:26s} {r['ms']:9.3f} ms a clip [{r['ms_min']:.3f}, {r['ms_max']:.3f}]  {r['ms'] / a.frames:7.3f} ms a frame "
              f"({r['calls_per_round']} calls a round)", flush=True)
    print(f"holes {holes} pixels, {100.0 * still / max(holes, 1):.1f} % left to Telea; {diffs / a.frames * 1e-9:.2f} G byte differences a frame, "
          f"{diffs / (fill['ms'] * 1e-3) * 1e-12:.2f} T/s", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
