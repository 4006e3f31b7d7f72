#!/usr/bin/env python3
"""Device time of the foreground segmenter (csrc/segment.hip, elvis_amd/segment.py) on one MI355X.
    python tools/segment_bench.py [--frames 30] [--runs 7] [--json PATH]

The clip: `--frames` frames of 1080p from the scene generator of tests/_segment_ref.py (random 8 x 8 colour patches, the
camera panning (4, 8) pixels a frame, a 256 x 384 object moving (0, 8), noise +-2), resident on the device, the
segmenter's defaults.  Timed: `foreground_masks_device` on the whole clip (ten launches and a memset, the workspace
allocation included).  Device time by events over back-to-back calls in a window of at least 0.2 s, median of `--runs`
rounds after a warm-up, with the smallest and the largest round.  Also reported: the bytes the call has to move by its
own layout - the frames read once, the masks written once, every per-pixel intermediate of the workspace written once
and read once - and what that is over the measured time as a rate.  It is a count from the shapes, not a counter
reading.
No GPU: an error, not a fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _segment_ref as R  # noqa: E402
from elvis_amd import _lib as L  # noqa: E402
from elvis_amd.segment import Q, SegmentConfig, foreground_masks_device, workspace_layout  # noqa: E402

H, W = 1080, 1920


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


def bytes_moved(n, h, w, c, radius):
    """Frames in, masks out, and every per-pixel section of the workspace (red, M, S, Mn, Sn, F, pre, voted) written
    once and read once; re-reads that a cache serves (halos, the partner frame, the x 4 upsample) are not counted."""
    p = (h // Q) * (w // Q)
    frames, masks = n * h * w * c, n * h * w
    work = 2 * n * p * (3 * 2 + 2 + 2 + 1 + 1 + 1 + 1 + 1)
    return dict(frames=frames, masks=masks, workspace_traffic=work, total=frames + masks + work,
                workspace_bytes=workspace_layout(n, h, w, radius)["total"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")
    dev = L.resolve_device("cuda:0")
    frames, boxes = R.scene((4, 8), (0, 8), 2, n=a.frames, h=H, w=W, obj=(256, 384))
    cfg = SegmentConfig()
    with torch.cuda.device(dev):
        fd = torch.from_numpy(frames).to(dev)
        masks, det = foreground_masks_device(fd, details=True)
        share = float(masks.float().mean())
        shifts = det["shift"].cpu().tolist()
        row = measure(lambda: foreground_masks_device(fd), a.runs)
    moved = bytes_moved(a.frames, H, W, 3, cfg.radius)
    result = dict(frames=a.frames, height=H, width=W, config=vars(cfg), foreground_share=share, shifts=shifts[:3],
                  ms_per_frame=row["ms"] / a.frames, bytes=moved, bytes_per_second=moved["total"] / (row["ms"] * 1e-3), **row)
    print(f"foreground_masks_device {row['ms']:9.3f} ms a clip [{row['ms_min']:.3f}, {row['ms_max']:.3f}]  "
          f"{row['ms'] / a.frames:7.4f} ms a frame ({row['calls_per_round']} calls a round)", flush=True)
    print(f"foreground share {share:.3f}, shifts {shifts[:3]} ...; {moved['total'] / a.frames * 1e-6:.2f} MB a frame by the layout "
          f"({moved['frames'] / a.frames * 1e-6:.2f} MB of it the frame itself) = {moved['total'] / (row['ms'] * 1e-3) * 1e-12:.3f} TB/s; "
          f"workspace {moved['workspace_bytes'] * 1e-6:.1f} MB", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
