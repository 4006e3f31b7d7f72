"""numpy statement of the clip intake's two resizes (elvis_amd/intake.py, csrc/resize.hip) - what the GPU output is pinned
against, bit for bit.  Written from the rules, not from the kernel: no tiles, no chunks of rows, no LDS; every destination
value is its own sum over its table entries, in table order (the loops run over the position of an entry in its
destination's list, all destination values at once).

    resize_area_u8(frames, hd, wd, mutate=None)   cv2.resize(INTER_AREA) of [n,Hs,Ws,C] u8, OpenCV 4.x restated
    resize_nearest_u8(x, hd, wd)                  cv2.resize(INTER_NEAREST) of [n,Hs,Ws,C] or [n,Hs,Ws] u8

`mutate` changes one clause of the rule (MUTANTS); tests/test_resize_host.py shows that the GPU cases see each.
`cases()` and `frames()` are the inputs tests/test_gpu_resize.py runs.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np

MUTANTS = ("fma", "box2_everywhere", "half_up", "no_cutoff", "swap_axes_tables", "fast_when_one_axis_whole")
CHANNELS = (1, 3, 4)


def entries(src: int, dst: int, eps: float = 1e-3) -> List[Tuple[int, int, np.float32]]:
    """computeResizeAreaTab (OpenCV 4.x resize.cpp) for one axis: (destination, source, float32 weight) in order.  `eps`
    is the cut-off of its two partial cells (the `no_cutoff` mutant passes 0)."""
    scale = 1.0 / (dst / src)
    out = []
    for dx in range(dst):
        fsx1 = dx * scale
        fsx2 = fsx1 + scale
        cell_width = min(scale, src - fsx1)
        sx1 = math.ceil(fsx1)
        sx2 = min(math.floor(fsx2), src - 1)
        sx1 = min(sx1, sx2)
        if sx1 - fsx1 > eps:
            out.append((dx, sx1 - 1, np.float32((sx1 - fsx1) / cell_width)))
        for sx in range(sx1, sx2):
            out.append((dx, sx, np.float32(1.0 / cell_width)))
        if fsx2 - sx2 > eps:
            out.append((dx, sx2, np.float32(min(min(fsx2 - sx2, 1.0), cell_width) / cell_width)))
    return out


def _by_position(tab, dst: int, limit: int):
    """The entries of every destination index side by side: source index [dst, m], weight [dst, m], count [dst]."""
    lists = [[] for _ in range(dst)]
    for d, s, w in tab:
        lists[d].append((min(s, limit - 1), w))
    m = max(1, max(len(e) for e in lists))
    idx = np.zeros((dst, m), np.int64)
    wgt = np.zeros((dst, m), np.float32)
    for d, e in enumerate(lists):
        for k, (s, w) in enumerate(e):
            idx[d, k], wgt[d, k] = s, w
    return idx, wgt, np.array([len(e) for e in lists])


def _round(x: np.ndarray, mutate) -> np.ndarray:
    if mutate == "half_up":
        return np.floor(x.astype(np.float64) + 0.5).astype(np.int64)
    return np.rint(x).astype(np.int64)


def _box(x: np.ndarray, hd: int, wd: int, fy: int, fx: int, mutate) -> np.ndarray:
    n, hs, ws, c = x.shape
    s = np.zeros((n, hd, wd, c), np.int64)
    for k in range(fy):
        for j in range(fx):
            s += x[:, k:k + fy * hd:fy, j:j + fx * wd:fx].astype(np.int64)
    area = fx * fy
    if mutate == "box2_everywhere":
        return (s + area // 2) // area
    if area == 1:
        return s
    if fx == 2 and fy == 2:
        return (s + 2) >> 2
    return _round(s.astype(np.float32) * np.float32(1.0 / area), mutate)


def resize_area_u8(frames: np.ndarray, hd: int, wd: int, mutate: Optional[str] = None) -> np.ndarray:
    """cv2.resize(frame, (wd, hd), interpolation=cv2.INTER_AREA) of every frame of [n,Hs,Ws,C] u8, hd <= Hs, wd <= Ws.
    Both ratios whole: the box sum - itself at 1x1, (sum + 2) >> 2 at 2x2, otherwise rint(float32(sum) * float32(1.0 /
    area)).  Otherwise ResizeArea_<uchar, float> with a table per axis: per destination value and y entry (sy, beta),
    buf = 0, then buf = buf + S[sy][sx] * alpha over the x entries; sum = sum + beta * buf from 0; every product and every
    sum rounded to float32; rint, clipped to [0, 255]."""
    assert mutate is None or mutate in MUTANTS, mutate
    x = np.asarray(frames)
    assert x.dtype == np.uint8 and x.ndim == 4
    n, hs, ws, c = x.shape
    if hd > hs or wd > ws or hd < 1 or wd < 1:
        raise ValueError(f"resize_area_u8: {hs}x{ws} -> {hd}x{wd} is not a downscale")
    whole_y, whole_x = hs % hd == 0, ws % wd == 0
    if (whole_y and whole_x) or (mutate == "fast_when_one_axis_whole" and (whole_y or whole_x)):
        return np.clip(_box(x, hd, wd, hs // hd, ws // wd, mutate), 0, 255).astype(np.uint8)
    eps = 0.0 if mutate == "no_cutoff" else 1e-3
    xi, xw, xn = _by_position(entries(ws, wd, eps), wd, ws)
    if mutate == "swap_axes_tables":                       # the x table read for y: row min(dy, wd - 1) of it, inside the source
        pick = np.minimum(np.arange(hd), wd - 1)
        yi, yw, yn = np.minimum(xi[pick], hs - 1), xw[pick], xn[pick]
    else:
        yi, yw, yn = _by_position(entries(hs, hd, eps), hd, hs)
    src = x.astype(np.float32)
    total = np.zeros((n, hd, wd, c), np.float32)
    for k in range(yi.shape[1]):
        rows = src[:, yi[:, k]]                                                    # n, hd, ws, c: entry k's source row of every dy
        buf = np.zeros((n, hd, wd, c), np.float32)
        for j in range(xi.shape[1]):
            live = (xn > j)[None, None, :, None]
            alpha = xw[:, j][None, None, :, None]
            s = rows[:, :, xi[:, j]]
            if mutate == "fma":
                step = (buf.astype(np.float64) + s.astype(np.float64) * alpha.astype(np.float64)).astype(np.float32)
            else:
                step = buf + s * alpha
            buf = np.where(live, step, buf)
        live = (yn > k)[None, :, None, None]
        beta = yw[:, k][None, :, None, None]
        if mutate == "fma":
            step = (total.astype(np.float64) + beta.astype(np.float64) * buf.astype(np.float64)).astype(np.float32)
        else:
            step = total + beta * buf
        total = np.where(live, step, total)
    return np.clip(_round(total, mutate), 0, 255).astype(np.uint8)


def resize_nearest_u8(x: np.ndarray, hd: int, wd: int) -> np.ndarray:
    """cv2.resize(x, (wd, hd), interpolation=cv2.INTER_NEAREST) of [n,Hs,Ws,C] or [n,Hs,Ws]: destination index d reads
    source index floor(d * src / dst) on each axis, in integers."""
    x = np.asarray(x)
    hs, ws = x.shape[1:3]
    rows = [(d * hs) // hd for d in range(hd)]
    cols = [(d * ws) // wd for d in range(wd)]
    return x[:, rows][:, :, cols]


# ----------------------------------------------------------------------------- the cases of tests/test_gpu_resize.py
WHOLE = {"8x12->4x6": (8, 12, 4, 6), "9x12->3x4": (9, 12, 3, 4), "6x12->3x4": (6, 12, 3, 4), "5x7->5x7": (5, 7, 5, 7)}
FRACTIONAL = {"7x10->3x4": (7, 10, 3, 4), "5x7->5x3": (5, 7, 5, 3), "12x10->4x4": (12, 10, 4, 4), "3x3->1x1": (3, 3, 1, 1),
              "17x33->16x32": (17, 33, 16, 32), "63x79->8x10": (63, 79, 8, 10), "200x3->1x1": (200, 3, 1, 1),
              "1x1001->1x1000": (1, 1001, 1, 1000), "1500x1->1499x1": (1500, 1, 1499, 1)}
# where the kernel takes another path: one destination column's share of a source row fills the LDS chunk on its own (one
# row per chunk at C = 1) or does not fit it at all (C = 3, 4: the source is read in place), box rule and float rule; n = 1
STEEP = {"2x45000->1x1": (2, 45000, 1, 1), "2x90001->1x2": (2, 90001, 1, 2)}
# ... and where even one channel's share of a source row exceeds the LDS: the in-place kernels at C = 1 (run at C = 1 only)
STEEP_C1 = {"2x65600->1x1": (2, 65600, 1, 1), "2x131203->1x2": (2, 131203, 1, 2)}

# What elvis_last_launch reports after the two entry points, stated once: by (both ratios whole, the source is read in
# place: row_stride 0 of the plan).  csrc/resize.hip notes these very strings.
AREA_KERNELS = {(True, False): "resize_area_kernel<whole,lds>", (True, True): "resize_area_kernel<whole,direct>",
                (False, False): "resize_area_kernel<frac,lds>", (False, True): "resize_area_kernel<frac,direct>"}
NEAREST_KERNEL = "resize_nearest_kernel"


def area_kernel(hs: int, ws: int, hd: int, wd: int, c: int) -> str:
    """The instantiation `intake.resize_area_device` launches for this resize: the dispatch of elvis_resize_area_u8 on the
    plan's row_stride and the two ratios."""
    from elvis_amd.intake import _plan
    return AREA_KERNELS[(hs % hd == 0 and ws % wd == 0, _plan(hs, ws, hd, wd, c)[3] == 0)]


def tiling_cases(c: int) -> Dict[str, Tuple[int, int, int, int]]:
    """A destination of (2 th + 1) x (2 tw + 3) - two whole tiles and a remainder on both axes - from a source about 1.5x
    and about 2.5x as large, with (th, tw) the kernel's tile for that very resize (`intake.resize_area_plan`)."""
    from elvis_amd.intake import resize_area_plan
    out = {}
    for name, num, den in (("1.5", 3, 2), ("2.5", 5, 2)):
        th, tw, _ = resize_area_plan(4096, 4096, 2048, 2048, c)               # a first guess: the tile of a large frame
        for _ in range(4):
            hd, wd = 2 * th + 1, 2 * tw + 3
            hs, ws = hd * num // den + 1, wd * num // den + 2
            th2, tw2, _ = resize_area_plan(hs, ws, hd, wd, c)
            if (th2, tw2) == (th, tw):
                break
            th, tw = th2, tw2
        else:
            raise AssertionError("no fixed point of the tile plan")
        out[f"tiles{name}_c{c}"] = (hs, ws, hd, wd)
    return out


def cases(c: int) -> Dict[str, Tuple[int, int, int, int]]:
    return {**WHOLE, **FRACTIONAL, **STEEP, **(STEEP_C1 if c == 1 else {}), **tiling_cases(c)}


def frames(hs: int, ws: int, c: int, n: int, seed: int = 0) -> np.ndarray:
    """Seeded random bytes [n,hs,ws,c]; the last frame carries a 0 / 255 checkerboard in its upper left quarter and
    single-pixel impulses (255 on 0, 0 on 255) in its lower right one; its other two quarters stay random."""
    rng = np.random.default_rng([seed, hs, ws, c, n])
    x = rng.integers(0, 256, (n, hs, ws, c), dtype=np.uint8)
    f = x[-1]
    ch, cw = max(1, hs // 2), max(1, ws // 2)
    yy, xx = np.mgrid[:ch, :cw]
    f[:ch, :cw] = (((yy + xx) & 1) * 255).astype(np.uint8)[..., None]
    if hs > ch and ws > cw:
        q = f[ch:, cw:]
        qh, qw = q.shape[:2]
        q[:] = 0
        q[qh // 4, qw // 2] = 255
        if qh >= 2:
            q[qh // 2:] = 255
            q[qh // 2 + (qh - qh // 2) // 2, qw // 3] = 0
    return x
