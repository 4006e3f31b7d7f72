"""The case matrix for the ten kernels of csrc/classical.hip, csrc/degrade.hip and csrc/shrink.hip (importable without a
GPU: tests/test_gpu_block_matrix.py runs the cases on the device, tests/test_block_ledger.py checks the ledger, the
branch coverage of the case list, the pins and the discrimination of the inputs on the CPU).

Every comparison is on integers and bit-exact.  The expected outputs come from the three references that already
exist and are already pinned - tests/_classical_ref.py, oracle/degrade_ref.py, tests/_shrink_ref.py - with one thin
wrap where a reference lacks a contract the kernel documents in include/elvis_amd.h (the Gaussian's rounds are clamped
to 32 there; the oracle does not clamp).  The `*_ref` functions below restate the same operations with a `mutant`
hook, for the discrimination test only: with mutant=None each equals the existing reference on every case (pinned by
the ledger), with a mutant it is a plausible wrong kernel.

NaN scores are outside the matrix: the frame-level wrappers reject them and the kernels' behaviour on them is not
defined."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import _classical_ref as C
import _shrink_ref as S
from _glueref import first_difference, kernel_stems, kernel_symbols  # noqa: F401  (re-exported for the tests)
from elvis_amd.classical import MAX_LEVEL, gaussian_taps_u8, lanczos_taps
from oracle import degrade_ref as D

F32, I64 = np.float32, np.int64
GATHER_CAP_ITEMS = 256 * 32 * 256          # the launch code's grid limit times the 256 lanes: above it the loop strides
GAUSS_MAX_ROUNDS = 32                      # elvis_degrade_gaussian_u8's documented clamp
DCT_LEVELS = 4                             # elvis_amd.degrade.DCT_LEVELS
SOURCES = ("classical.hip", "degrade.hip", "shrink.hip")

KERNEL = {"gather": "block_gather_u8_kernel", "topk": "shrink_select_topk_kernel", "passes": "shrink_select_passes_kernel",
          "stretch": "stretch_index_kernel", "lanczos": "classical_lanczos_kernel", "unsharp": "classical_unsharp_kernel",
          "blend": "temporal_blend_kernel", "downsample": "degrade_downsample_kernel", "gaussian": "degrade_gaussian_kernel",
          "dct": "degrade_dct_kernel"}
OPS = tuple(KERNEL)


# ============================================================================================ shared pieces
def border_index(i, n: int, mode: str = "reflect101"):
    """cv::borderInterpolate over an index array, reflecting as often as needed: reflect101 (gfedcb|abcdefgh|gfedcba),
    and the two wrong ones the mutants use - replicate (aaaaaa|abcdefgh|hhhhhhh) and reflect (fedcba|abcdefgh|hgfedcb)."""
    i = np.asarray(i, I64)
    if n == 1:
        return np.zeros_like(i)
    if mode == "replicate":
        return np.clip(i, 0, n - 1)
    if mode == "reflect":
        j = np.mod(i, 2 * n)
        return np.where(j >= n, 2 * n - 1 - j, j)
    p = 2 * (n - 1)
    j = np.mod(i, p)
    return np.where(j >= n, p - j, j)


def _border_mode(mutant):
    return mutant if mutant in ("replicate", "reflect") else "reflect101"


def area_small(sums, fac: int, mutant: Optional[str] = None):
    """cv::resizeAreaFast_ on u8 sums: (s + 2) >> 2 at factor 2, else rint(s * (1.f / area)) in float32 (exact for these
    power-of-two areas, so round half to even).  Mutants: `half_up`, `fac2_float` (factor 2 by the float rule)."""
    area = fac * fac
    if mutant == "half_up":
        v = (sums + area // 2) // area
    elif fac == 2 and mutant != "fac2_float":
        v = (sums + 2) >> 2
    else:
        v = np.rint(sums.astype(F32) * F32(1.0 / area)).astype(I64)
    return np.minimum(v, 255)


TIE_Q = (0, 1, 2, 3, 100, 101, 127, 128, 253, 254)


def tie_sums(f: int):
    """The 30 block sums q area + area / 2 + d for the quotients of TIE_Q (even and odd) and d in -1, 0, +1."""
    area = f * f
    return [q * area + area // 2 + d for q in TIE_Q for d in (-1, 0, 1)]


def tie_sum_image(f: int, c: int, seed: int = 0, block: Optional[int] = None):
    """[1, 5 f, 6 f, c] u8 (tiled up to whole `block`s) whose f x f cells sum to tie_sums(f), channel ch rotated by 7 ch:
    the exact ties of the INTER_AREA division with an even and with an odd quotient, and their two neighbours.  A
    cell's sum k is spread as k // f^2 everywhere and + 1 on k % f^2 positions chosen by a seeded shuffle (the
    construction of _glueref.every_sum_image; every sum of a 32 x 32 cell would take 261 121 cells)."""
    ks = np.asarray(tie_sums(f))
    area = f * f
    rng = np.random.default_rng(seed)
    k = ks[(np.arange(30)[:, None] + 7 * np.arange(c)[None, :]) % 30]
    base, rem = k // area, k % area
    order = rng.permuted(np.tile(np.arange(area), (30, c, 1)), axis=2)
    px = base[..., None] + (order < rem[..., None])
    img = px.reshape(5, 6, c, f, f).transpose(0, 3, 1, 4, 2).reshape(1, 5 * f, 6 * f, c)
    assert img.max() <= 255 and img.min() >= 0
    if block and block != f:
        img = np.tile(img, (1, block // math.gcd(5 * f, block), block // math.gcd(6 * f, block), 1))
    return img.astype(np.uint8)


def level_map(levels, n: int, by: int, bx: int):
    """int32 [n, by, bx]: the values of `levels` in order, cycled, frame f started 3 f further: every value occurs in
    every frame once the grid has as many cells as there are values (the ledger asserts which values the cases reach),
    and the frames' maps differ."""
    i = np.arange(by * bx)[None, :] + 3 * np.arange(n)[:, None]
    return np.asarray(levels, np.int32)[i % len(levels)].reshape(n, by, bx)


def content(kind: str, shape, rng):
    n, h, w, c = shape
    if kind == "flat0":
        return np.zeros(shape, np.uint8)
    if kind == "flat255":
        return np.full(shape, 255, np.uint8)
    if kind == "checker":       # 0 / 255 per pixel
        y, x = np.mgrid[0:h, 0:w]
        return np.broadcast_to((((y + x) & 1) * 255).astype(np.uint8)[None, :, :, None], shape).copy()
    if kind == "step":          # 0 | 255 at an odd column, so that the edge falls inside the blocks
        img = np.zeros(shape, np.uint8)
        img[:, :, (w // 2) | 1:] = 255
        return img
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    raise ValueError(kind)


# ============================================================================================ shrink references
def topk_ref(scores, k: int, *, mutant: Optional[str] = None):
    """S.topk_select with hooks.  Mutants: `tie_higher` (the higher column first among equals), `beat_le` (beat <= k:
    one column too many goes)."""
    scores = np.asarray(scores, np.float64)
    by, bx = scores.shape
    kk = min(k + 1, bx) if mutant == "beat_le" else k
    mask = np.zeros((by, bx), np.int8)
    for r in range(by):
        order = sorted(range(bx), key=lambda i: (-scores[r, i], -i if mutant == "tie_higher" else i))
        mask[r, order[:kk]] = 1
    keep = np.stack([np.flatnonzero(mask[r] == 0) for r in range(by)])
    return mask, (keep + np.arange(by)[:, None] * bx).astype(np.int32)


def passes_ref(scores, target: int, rows_only: bool, *, mutant: Optional[str] = None):
    """S.passes_select with hooks; also returns the trace [(axis, line length, lines visited)] of the passes.  Mutants:
    `argmin_last` (the last of equal minima), `rows_keep_width` (the rows-only form shortens the rows after a whole pass
    only, as the row-and-column form does)."""
    sc = np.array(scores, np.float64)
    by, bx = sc.shape
    origin = np.arange(by * bx).reshape(by, bx)
    mask = np.zeros(by * bx, bool)
    live, removed, passes, trace, axis = [by, bx], 0, [], [], 0
    while removed < target and live[0] > 0 and live[1] > 0 and not (rows_only and live[1] <= 1):
        s, o = (sc, origin) if axis == 0 else (sc.T, origin.T)
        n_lines, length = (live[0], live[1]) if axis == 0 else (live[1], live[0])
        hit = []
        for line in range(min(n_lines, target - removed)):
            v = s[line, :length]
            i = int(length - 1 - np.argmin(v[::-1])) if mutant == "argmin_last" else int(np.argmin(v))
            mask[o[line, i]] = True
            s[line, i:length - 1] = s[line, i + 1:length].copy()
            o[line, i:length - 1] = o[line, i + 1:length].copy()
            hit.append(i)
        removed += len(hit)
        trace.append((axis, length, len(hit)))
        whole = len(hit) == n_lines
        if axis == 0 and ((rows_only and mutant != "rows_keep_width") or whole):
            live[1] -= 1
        if axis == 1 and whole:
            live[0] -= 1
        passes.append(np.array(hit, np.int32))
        if not rows_only:
            axis ^= 1
    return mask.reshape(by, bx), origin[:live[0], :live[1]].astype(np.int32), passes, trace


def stretch_ref(mask, sgrid, mode: str, *, mutant: Optional[str] = None):
    """S.flat_rank_src_of / S.row_rank_src_of with hooks.  Mutants: `limit_off_by_one` (rank <= limit), `polarity`."""
    kept = (np.asarray(mask) != 0) if mutant == "polarity" else (np.asarray(mask) == 0)
    extra = 1 if mutant == "limit_off_by_one" else 0
    if mode == "flat":
        rank = np.cumsum(kept.ravel()) - 1
        ok = kept.ravel() & (rank < sgrid[0] * sgrid[1] + extra)
        return np.where(ok, rank, -1).reshape(kept.shape).astype(np.int32)
    rank = np.cumsum(kept, axis=1) - 1
    rows = np.arange(kept.shape[0])[:, None]
    ok = kept & (rank < np.where(rows < sgrid[0], sgrid[1] + extra, 0))
    return np.where(ok, rows * sgrid[1] + rank, -1).astype(np.int32)


def gather_ref(frames, src_of, block: int, sgrid, *, mutant: Optional[str] = None):
    """S.gather_blocks + S.fullres_mask per frame.  Mutants: `hole_fill` (a hole is filled with 1), `polarity` (the mask
    is 255 on the kept blocks)."""
    n, c = src_of.shape[0], frames.shape[3]
    nsrc = sgrid[0] * sgrid[1]
    holes = np.where((src_of < 0) | (src_of >= nsrc), -1, src_of)
    if nsrc == 0:
        out = np.zeros((n, src_of.shape[1] * block, src_of.shape[2] * block, c), np.uint8)
    else:
        out = np.stack([S.gather_blocks(frames[f], src_of[f], block, sgrid) for f in range(n)])
    mask = np.stack([S.fullres_mask(holes[f], block) for f in range(n)])
    if mutant == "hole_fill":
        out[mask == 255] = 1
    if mutant == "polarity":
        mask = (255 - mask).astype(np.uint8)
    return out, mask


def gather_launch(seg: int, pitch: int, off_src: int, off_dst: int) -> str:
    """widest_vector restated, for bases that are 16-byte aligned before the offsets."""
    for v in (16, 8, 4):
        if seg % v == 0 and pitch % v == 0 and (off_src | off_dst) % v == 0:
            return f"block_gather_u8_kernel<{v}>"
    return "block_gather_u8_kernel<1>"


# ============================================================================================ classical references
def lanczos_ref(frames, levels, b: int, *, mutant: Optional[str] = None):
    """C.lanczos_restore with hooks.  Mutants: `half_up`, `fac2_float` (area_small), `border_reflect` (REFLECT_101 in
    place of BORDER_REPLICATE), `no_round` ((v) >> 22 without the 2^21), `lo` (a negative level counts as its size)."""
    lv = np.abs(levels.astype(I64)) if mutant == "lo" else levels.astype(I64)
    lv = np.clip(lv, 0, MAX_LEVEL)
    blocks = C._blocks(frames, levels, b)
    res = blocks.copy()
    lb = int(np.log2(b))
    for level in np.unique(lv[lv > 0]):
        sel = lv == level
        blk = blocks[sel].astype(I64)
        nb, c = blk.shape[0], blk.shape[-1]
        lf = min(int(level), lb)
        fac, s = 1 << lf, b >> lf
        small = area_small(blk.reshape(nb, s, fac, s, fac, c).sum(axis=(2, 4)), fac, mutant)
        first, taps = lanczos_taps(fac, b)
        raw = first[:, None] + np.arange(8)
        idx = border_index(raw, s) if mutant == "border_reflect" else np.clip(raw, 0, s - 1)
        t = taps.astype(I64)
        hp = (small[:, :, idx, :] * t[None, None, :, :, None]).sum(axis=3)
        v = (hp[:, idx, :, :] * t[None, :, :, None, None]).sum(axis=2)
        res[sel] = np.clip((v + (0 if mutant == "no_round" else 1 << 21)) >> 22, 0, 255).astype(np.uint8)
    return C._unblocks(frames.copy(), res)


def unsharp_ref(frames, levels, b: int, halo: int = 0, *, mutant: Optional[str] = None):
    """C.unsharp_restore block by block, with hooks.  Mutants: `tie_odd` (a tie of the final halving goes to the odd
    neighbour), `halo_short` (the tile grows by halo - 1), `replicate` / `reflect` (the blur's border), `hi` (a level
    above 16 is not clamped), `lo` (a negative level counts as its size)."""
    n, h, w, c = frames.shape
    lv = np.abs(levels.astype(I64)) if mutant == "lo" else levels.astype(I64)
    lv = np.maximum(lv, 0) if mutant == "hi" else np.clip(lv, 0, MAX_LEVEL)
    hl = max(halo - 1, 0) if mutant == "halo_short" else halo
    mode = _border_mode(mutant)
    out = frames.copy()
    ar = np.arange(b)[:, None]
    for f, i, j in np.argwhere(lv > 0):
        L = int(lv[f, i, j])
        y0, x0 = i * b, j * b
        ty0, tx0 = max(0, y0 - hl), max(0, x0 - hl)
        tile = frames[f, ty0:min(h, y0 + b + hl), tx0:min(w, x0 + b + hl)].astype(I64)
        th, tw = tile.shape[:2]
        taps = gaussian_taps_u8(L).astype(I64)
        kk = np.arange(6 * L + 1) - 3 * L
        cols = border_index((x0 - tx0) + ar + kk, tw, mode)                      # [b, taps]
        hp = (tile[:, cols, :] * taps[None, None, :, None]).sum(axis=2)           # [th, b, c]
        rows = border_index((y0 - ty0) + ar + kk, th, mode)
        acc = (hp[rows] * taps[None, :, None, None]).sum(axis=1)                  # [b, b, c]
        blur = (acc + 0x8000) >> 16
        x = tile[y0 - ty0:y0 - ty0 + b, x0 - tx0:x0 - tx0 + b]
        v2 = (2 + L) * x - L * blur
        q = v2 >> 1
        q = q + ((v2 & 1) & ((~q if mutant == "tie_odd" else q) & 1))
        out[f, y0:y0 + b, x0:x0 + b] = np.clip(q, 0, 255).astype(np.uint8)
    return out


def blend_ref(frames, tb: float, *, mutant: Optional[str] = None):
    """C.temporal_blend with a hook.  Mutant: `round` (to nearest in place of the truncation)."""
    out = frames.copy()
    for f in range(1, len(frames)):
        v = tb * out[f - 1] + (1 - tb) * frames[f]
        out[f] = (np.rint(v) if mutant == "round" else v).astype(np.uint8)
    return out


# ============================================================================================ degrade references
def _down_block(block, level: int, mutant):
    b = block.shape[0]
    fac = 1 << min(max(level, 0), 4)
    if fac <= 1:
        return block.copy()
    s = b // fac
    if s < 1:
        s, fac = 1, b
    small = area_small(block.reshape(s, fac, s, fac, -1).astype(I64).sum(axis=(1, 3)), fac, mutant)
    coef = [D._linear_coef(d, s, b) for d in range(b)]
    out = np.empty_like(block)
    for y in range(b):
        y0, b0, b1 = coef[y]
        y1 = min(y0 + 1, s - 1)
        for x in range(b):
            x0, a0, a1 = coef[x]
            x1 = min(x0 + 1, s - 1)
            r0 = small[y0, x0] * a0 + small[y0, x1] * a1
            r1 = small[y1, x0] * a0 + small[y1, x1] * a1
            out[y, x] = np.clip((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2, 0, 255).astype(np.uint8)
    return out


def downsample_ref(frames, levels, b: int, *, mutant: Optional[str] = None):
    """D.degrade_downsample over a clip, with hooks.  Levels are clamped to [0, 4].  Mutants: `half_up`, `fac2_float`,
    `lo` (a negative level counts as its size), `hi` (no upper clamp: the shift takes the level modulo 32, as the
    hardware does - level 32 then copies the block.  Levels 5 .. 31 cannot tell: with blocks of at most 16 every factor
    above the block averages the whole block, clamped or not)."""
    lv = levels.astype(I64)
    if mutant == "lo":
        lv = np.abs(lv)
    if mutant == "hi":
        lv = np.where(lv > 4, lv & 31, lv)
    out = frames.copy()
    for f, i, j in np.argwhere(lv > 0):
        sl = (f, slice(i * b, (i + 1) * b), slice(j * b, (j + 1) * b))
        out[sl] = _down_block(frames[sl], int(lv[f, i, j]), mutant)
    return out


def gaussian_ref(frames, rounds, b: int, *, mutant: Optional[str] = None):
    """D.degrade_gaussian over a clip with the kernel's clamp of the rounds to [0, 32], with hooks.  A block that a
    round leaves unchanged is a fixed point, so the remaining rounds are skipped.  Mutants: `replicate` / `reflect`
    (the border), `hi` (no clamp at 32), `lo` (a negative count counts as its size)."""
    r = np.abs(rounds.astype(I64)) if mutant == "lo" else rounds.astype(I64)
    r = np.maximum(r, 0) if mutant == "hi" else np.clip(r, 0, GAUSS_MAX_ROUNDS)
    k0, k1, k2 = D.gaussian_taps()
    kk = [k0, k1, k2, k1, k0]
    idx = border_index(np.arange(b)[:, None] + np.arange(5) - 2, b, _border_mode(mutant))     # [b, 5]
    out = frames.copy()
    for f, i, j in np.argwhere(r > 0):
        sl = (f, slice(i * b, (i + 1) * b), slice(j * b, (j + 1) * b))
        cur = frames[sl].copy()
        for _ in range(int(r[f, i, j])):
            x = cur.astype(F32)
            tmp = np.zeros_like(x)
            for d in range(5):
                tmp = tmp + kk[d] * x[:, idx[:, d]]
            acc = np.zeros_like(x)
            for d in range(5):
                acc = acc + kk[d] * tmp[idx[:, d], :]
            new = np.clip(np.rint(acc), 0, 255).astype(np.uint8)
            if np.array_equal(new, cur):
                break
            cur = new
        out[sl] = cur
    return out


def gaussian_expected(frames, rounds, b: int):
    """The wrap of the oracle: elvis_degrade_gaussian_u8 clamps the rounds to [0, 32], oracle.degrade_ref does not."""
    r = np.clip(rounds, 0, GAUSS_MAX_ROUNDS)
    return np.stack([D.degrade_gaussian(frames[f], r[f], b) for f in range(frames.shape[0])])


def dct_ref(frames, levels, *, mutant: Optional[str] = None):
    """D.dct_dampen over a clip.  Levels are clamped to [0, DCT_LEVELS).  Mutants: `hi` (the gain of the level itself),
    `lo` (a negative level counts as its size)."""
    lv = np.abs(levels) if mutant == "lo" else levels
    n_levels = int(max(lv.max() + 1, DCT_LEVELS)) if mutant == "hi" else DCT_LEVELS
    return np.stack([D.dct_dampen(frames[f], lv[f], n_levels) for f in range(frames.shape[0])])


# ============================================================================================ cases
@dataclass
class Case:
    id: str
    op: str
    shape: Tuple[int, ...] = ()           # the frames [n, h, w, c]; () for the selection kernels, which see no frames
    block: int = 1
    grid: Tuple[int, ...] = ()            # [n, by, bx] of the scores / mask / level map
    kind: str = ""                        # the inputs' recipe
    levels: Tuple[int, ...] = ()          # the map's values (level_map)
    k: int = 0                            # topk
    target: int = 0                       # passes
    mode: str = ""                        # passes: rows | rows_cols; stretch: flat | rows
    ridx: bool = True                     # passes: removal_idx given (False: NULL)
    sgrid: Tuple[int, int] = (0, 0)       # stretch: the shrunk grid; gather: the source grid
    dgrid: Tuple[int, int] = (0, 0)       # gather: the destination grid
    offs: Tuple[int, int, int] = (0, 0, 0)    # gather: byte offsets of the src, dst and mask bases from 16-byte alignment
    launch: str = ""                      # gather: what elvis_last_launch reports
    halo: int = 0
    tb: float = 0.0
    alias: bool = False                   # blend: out is cur
    big: bool = False
    seed: int = 0

    @property
    def kernel(self):
        return KERNEL[self.op]


LINE_LENGTHS = (1, 2, 63, 64, 65, 66, 128, 129, 130)
TOPK_BX = (1, 2, 255, 256, 257, 600)
TOPK_KINDS = ("random", "equal", "ties", "zeros", "inf")
STRETCH_LENGTHS = (1, 255, 256, 257, 513, 1000)
STRETCH_KINDS = ("all_kept", "all_removed", "surplus", "short_rows", "bytes")
GATHER_WIDTHS = ((64, 96, 16, 3), (64, 96, 16, 1), (40, 104, 8, 3), (40, 104, 8, 1), (36, 60, 4, 3), (35, 55, 5, 3),
                 (21, 33, 3, 1), (28, 49, 7, 3), (67, 99, 16, 3), (12, 20, 1, 3))
GATHER_OFFSETS = ((1, 0, 0), (4, 0, 0), (8, 0, 0), (0, 1, 0), (0, 4, 0), (0, 8, 0), (0, 0, 1), (0, 0, 4), (0, 0, 8), (8, 4, 1))
CLASSICAL_C = (1, 2, 3, 4)
CLASSICAL_B = (2, 4, 8, 16, 32)
HALOS = (0, 1, 3, 32)
TBS = (0.0, 0.3, 0.5, 0.7, 1.0)
DEGRADE_TOTALS = {63: ((1, 7, 9, 1), (3, 7, 1, 3)), 64: ((1, 8, 8, 1), (1, 4, 4, 4)), 65: ((1, 5, 13, 1),)}   # n, by, bx, c
DOWN_B = (1, 2, 4, 8, 16)
DOWN_LEVELS = (-1, 0, 1, 2, 3, 4, 5, 32, 100)
GAUSS_B = (1, 2, 3, 5, 8, 12, 16)
GAUSS_ROUNDS = (-3, 0, 1, 10, 32, 33, 1000)
DCT_MAP = (-1, 0, 1, 2, 3, 4, 9)
CONTENTS = ("flat0", "flat255", "checker", "noise")


def lanczos_levels(b: int):
    lb = int(np.log2(b))
    return tuple([-1] + list(range(0, lb + 2)) + [16, 17])


UNSHARP_LEVELS = tuple([-1, 0] + list(range(1, MAX_LEVEL + 2)))


def _topk_cases(add):
    j = 0
    for bx in TOPK_BX:
        for k in sorted({0, 1, bx - 1, bx}):
            for kind in TOPK_KINDS:
                by, n = ((1, 1), (3, 2), (1, 2), (3, 1))[j % 4]
                j += 1
                add(id=f"topk_{n}x{by}x{bx}_k{k}_{kind}", op="topk", grid=(n, by, bx), k=k, kind=kind)


def _passes_cases(add):
    P = lambda tag, grid, target, mode, kind="random", ridx=True: add(
        id=f"passes_{tag}_{'x'.join(map(str, grid))}_t{target}_{mode}" + ("" if ridx else "_noridx"), op="passes", grid=grid,
        target=target, mode=mode, kind=kind, ridx=ridx)
    # every target of the list, both modes, with and without the removal indices, on grids with more rows than waves
    for (by, bx) in ((17, 5), (33, 3)):
        for t in (0, 1, by, by + 1, by + bx - 1, by * bx - 1, by * bx):
            for mode in ("rows", "rows_cols"):
                P("target", (1, by, bx), t, mode)
        P("target", (1, by, bx), by + 1, "rows_cols", ridx=False)
        P("target", (1, by, bx), by + 1, "rows", ridx=False)
    P("target", (1, 15, 4), 31, "rows_cols")
    P("target", (1, 16, 4), 33, "rows")
    # deep sequences: every working line length from 130 down, as a row (both modes) and as a column
    P("deep", (1, 15, 130), 15 * 129, "rows")
    P("deep", (1, 16, 66), 16 * 66, "rows_cols", kind="ties")
    P("deep", (1, 130, 4), 130 * 4, "rows_cols")
    P("deep", (1, 66, 5), 66 * 5, "rows_cols", kind="ties")
    P("deep", (1, 2, 2), 4, "rows_cols")
    P("deep", (1, 1, 2), 2, "rows_cols")
    P("deep", (1, 2, 1), 2, "rows_cols")
    P("deep", (1, 1, 1), 1, "rows_cols")
    # rows-only with one column: the loop body must not run
    P("onecol", (1, 15, 1), 5, "rows")
    P("onecol", (2, 33, 1), 33, "rows", ridx=False)
    # where the minimum sits, and equal minima 64 and 1 apart: along the rows, and along the columns (kind *_cols: every
    # row holds its minimum in the last column, so the whole first row pass shifts nothing and drops that column, and
    # the whole column pass that follows sees the other columns as built)
    for L in (65, 129, 130):
        for kind in ("place", "tie64", "tie1"):
            P(kind, (1, 17, L), 17, "rows", kind=kind)
            P(kind, (1, 17, L), 17 * 2 + 3, "rows_cols", kind=kind)
            P(kind, (1, L, 17), L + 16, "rows_cols", kind=kind + "_cols")
    # three frames with different scores: the workspace and output offsets
    P("clip", (3, 17, 9), 17 * 3 + 4, "rows")
    P("clip", (3, 17, 9), 17 * 3 + 4, "rows_cols")
    P("clip", (3, 16, 130), 16 * 70, "rows", kind="ties")
    P("clip", (3, 5, 7), 11, "rows_cols", ridx=False)


def _stretch_cases(add):
    shapes = {1: (1, 1), 255: (15, 17), 256: (16, 16), 257: (1, 257), 513: (27, 19), 1000: (25, 40)}
    for L in STRETCH_LENGTHS:
        for kind in STRETCH_KINDS:
            for mode in ("flat", "rows"):
                by, bx = shapes[L] if mode == "flat" else (3, L)
                if kind == "surplus":
                    sg = (max(by // 2, 1), max(bx // 2, 1)) if mode == "flat" else (by, max(bx // 3, 1))
                    if mode == "flat" and by * bx == 1:
                        sg = (0, 1)
                elif kind == "short_rows":
                    sg = (by - 1, bx) if mode == "rows" else (max(by - 1, 0), bx)
                else:
                    sg = (by, bx)
                add(id=f"stretch_{mode}_len{L}_{kind}", op="stretch", grid=(2, by, bx), sgrid=sg, mode=mode, kind=kind)


def _gather_cases(add):
    for (h, w, b, c) in GATHER_WIDTHS:
        by, bx = h // b, w // b
        add(id=f"gather_{h}x{w}x{c}_b{b}", op="gather", shape=(2, h, w, c), block=b, sgrid=(by, bx), dgrid=(by + 1, max(1, bx - 2)),
            launch=gather_launch(b * c, w * c, 0, 0), kind="random")
    h, w, b, c = 64, 96, 16, 3
    for offs in GATHER_OFFSETS:
        add(id=f"gather_offsets_{offs[0]}_{offs[1]}_{offs[2]}", op="gather", shape=(2, h, w, c), block=b, sgrid=(4, 6), dgrid=(5, 4),
            offs=offs, launch=gather_launch(b * c, w * c, offs[0], offs[1]), kind="random")
    add(id="gather_no_source", op="gather", shape=(2, 0, 0, 3), block=8, sgrid=(0, 0), dgrid=(3, 5),
        launch=gather_launch(24, 0, 0, 0), kind="random")
    add(id="gather_over_cap_bytes_1x700x1100x3_b5", op="gather", shape=(1, 700, 1100, 3), block=5, sgrid=(140, 220),
        dgrid=(140, 220), launch="block_gather_u8_kernel<1>", kind="random", big=True)
    add(id="gather_over_cap_vec16_6x1072x1920x3_b16", op="gather", shape=(6, 1072, 1920, 3), block=16, sgrid=(67, 120),
        dgrid=(67, 120), launch="block_gather_u8_kernel<16>", kind="random", big=True)


def _lanczos_cases(add):
    for c in CLASSICAL_C:
        for b in CLASSICAL_B:
            add(id=f"lanczos_c{c}_b{b}", op="lanczos", shape=(2, 3 * b, 4 * b, c), block=b, grid=(2, 3, 4), levels=lanczos_levels(b),
                kind="noise")
    for f in (2, 4, 8, 16, 32):
        lf = int(np.log2(f))
        for b in sorted({f, 32}):
            shp = tie_sum_image(f, 3 if f < 32 else 1, f, b).shape
            add(id=f"lanczos_ties_f{f}_b{b}", op="lanczos", shape=shp, block=b, grid=(1, shp[1] // b, shp[2] // b), levels=(lf,),
                kind=f"ties{f}")
    for b, lv in ((8, 1), (16, 2), (32, 2), (32, 3)):
        for kind in ("small_step", "small_checker"):
            add(id=f"lanczos_{kind}_b{b}_l{lv}", op="lanczos", shape=(1, 2 * b, 3 * b, 3), block=b, grid=(1, 2, 3), levels=(lv,),
                kind=kind)


def _unsharp_cases(add):
    for ib, b in enumerate(CLASSICAL_B):
        for ih, halo in enumerate(HALOS):
            c = CLASSICAL_C[(ib + ih) % 4]
            add(id=f"unsharp_c{c}_b{b}_halo{halo}", op="unsharp", shape=(1, 4 * b, 5 * b, c), block=b, grid=(1, 4, 5),
                levels=UNSHARP_LEVELS, halo=halo, kind="noise")
    add(id="unsharp_reflect_many_b2_top_level", op="unsharp", shape=(2, 4, 6, 3), block=2, grid=(2, 2, 3), levels=(MAX_LEVEL,),
        halo=0, kind="noise")
    for halo in (0, 3):
        for (h, w, b) in ((37, 29, 8), (21, 35, 4)):        # the block does not divide the frame
            add(id=f"unsharp_ragged_{h}x{w}_b{b}_halo{halo}", op="unsharp", shape=(2, h, w, 3), block=b, grid=(2, h // b, w // b),
                levels=(3, 0, 1, 7, -2, 16, 2, 5), halo=halo, kind="noise")
    for kind in ("checker", "step", "noise"):               # ties and both saturations at the odd levels
        for halo in (0, 3):
            add(id=f"unsharp_odd_levels_{kind}_halo{halo}", op="unsharp", shape=(1, 16, 32, 3), block=8, grid=(1, 2, 4),
                levels=(1, 3, 5, 7, 9, 11, 13, 15), halo=halo, kind=kind)
    add(id="unsharp_largest_lds_96x96x4_b32_halo32", op="unsharp", shape=(1, 96, 96, 4), block=32, grid=(1, 3, 3),
        levels=(1, MAX_LEVEL, 9), halo=32, kind="noise", big=True)


def _blend_cases(add):
    for i, tb in enumerate(TBS):
        add(id=f"blend_pairs_tb{i}", op="blend", shape=(2, 256, 256, 1), tb=tb, kind="pairs")
        add(id=f"blend_five_frames_tb{i}", op="blend", shape=(5, 7, 9, 3), tb=tb, kind="noise")
        add(id=f"blend_one_frame_tb{i}", op="blend", shape=(1, 5, 5, 3), tb=tb, kind="noise")
        add(id=f"blend_in_place_tb{i}", op="blend", shape=(4, 9, 11, 3), tb=tb, kind="noise", alias=True)
        for shp in ((3, 1, 1, 1), (3, 5, 17, 3), (3, 16, 16, 1), (3, 257, 1, 1)):
            add(id=f"blend_{int(np.prod(shp[1:]))}px_tb{i}", op="blend", shape=shp, tb=tb, kind="noise")
    add(id="blend_pairs_in_place_tb0.3", op="blend", shape=(2, 256, 256, 1), tb=0.3, kind="pairs", alias=True)


def _grid_cases(add, op, b, levels, tag, kind="noise"):
    """The (n, c) and thread-total cases every degrade kernel shares: c in 1, 3, 4; n in 1, 3; totals 63 / 64 / 65."""
    for total, grids in DEGRADE_TOTALS.items():
        for (n, by, bx, c) in grids:
            assert n * by * bx * c == total
            add(id=f"{op}_{tag}_total{total}_n{n}_c{c}", op=op, shape=(n, by * b, bx * b, c), block=b, grid=(n, by, bx),
                levels=levels, kind=kind)
    add(id=f"{op}_{tag}_n3_c4", op=op, shape=(3, 3 * b, 4 * b, 4), block=b, grid=(3, 3, 4), levels=levels, kind=kind)


def _downsample_cases(add):
    _grid_cases(add, "downsample", 4, DOWN_LEVELS, "b4")
    for i, b in enumerate(DOWN_B):
        c, n = (1, 3, 4)[i % 3], (1, 3)[i % 2]
        add(id=f"downsample_b{b}_c{c}_n{n}", op="downsample", shape=(n, 3 * b, 3 * b, c), block=b, grid=(n, 3, 3), levels=DOWN_LEVELS,
            kind="noise")
        add(id=f"downsample_b{b}_checker", op="downsample", shape=(1, 3 * b, 3 * b, 3), block=b, grid=(1, 3, 3), levels=DOWN_LEVELS,
            kind="checker")
    for f in (2, 4, 8, 16):
        lf = int(np.log2(f))
        for b in sorted({f, 16}):
            shp = tie_sum_image(f, 3, f, b).shape
            add(id=f"downsample_ties_f{f}_b{b}", op="downsample", shape=shp, block=b, grid=(1, shp[1] // b, shp[2] // b),
                levels=(lf,), kind=f"ties{f}")


def _gaussian_cases(add):
    _grid_cases(add, "gaussian", 5, GAUSS_ROUNDS, "b5")
    j = 0
    for b in GAUSS_B:
        for kind in CONTENTS:
            c, n = (1, 3, 4)[j % 3], (1, 3)[j % 2]
            j += 1
            add(id=f"gaussian_b{b}_{kind}_c{c}_n{n}", op="gaussian", shape=(n, 2 * b, 4 * b, c), block=b, grid=(n, 2, 4),
                levels=GAUSS_ROUNDS, kind=kind)


def _dct_cases(add):
    _grid_cases(add, "dct", 8, DCT_MAP, "noise")
    for j, kind in enumerate(CONTENTS):
        c, n = (1, 3, 4)[j % 3], (1, 3)[j % 2]
        add(id=f"dct_{kind}_c{c}_n{n}", op="dct", shape=(n, 16, 32, c), block=8, grid=(n, 2, 4), levels=DCT_MAP, kind=kind)
        add(id=f"dct_{kind}_c3", op="dct", shape=(1, 24, 24, 3), block=8, grid=(1, 3, 3), levels=DCT_MAP, kind=kind)


def _build_cases():
    out = []
    add = lambda **kw: out.append(Case(**kw))
    for fn in (_topk_cases, _passes_cases, _stretch_cases, _gather_cases, _lanczos_cases, _unsharp_cases, _blend_cases,
               _downsample_cases, _gaussian_cases, _dct_cases):
        fn(add)
    for j, c in enumerate(out):
        c.seed = 500 + j
    return out


CASES = _build_cases()
BY_ID = {c.id: c for c in CASES}


# ============================================================================================ inputs (shared, read-only)
def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=8)
def _inputs_cached(case_id: str):
    return _make_inputs(BY_ID[case_id])


def inputs(case: Case):
    """The case's input arrays (read-only; built once per case, shared by the GPU test and the CPU checks)."""
    return _inputs_cached(case.id)


def _placed_scores(rng, lines: int, length: int, kind: str):
    """[lines, length] float64 in [1, 2) with, per line, the minimum 0 at index 0 / 63 / 64 / last in turn (`place`),
    two equal minima 64 apart (`tie64`) or next to each other (`tie1`), starting where the line number says."""
    s = rng.random((lines, length)) + 1.0
    for r in range(lines):
        if kind == "place":
            s[r, (0, 63, 64, length - 1)[r % 4]] = 0.0
        else:
            gap = 64 if kind == "tie64" else 1
            i = (0, length - 1 - gap, 63 if gap == 1 else (r * 7) % (length - gap), 62 if gap == 1 else 0)[r % 4]
            s[r, i] = s[r, i + gap] = 0.0
    return s


def _make_inputs(c: Case):
    rng = np.random.default_rng(c.seed)
    if c.op in ("topk", "passes"):
        n, by, bx = c.grid
        base = c.kind[:-5] if c.kind.endswith("_cols") else c.kind
        if base == "random":
            s = rng.random(c.grid)
        elif base == "equal":
            s = np.full(c.grid, 0.25)
        elif base == "ties":
            s = rng.integers(0, 4, c.grid).astype(np.float64)
        elif base == "zeros":
            s = np.where(rng.random(c.grid) < 0.5, 0.0, -0.0)
        elif base == "inf":
            s = rng.random(c.grid)
            u = rng.random(c.grid)
            s[u < 0.2] = np.inf
            s[u > 0.8] = -np.inf
        elif c.kind.endswith("_cols"):
            s = np.stack([np.concatenate([_placed_scores(rng, bx - 1, by, base).T, np.full((by, 1), -1.0)], axis=1) for _ in range(n)])
        else:
            s = np.stack([_placed_scores(rng, by, bx, base) for _ in range(n)])
        return _ro(np.ascontiguousarray(s, dtype=np.float64))
    if c.op == "stretch":
        n, by, bx = c.grid
        if c.kind == "all_kept":
            m = np.zeros(c.grid, np.uint8)
        elif c.kind == "all_removed":
            m = np.array([1, 2, 255], np.uint8)[rng.integers(0, 3, c.grid)]
        elif c.kind == "bytes":
            m = np.array([0, 1, 2, 255], np.uint8)[rng.integers(0, 4, c.grid)]
        else:
            m = (rng.random(c.grid) < 0.3).astype(np.uint8)
        return _ro(m)
    if c.op == "gather":
        frames = rng.integers(1, 256, c.shape, dtype=np.uint8)          # never 0: a hole is told from every block
        nsrc = c.sgrid[0] * c.sgrid[1]
        src_of = rng.integers(-3, nsrc + 2, (c.shape[0],) + c.dgrid).astype(np.int32)
        src_of[0, 0, 0], src_of[-1, -1, -1] = nsrc, -1                  # one index just beyond the source grid, one hole
        return _ro(frames, src_of)
    if c.op == "blend":
        if c.kind == "pairs":
            f = np.empty(c.shape, np.uint8)
            f[0, :, :, 0] = np.arange(256, dtype=np.uint8)[:, None]
            f[1, :, :, 0] = np.arange(256, dtype=np.uint8)[None, :]
            return _ro(f)
        return _ro(rng.integers(0, 256, c.shape, dtype=np.uint8))
    n, h, w, ch = c.shape
    m = level_map(c.levels, *c.grid)
    if c.kind.startswith("ties"):
        f = int(c.kind[4:])
        x = tie_sum_image(f, ch, f, c.block)
    elif c.kind.startswith("small_"):       # a 0 / 255 pattern in the small image: the Lanczos overshoot clips at both ends
        lf = c.levels[0]
        s, fac = c.block >> lf, 1 << lf
        yy, xx = np.mgrid[0:h // fac, 0:w // fac]
        p = ((yy + xx) & 1) if c.kind == "small_checker" else (xx % s >= s // 2).astype(int)
        x = np.broadcast_to(np.kron(p * 255, np.ones((fac, fac), int)).astype(np.uint8)[None, :, :, None], c.shape).copy()
    else:
        x = content(c.kind, c.shape, rng)
    assert x.shape == tuple(c.shape), (c.id, x.shape)
    return _ro(x, m)


# ============================================================================================ expected outputs
def passes_counts(c: Case):
    """The removals of every pass, from the restated plan (a function of the grid, the target and the mode alone)."""
    _, by, bx = c.grid
    return [t[2] for t in passes_ref(np.zeros((by, bx)), c.target, c.mode == "rows")[3]]


def passes_trace(c: Case):
    _, by, bx = c.grid
    return passes_ref(np.zeros((by, bx)), c.target, c.mode == "rows")[3]


def expected(c: Case, *, mutant: Optional[str] = None):
    """The reference outputs of a case as a tuple of arrays: from the existing references, or, for a mutant, from the
    hooked restatements above."""
    x = inputs(c)
    n = (c.grid or c.shape)[0]
    if c.op == "topk":
        per = [topk_ref(x[0][f], c.k, mutant=mutant) if mutant else S.topk_select(x[0][f], c.k) for f in range(n)]
        return np.stack([p[0] for p in per]), np.stack([p[1] for p in per])
    if c.op == "passes":
        rows_only = c.mode == "rows"
        per = [passes_ref(x[0][f], c.target, rows_only, mutant=mutant) if mutant else S.passes_select(x[0][f], c.target, rows_only)
               for f in range(n)]
        ridx = np.stack([np.concatenate(p[2]) if p[2] else np.zeros(0, np.int32) for p in per]).astype(np.int32)
        return np.stack([p[0] for p in per]).astype(np.uint8), np.stack([p[1] for p in per]), ridx
    if c.op == "stretch":
        if mutant:
            return (np.stack([stretch_ref(x[0][f], c.sgrid, c.mode, mutant=mutant) for f in range(n)]),)
        fn = S.flat_rank_src_of if c.mode == "flat" else S.row_rank_src_of
        return (np.stack([fn(x[0][f], c.sgrid) for f in range(n)]),)
    if c.op == "gather":
        return gather_ref(x[0], x[1], c.block, c.sgrid, mutant=mutant)
    if c.op == "blend":
        return (blend_ref(x[0], c.tb, mutant=mutant) if mutant else C.temporal_blend(x[0], c.tb),)
    frames, m = x
    if c.op == "lanczos":
        return (lanczos_ref(frames, m, c.block, mutant=mutant) if mutant else C.lanczos_restore(frames, m, c.block),)
    if c.op == "unsharp":
        return (unsharp_ref(frames, m, c.block, c.halo, mutant=mutant) if mutant else C.unsharp_restore(frames, m, c.block, c.halo),)
    if c.op == "downsample":
        if mutant:
            return (downsample_ref(frames, m, c.block, mutant=mutant),)
        return (np.stack([D.degrade_downsample(frames[f], m[f], c.block) for f in range(n)]),)
    if c.op == "gaussian":
        return (gaussian_ref(frames, m, c.block, mutant=mutant) if mutant else gaussian_expected(frames, m, c.block),)
    if c.op == "dct":
        return (dct_ref(frames, m, mutant=mutant),)
    raise ValueError(c.op)
