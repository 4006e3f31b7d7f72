"""Per-block rate allocation of the device JPEG writer (elvis_amd/jpeg_write.py `roi_levels=` / `roi_block_size=`,
csrc/jpeg_write.hip, csrc/jpeg_encode.h) stated on top of tests/_jpeg_write_ref.py: its planes, its FDCT, its entropy
coder and its header, and the intervals of tests/_jpeg_restart_ref.py; only the quantiser is another.  Importable
without a GPU.

The rule.  `levels` is uint8 [By, Bx] on a grid of B x B luma pixels, B a multiple of 8, By either max(1, h // B) or
ceil(h / B), Bx likewise; a level is 0..48 in HEVC QP units, scale16(L) = round(16 * 2^(L / 6)).  A DCT block of a
component whose samples are fx x fy luma pixels (1 x 1 for luma and gray, hmax x vmax for chroma) has the footprint x0 =
bx * 8 * fx .. x0 + 8 * fx - 1, y likewise, both ends clamped to the frame; a pixel's cell is min(p // B, Bx - 1), min(p
// B, By - 1); the block's level is the minimum over the cells its footprint touches, at most 48.  An AC coefficient
with FDCT output c (scaled by 8) and table entry Q is zeroed when 16 * |c| + (d >> 1) < d, d = scale16(level) * (Q <<
3), and is quantised as the writer always quantised it otherwise.  DC is never touched; a dummy block keeps its DC only.
`mutant=` switches on one named deviation.

    python tests/_jpeg_roi_ref.py dump FILE      writes every case of the corpus for tools/jpeg_roi_check.cpp
"""
from __future__ import annotations

import struct
import sys
from dataclasses import dataclass
from functools import lru_cache
from typing import List, Optional, Tuple

import numpy as np

if __name__ == "__main__":          # run as a script: the package lies beside tests/
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import _jpeg_ref as R
import _jpeg_restart_ref as S
import _jpeg_write_ref as W

MUTANTS = ("dc_zeroed_too", "top_left_cell", "max_not_min", "half_dropped", "chroma_footprint_in_chroma_pixels", "table_off_by_one",
           "cell_not_clamped")
MAX_LEVEL = 48
SIZES = ((33, 17), (53, 37), (16, 16), (64, 48), (52, 40), (24, 8))          # (w, h)
BLOCK_SIZES = (8, 16, 32)
GRIDS = ("floor", "ceil")
MAPS = ("zero", "all48", "random", "checker30", "corner")
QUALITIES = (95, 75, 50)
CONTENTS = ("noise", "ramp", "checker")


def scale16(level: int) -> int:
    """round(16 * 2^(level / 6)), half up, in exact integer arithmetic: the rounded value is the largest v with
    (2 v - 1)^6 <= 32^6 * 2^level."""
    v = int(16 * 2 ** (level / 6))
    while (2 * (v + 1) - 1) ** 6 <= 32 ** 6 * 2 ** level:
        v += 1
    while (2 * v - 1) ** 6 > 32 ** 6 * 2 ** level:
        v -= 1
    return v


def grid_dims(w: int, h: int, B: int, grid: str) -> Tuple[int, int]:
    """(By, Bx) of the floored or the full grid."""
    if grid == "floor":
        return max(1, h // B), max(1, w // B)
    return -(-h // B), -(-w // B)


def block_level(levels: np.ndarray, B: int, w: int, h: int, by: int, bx: int, fx: int, fy: int, mutant: Optional[str] = None) -> int:
    """The level of block (by, bx) of a component whose samples are fx x fy luma pixels."""
    By, Bx = levels.shape
    x0, y0 = bx * 8 * fx, by * 8 * fy
    x1, y1 = x0 + 8 * fx - 1, y0 + 8 * fy - 1
    x0, x1, y0, y1 = min(x0, w - 1), min(x1, w - 1), min(y0, h - 1), min(y1, h - 1)
    if mutant == "cell_not_clamped":           # an index past the grid wraps round
        cell = lambda p, n: (p // B) % n
    else:
        cell = lambda p, n: min(p // B, n - 1)
    if mutant == "top_left_cell":
        return min(int(levels[cell(y0, By), cell(x0, Bx)]), MAX_LEVEL)
    seen = [int(levels[cell(y, By), cell(x, Bx)]) for y in range(y0, y1 + 1) for x in range(x0, x1 + 1)]
    return min(max(seen) if mutant == "max_not_min" else min(seen), MAX_LEVEL)


def quantise_roi(coef: np.ndarray, table: np.ndarray, level: np.ndarray, mutant: Optional[str] = None) -> np.ndarray:
    """coef int64 [blocks, 8, 8] (scaled by 8), table [64] natural order, level int [blocks]."""
    if mutant == "table_off_by_one":
        level = np.minimum(level + 1, MAX_LEVEL)
    s16 = np.asarray([scale16(int(v)) for v in level], np.int64)
    q8 = table.reshape(8, 8).astype(np.int64) << 3
    d = s16[:, None, None] * q8[None]
    half = 0 if mutant == "half_dropped" else d >> 1
    dead = 16 * np.abs(coef) + half < d
    if mutant != "dc_zeroed_too":
        dead[:, 0, 0] = False
    return np.where(dead, 0, W.quantise(coef, table))


def quantised_blocks(frame: np.ndarray, quality: int, subsampling: str, order: str, levels: np.ndarray, B: int, mutant: Optional[str] = None):
    """tests/_jpeg_write_ref.py `quantised_blocks` with the quantiser of above: (blocks int64 [blocks, 64] in zigzag and
    MCU scan order, dummy flags, component of every block, the tables, the level of every block, -1 for a dummy)."""
    planes = W._planes(frame, order)
    h, w = planes[0].shape
    tables = W.quant_tables(quality)
    levels = np.asarray(levels)
    hmax, vmax = (1, 1) if len(planes) == 1 else W._FACTORS[subsampling]
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    grids = []
    for c, p in enumerate(planes):
        hs, vs = (hmax, vmax) if c == 0 else (1, 1)
        cw, ch = -(-w * hs // hmax), -(-h * vs // vmax)
        wib, hib = -(-cw // 8), -(-ch // 8)
        plane = W.component_plane(p, hmax // hs, vmax // vs, wib, hib)
        blk = plane.reshape(hib, 8, wib, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        fx, fy = (hmax // hs, vmax // vs)
        if mutant == "chroma_footprint_in_chroma_pixels":
            fx = fy = 1
        lev = np.asarray([block_level(levels, B, w, h, by, bx, fx, fy, mutant) for by in range(hib) for bx in range(wib)], np.int64)
        q = quantise_roi(W.fdct_blocks(blk), tables[min(c, 1)], lev, mutant).reshape(hib, wib, 64)[:, :, list(R.ZIGZAG)]
        grids.append((q, hs, vs, wib, hib, lev.reshape(hib, wib)))
    out, dummy, comp, used = [], [], [], []
    for my in range(mcuy):
        for mx in range(mcux):
            for c, (q, hs, vs, wib, hib, lev) in enumerate(grids):
                for vy in range(vs):
                    for hx in range(hs):
                        by, bx = my * vs + vy, mx * hs + hx
                        if by < hib and bx < wib:
                            out.append(q[by, bx])
                            used.append(int(lev[by, bx]))
                        else:
                            z = np.zeros(64, np.int64)
                            z[0] = out[-1][0]
                            out.append(z)
                            used.append(-1)
                        dummy.append(used[-1] < 0)
                        comp.append(c)
    return np.asarray(out), np.asarray(dummy), np.asarray(comp), (tables[:1] if len(planes) == 1 else tables), np.asarray(used)


@dataclass
class Encoded:
    data: bytes                 # the whole file
    scan: bytes                 # everything between SOS and EOI
    blocks: np.ndarray          # int16 [blocks, 64], zigzag, MCU scan order
    dummy: np.ndarray
    comp: np.ndarray
    block_levels: np.ndarray    # the level every block was quantised with, -1 for a dummy block
    ri: int


def encode(frame: np.ndarray, quality: int = 95, subsampling: str = "420", order: str = "rgb", levels=None, B: int = 8, restart_rows: int = 0,
           restart_mcus: int = 0, mutant: Optional[str] = None) -> Encoded:
    """One uint8 frame (H,W), (H,W,1) or (H,W,3) with its map uint8 [By, Bx] as a baseline JPEG file, with restart intervals
    where asked for."""
    a = np.asarray(frame)
    channels = 1 if a.ndim == 2 else a.shape[2]
    h, w = a.shape[:2]
    blocks, dummy, comp, tables, used = quantised_blocks(a, quality, subsampling, order, levels, B, mutant)
    mcux, mcuy, bpm = S.mcu_grid(w, h, channels, subsampling)
    mcus = mcux * mcuy
    ri = S.restart_interval(w, h, channels, subsampling, restart_rows, restart_mcus)
    step = ri if ri else mcus
    scan = bytearray()
    for s, m in enumerate(range(0, mcus, step)):
        if s:
            scan += bytes([0xFF, 0xD0 + ((s - 1) & 7)])
        scan += S._interval(blocks, comp, m * bpm, min(m + step, mcus) * bpm, bpm, None)[0]
    data = S.header(w, h, channels, subsampling, tables, ri) + bytes(scan) + b"\xff\xd9"
    return Encoded(data, bytes(scan), blocks.astype(np.int16), dummy, comp, used, ri)


# ----------------------------------------------------------------------------- the corpus
def make_map(kind: str, By: int, Bx: int, seed: int) -> np.ndarray:
    if kind == "zero":
        return np.zeros((By, Bx), np.uint8)
    if kind == "all48":
        return np.full((By, Bx), MAX_LEVEL, np.uint8)
    if kind == "random":
        return np.random.default_rng(seed).integers(0, MAX_LEVEL + 1, size=(By, Bx)).astype(np.uint8)
    if kind == "checker30":
        yy, xx = np.mgrid[0:By, 0:Bx]
        return (((yy + xx) & 1) * 30).astype(np.uint8)
    if kind == "corner":
        m = np.zeros((By, Bx), np.uint8)
        m[-1, -1] = 36
        return m
    raise ValueError(kind)


@dataclass(frozen=True)
class Case:
    name: str
    w: int
    h: int
    sampling: str              # "gray" | "444" | "422" | "420"
    quality: int
    kind: str
    seed: int
    B: int
    grid: str                  # "floor" | "ceil"
    map_kind: str

    @property
    def channels(self) -> int:
        return 1 if self.sampling == "gray" else 3

    @property
    def subsampling(self) -> str:
        return "420" if self.sampling == "gray" else self.sampling

    def frame(self) -> np.ndarray:
        """uint8 [h, w, channels], RGB."""
        return R.make_content(self.kind, self.h, self.w, self.channels, self.seed)

    def levels(self) -> np.ndarray:
        """uint8 [By, Bx]."""
        return make_map(self.map_kind, *grid_dims(self.w, self.h, self.B, self.grid), self.seed + 1)


@lru_cache(maxsize=None)
def cases() -> Tuple[Case, ...]:
    """Every size x sampling x map, with the block size, the grid, the quality and the content cycling so that every size
    meets every block size and both grids; noise is the content two times out of four."""
    out, k = [], 0
    for w, h in SIZES:
        for s in R.SAMPLINGS:
            for m in MAPS:
                B, grid = BLOCK_SIZES[k % 3], GRIDS[(k // 3) % 2]
                q, kind = QUALITIES[(k // 2) % 3], ("noise", "ramp", "noise", "checker")[k % 4]
                out.append(Case(f"w{w}-h{h}-{s}-q{q}-{kind}-b{B}{grid}-{m}", w, h, s, q, kind, 1100 + k, B, grid, m))
                k += 1
    return tuple(out)


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


@lru_cache(maxsize=None)
def encoded(name: str, order: str = "rgb") -> Encoded:
    """The statement's file for a case by name, computed once."""
    c = case(name)
    frame = c.frame()
    return encode(frame[:, :, ::-1] if order == "bgr" and c.channels == 3 else frame, c.quality, c.subsampling, order, c.levels(), c.B)


# ----------------------------------------------------------------------------- the quality search
def bisect_transcription(size_of, target, quality_max):
    """The search of `jpeg_write.jpeg_quality_for_bytes` transcribed: (quality, fits, the qualities probed in their order)."""
    probes = [1]
    if size_of(1) > target:
        return 1, False, probes
    lo, hi = 1, quality_max
    while lo < hi:
        mid = (lo + hi + 1) // 2
        probes.append(mid)
        if size_of(mid) <= target:
            lo = mid
        else:
            hi = mid - 1
    return lo, True, probes


def statement_sizes(frames, subsampling="420", **roi):
    """quality -> int64 [n]: the statement's file lengths, computed on demand."""
    cache = {}

    def sizes(q):
        if q not in cache:
            if roi:
                cache[q] = np.asarray([len(encode(f, q, subsampling, "bgr", lv, roi["B"]).data) for f, lv in zip(frames, roi["levels"])], np.int64)
            else:
                cache[q] = np.asarray([len(W.encode(f, q, subsampling, "bgr").data) for f in frames], np.int64)
        return cache[q]
    return sizes


# ----------------------------------------------------------------------------- the corpus for the host check
def dump(path: str) -> None:
    """Every case as tools/jpeg_roi_check.cpp reads it: the shape, the settings and the grid, the pixels (the channel
    orders alternate), the map, and the statement's quantised blocks."""
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases())))
        for k, c in enumerate(cases()):
            order = "bgr" if k % 2 and c.channels == 3 else "rgb"
            frame = c.frame()
            pixels = np.ascontiguousarray(frame[:, :, ::-1] if order == "bgr" else frame)
            e = encoded(c.name, order)
            levels = c.levels()
            fh.write(struct.pack("<I", len(c.name)) + c.name.encode())
            fh.write(struct.pack("<9I", c.h, c.w, c.channels, int(order == "bgr"), c.quality, W.SUBSAMPLINGS.index(c.subsampling), c.B, *levels.shape))
            for blob in (pixels.tobytes(), np.ascontiguousarray(levels).tobytes(), e.blocks.astype("<i2").tobytes()):
                fh.write(struct.pack("<I", len(blob)) + blob)
    print(f"{len(cases())} cases -> {path}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(__doc__)
