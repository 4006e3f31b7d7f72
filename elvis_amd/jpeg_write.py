"""JPEG frames written by the device (csrc/jpeg_write.hip, csrc/jpeg_encode.h): the reference writes frames through
`cv2.imwrite(path, frame)` and lets the suffix choose the format (`save_frame`, elvis.py:131-135; `save_frames(...,
pattern=)`, elvis.py:160-175), and every one of its loaders takes `.jpg` / `.jpeg` beside `.png`.  This is the device
path for those suffixes, the writer half of jpeg.py:

  encode_jpeg_device(frames_d)                 resident clip -> one complete baseline JPEG file (bytes) per frame
  save_jpeg_frames_device(frames_d, paths)     the same, written to `paths`
  save_jpeg_frames(frames, paths, device)      host arrays, uploaded in chunks of 32 MB
  jpeg_roundtrip_device(frames_d, quality)     encode, then jpeg.decode_jpeg_device: (decoded resident clip, bytes per frame)
  jpeg_quant_tables(quality)                   host: the two quantisation tables
  jpeg_file_header(width, height, ...)         host: everything in front of the entropy-coded bytes
  jpeg_restart_interval(width, height, ...)    host: the restart interval in MCUs that `restart_rows=` / `restart_mcus=` ask for
  jpeg_encoded_sizes_device(frames_d, quality) the length of every file `encode_jpeg_device` would return, without producing it
  jpeg_quality_for_bytes(frames_d, target)     the bisect over the quality for a byte budget of the whole clip
  jpeg_roundtrip_at_bytes_device(frames_d, t)  that search, then the round trip at the quality found
  jpeg_roi_levels(delta_qp), jpeg_roi_scale16  host: delta QPs to the levels of `roi_levels=`, and the table behind a level
  jpeg_optimal_tables(hist, channels)          host: symbol histograms to the optimal Huffman tables of `optimize=True`

Colour conversion, edge replication, chroma downsampling, the forward DCT, the quantiser, the Huffman coding, the bit
packing and the byte stuffing run as HIP kernels; the host plans the layout from two small downloads (a frame's bit
count, then its byte count), writes the headers and downloads the finished scans.  Pixels and coefficients never visit
the host.  The arithmetic is libjpeg's (jccolor.c, jcsample.c, jfdctint.c, jcdctmgr.c, jchuff.c with the Annex K tables,
one interleaved scan): against a libjpeg-turbo PIL at the same quality and sampling with `optimize=False`, the
quantisation tables, the SOF0 / SOS contents and the entropy-coded bytes are equal bit for bit;
tests/_jpeg_write_ref.py states them.  Equality of whole files is not claimed (the JFIF header's density fields are the
writer's own), and PARITY WITH cv2 IS UNPINNED: quality 95 and 4:2:0, the defaults here, are what `cv2.imwrite` asks its
libjpeg for, but no cv2 is at hand to compare with.  Opt-in: `frameio.save_frame` stays PIL, and the directory drivers
write `.jpg` names through PIL unless called with `jpeg_writer="device"`.

Restart intervals.  By default a file has none, as `cv2.imwrite` writes it, and its scan is one entropy-coded segment:
the device reader (jpeg.py) decodes a segment per lane, so such a frame keeps one lane busy.  `restart_rows=r` (libjpeg's
`restart_in_rows`: an interval of min(r * MCUs per row, 65535) MCUs) or `restart_mcus=k` (`restart_interval = k`) on
every form above cuts the scan into intervals: the header gets a DRI segment in front of SOS, every interval starts on a
byte boundary with the DC predictors at 0 and ends in the 1-fill, and RSTm markers (m = 0..7 in turn) stand between
them (jchuff.c `emit_restart`).  Turn it on - `restart_rows=1` - whenever the device reader will read the files: what
`jpeg_roundtrip_device` decodes itself, a directory the next driver loads with `png_reader="device"`.  It costs the
markers, the fill bits and the DC resets in bytes, and any decoder reads the files.  The kernels are the same: behind
the transform they work per (frame, interval) instead of per frame, an interval being what a frame is without them.
The bit-for-bit claim extends to it: against PIL with `restart_marker_rows=` / `restart_marker_blocks=` the DRI
segment's place and content and the entropy-coded bytes, markers included, are equal; tests/_jpeg_restart_ref.py
states the rule.

Per-block rate allocation.  `roi_levels=` (uint8 [n, By, Bx], a level 0..48 per cell of `roi_block_size` x `roi_block_size`
luma pixels) on every form above decides per DCT block which coefficients survive.  A level is in HEVC QP units - the
step doubles every 6 - and comes from the same importance scores the reference turns into ROI files for its encoders
(`handoff.roi_levels_from_importance`).  It is A DEAD ZONE, NOT A RE-QUANTISATION: an AC coefficient that the file's
quantiser coarsened by the block's level would round to zero is zeroed, every other coefficient keeps the file's own
quantiser, DC is never touched, and the file keeps the tables of its header - baseline JPEG that any decoder reads.
(Quantising with a coarser step m * Q and writing k * m does not work with the Annex K Huffman tables: every surviving
coefficient pays log2 m more magnitude bits, which is what the coarser step saved.)  With scale16(L) = round(16 *
2^(L / 6)), a table of 49 integers, a = |c| of the FDCT's output and d = scale16(L) * (Q << 3), the coefficient is zeroed
when 16 * a + (d >> 1) < d; level 0 is the writer without a map for every input.  A block's level is the minimum over
the cells its footprint touches (8 x 8 luma pixels for a luma block, 8 hmax x 8 vmax for a chroma block, clamped to the
frame; cell indices clamped to the grid, which is the floored h // B x w // B or the full one).  Bytes are not monotone
in the level: a zeroed coefficient can turn two short symbols into a longer run.  tests/_jpeg_roi_ref.py states the
rule.  `jpeg_quality_for_bytes` finds the quality for a byte budget from the pack call's sizes alone.

Optimised Huffman tables.  `optimize=True` on every form above (the default, False, changes nothing: the same bytes, the
same buffers, the same launches) is libjpeg's `optimize_coding`, per frame: the device counts the symbols the frame's
scan will hold - DC difference categories and AC (run, category) symbols with ZRL and EOB, per table class, over exactly
the blocks the scan codes, dummy blocks included, predictors reset at every restart interval, coefficients behind the
ROI dead zone - into a histogram u32 [n, 2, 272] in the layout of the code tables (`jpeg_bits_kernel` in its tally mode,
an LDS histogram a workgroup); the histograms come down (2 KB a frame, THE THIRD SYNCHRONISATION OF A CLIP, in front of
the other two); the library's host entry point `elvis_jpeg_optimal_tables` restates `jpeg_gen_optimal_table` of jchuff.c
(csrc/jpeg_encode.h) and returns every frame's DHT contents and code words; the words go up, [n, 2, 272], and the bit
count and the pack kernel take frame f's tables at a stride.  Every file gets a header of its own, its tables in the
four (gray: two) DHT segments where the Annex K ones stand otherwise.  Any baseline decoder reads the files, the device
reader included.  A frame's bytes depend on that frame alone.  Against a libjpeg-turbo PIL with `optimize=True` the DHT
segments, their position and everything behind SOS are equal byte for byte, restart intervals included;
tests/_jpeg_opt_ref.py states the rule.
"""
from __future__ import annotations

import os
import struct
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib, ptr
from .jpeg import ZIGZAG
from .ops import _s

SUBSAMPLINGS = ("444", "422", "420")
_FACTORS = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}
SCAN_CHUNK_BLOCKS = 256         # ELVIS_JPEG_SCAN_CHUNK: values of one step of the device prefix sums
STUFF_CHUNK_BYTES = 1024        # ELVIS_JPEG_STUFF_CHUNK: stream bytes of one workgroup of the stuffing pass
HUFF_WORDS = 272                # per table class: 16 DC entries by category, 256 AC entries by symbol
MAX_BLOCKS = 1 << 20            # blocks of a frame
MAX_FRAMES = 65535              # frames of one launch
MAX_SEGMENTS = 1 << 24          # ELVIS_JPEG_MAX_SEGMENTS: (frame, restart interval) pairs of one launch
UPLOAD_CHUNK_BYTES = 32 << 20
JPEG_ROI_MAX_LEVEL = 48         # JPGE_ROI_MAX_LEVEL: levels are HEVC QP units, the step doubles every 6
# round(16 * 2^(L / 6)) for L = 0..48, as csrc/jpeg_encode.h `jpeg_roi_scale16` has it
ROI_SCALE16 = (16, 18, 20, 23, 25, 29, 32, 36, 40, 45, 51, 57, 64, 72, 81, 91, 102, 114, 128, 144, 161, 181, 203, 228, 256, 287, 323, 362, 406,
               456, 512, 575, 645, 724, 813, 912, 1024, 1149, 1290, 1448, 1625, 1825, 2048, 2299, 2580, 2896, 3251, 3649, 4096)
# ITU-T T.81 Annex K.1, K.2: the quantisation tables in natural order
BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
             80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
             95, 98, 112, 100, 103, 99)
BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99) + (99,) * 36
# Annex K.3: the Huffman tables as (codes of each length 1..16, symbols in code order)
STD_DC = (((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
          ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))))
STD_AC = (((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125),
           (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
            0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
            0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
            0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
            0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
            0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
            0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
            0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA)),
          ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119),
           (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
            0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25,
            0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47,
            0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74,
            0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
            0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA,
            0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4,
            0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA)))
_JFIF = b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"       # version 1.1, no units, aspect 1:1, no thumbnail


# ----------------------------------------------------------------------------- the host's part
def _check_quality(quality, who: str) -> int:
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError(f"{who}: quality must be an integer in 1..100, got {quality!r}")
    return int(quality)


def _check_subsampling(subsampling, who: str) -> int:
    if not isinstance(subsampling, str) or subsampling not in SUBSAMPLINGS:
        raise ValueError(f"{who}: subsampling must be one of {SUBSAMPLINGS}, got {subsampling!r}")
    return SUBSAMPLINGS.index(subsampling)


def _check_restart(restart_rows, restart_mcus, who: str) -> Tuple[int, int]:
    for name, v in (("restart_rows", restart_rows), ("restart_mcus", restart_mcus)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 0:
            raise ValueError(f"{who}: {name} must be a non-negative integer, got {v!r}")
    if restart_rows and restart_mcus:
        raise ValueError(f"{who}: restart_rows={restart_rows} and restart_mcus={restart_mcus}: give one of them")
    if int(restart_mcus) > 65535:
        raise ValueError(f"{who}: restart_mcus must be in 1..65535 (0: no interval), got {restart_mcus}")
    return int(restart_rows), int(restart_mcus)


def _check_optimize(optimize, who: str) -> bool:
    if not isinstance(optimize, (bool, np.bool_)):
        raise ValueError(f"{who}: optimize must be a bool, got {optimize!r}")
    return bool(optimize)


def jpeg_restart_interval(width: int, height: int, channels: int = 3, subsampling: str = "420", restart_rows: int = 0,
                          restart_mcus: int = 0) -> int:
    """Host only: the restart interval in MCUs of a width x height frame, 0 for none.  `restart_mcus=k`, 1..65535, is
    libjpeg's `restart_interval = k`; `restart_rows=r` is its `restart_in_rows`: min(r * MCUs per row, 65535), an MCU
    being 8 x 8 pixels of a gray frame and 8 * hmax x 8 * vmax of a colour one.  Giving both is a ValueError."""
    who = "jpeg_restart_interval"
    rows, mcus = _check_restart(restart_rows, restart_mcus, who)
    _check_subsampling(subsampling, who)
    if isinstance(channels, bool) or channels not in (1, 3):
        raise ValueError(f"{who}: channels must be 1 or 3, got {channels!r}")
    if not 1 <= int(width) <= 65535 or not 1 <= int(height) <= 65535:
        raise ValueError(f"{who}: width and height must be in 1..65535, got {width} x {height}")
    if mcus:
        return mcus
    hmax = _FACTORS[subsampling][0] if channels == 3 else 1
    return min(rows * -(-int(width) // (8 * hmax)), 65535)


def jpeg_roi_scale16(level: int) -> int:
    """Host only: 16 times the factor by which ROI level `level` (0..48, HEVC QP units) coarsens the step that decides
    whether a coefficient survives: round(16 * 2^(level / 6)), from the table the kernel has."""
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 0 <= int(level) <= JPEG_ROI_MAX_LEVEL:
        raise ValueError(f"jpeg_roi_scale16: level must be an integer in 0..{JPEG_ROI_MAX_LEVEL}, got {level!r}")
    return ROI_SCALE16[int(level)]


def jpeg_roi_levels(delta_qp, floor=None) -> np.ndarray:
    """Host only: delta QPs (an integer array of any shape, as `handoff.kvazaar_delta_qp` gives them) to the levels
    `roi_levels=` takes: uint8 clip(delta_qp - floor, 0, 48).  `floor` is the delta QP that stands for the file's own
    quality, by default the array's minimum; a float dtype or a floor above the minimum is a ValueError."""
    a = np.asarray(delta_qp)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"jpeg_roi_levels: delta_qp must be an integer array, got {a.dtype}")
    low = int(a.min()) if a.size else 0
    if floor is None:
        floor = low
    if isinstance(floor, bool) or not isinstance(floor, (int, np.integer)):
        raise ValueError(f"jpeg_roi_levels: floor must be an integer, got {floor!r}")
    if a.size and int(floor) > low:
        raise ValueError(f"jpeg_roi_levels: floor {int(floor)} is above the smallest delta QP, {low}")
    return np.clip(a.astype(np.int64) - int(floor), 0, JPEG_ROI_MAX_LEVEL).astype(np.uint8)


def _check_roi(roi_levels, roi_block_size, n: int, h: int, w: int, who: str):
    """The checks of `roi_levels=` / `roi_block_size=` that need no device: None without a map, else (the map - a host
    array, or a tensor that is resident - and its By, Bx, B)."""
    b = roi_block_size
    if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or int(b) < 0:
        raise ValueError(f"{who}: roi_block_size must be a non-negative integer, got {b!r}")
    b = int(b)
    if roi_levels is None:
        if b:
            raise ValueError(f"{who}: roi_block_size={b} without roi_levels")
        return None
    if isinstance(roi_levels, torch.Tensor):
        levels = roi_levels if roi_levels.is_cuda else roi_levels.numpy()
    else:
        levels = np.asarray(roi_levels)
    if levels.dtype != (torch.uint8 if isinstance(levels, torch.Tensor) else np.uint8):
        raise ValueError(f"{who}: roi_levels must be uint8, got {levels.dtype}")
    if b < 8 or b % 8:
        raise ValueError(f"{who}: roi_block_size must be a positive multiple of 8, got {b}")
    if levels.ndim != 3 or int(levels.shape[0]) != n:
        raise ValueError(f"{who}: roi_levels must be [n, By, Bx] with n = {n}, got {tuple(levels.shape)}")
    by, bx = int(levels.shape[1]), int(levels.shape[2])
    if by not in (max(1, h // b), -(-h // b)) or bx not in (max(1, w // b), -(-w // b)):
        raise ValueError(f"{who}: roi_levels of {by} x {bx} cells are not the grid of a {h} x {w} frame in blocks of {b}: "
                         f"{max(1, h // b)} or {-(-h // b)} rows, {max(1, w // b)} or {-(-w // b)} columns")
    if n and int(levels.max()) > JPEG_ROI_MAX_LEVEL:
        raise ValueError(f"{who}: roi_levels holds {int(levels.max())}, above {JPEG_ROI_MAX_LEVEL}")
    return levels, by, bx, b


def jpeg_quant_tables(quality: int = 95) -> Tuple[np.ndarray, np.ndarray]:
    """Host only: (luma, chroma) quantisation tables, uint16 [64] in natural order, as libjpeg's
    `jpeg_set_quality(quality, force_baseline=TRUE)` scales the Annex K tables: (base * scale + 50) // 100 clamped to
    1..255, scale = 5000 // quality below 50 and 200 - 2 * quality from there."""
    q = _check_quality(quality, "jpeg_quant_tables")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.asarray(base, np.int64) * scale + 50) // 100, 1, 255).astype(np.uint16) for base in (BASE_LUMA, BASE_CHROMA))


def huffman_codes(counts: Sequence[int], values: Sequence[int]) -> Dict[int, Tuple[int, int]]:
    """symbol -> (code, length) of a (16 counts, values) table (T.81 C.2)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[values[k]] = (code, length)
            k += 1
            code += 1
        code <<= 1
    return out


def encode_tables() -> np.ndarray:
    """What the kernels look up: uint32 [2, 272], per table class (0 luma, 1 chroma) 16 DC entries by category and 256 AC
    entries by symbol, (code << 5) | length; 0 where the table has no such symbol."""
    tab = np.zeros((2, HUFF_WORDS), np.uint32)
    for t in range(2):
        for sym, (code, length) in huffman_codes(*STD_DC[t]).items():
            tab[t, sym] = code << 5 | length
        for sym, (code, length) in huffman_codes(*STD_AC[t]).items():
            tab[t, 16 + sym] = code << 5 | length
    return tab


def jpeg_optimal_tables(hist, channels: int = 3):
    """Host only (the library's `elvis_jpeg_optimal_tables`, no device): symbol histograms, uint32 [n, 2, 272] or [2, 272]
    in the layout of `encode_tables` - per table class 16 DC entries by category, 256 AC entries by symbol - to the
    optimal length-limited tables of libjpeg's `jpeg_gen_optimal_table`.  Returns (tables, ehuff): `tables` is a list
    with one tuple per frame, ((counts, symbols) for DC 0, AC 0 and, for `channels` 3, DC 1, AC 1) as
    `jpeg_file_header(huffman=)` takes it, counts a tuple of 16 and symbols the symbol values in code order; `ehuff` is
    uint32 [n, 2, 272], (code << 5) | length, class 1 all zero for a gray clip.  A [2, 272] histogram gives one frame's
    tuple and [2, 272].  ValueError for a table without a symbol or a count above 2^26."""
    who = "jpeg_optimal_tables"
    if isinstance(channels, bool) or channels not in (1, 3):
        raise ValueError(f"{who}: channels must be 1 or 3, got {channels!r}")
    a = np.asarray(hist)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{who}: hist must be an integer array, got {a.dtype}")
    single = a.ndim == 2
    if a.ndim not in (2, 3) or a.shape[-2:] != (2, HUFF_WORDS):
        raise ValueError(f"{who}: hist must be [n, 2, {HUFF_WORDS}] or [2, {HUFF_WORDS}], got {a.shape}")
    if a.size and (int(a.min()) < 0 or int(a.max()) > MAX_BLOCKS * 64):
        raise ValueError(f"{who}: counts must be in 0..2^26")
    a = np.ascontiguousarray(a.reshape(-1, 2, HUFF_WORDS).astype(np.uint32))
    n = a.shape[0]
    if n > MAX_FRAMES:
        raise ValueError(f"{who}: {n} frames (at most {MAX_FRAMES})")
    counts = np.zeros((n, 2, 2, 16), np.uint8)
    symbols = np.zeros((n, 2, 2, 256), np.uint8)
    nsym = np.zeros((n, 2, 2), np.int32)
    ehuff = np.zeros((n, 2, HUFF_WORDS), np.uint32)
    if n:
        check(lib().elvis_jpeg_optimal_tables(a.ctypes.data, n, int(channels), counts.ctypes.data, symbols.ctypes.data, nsym.ctypes.data,
                                              ehuff.ctypes.data))
    tables = [tuple((tuple(counts[f, t, k].tolist()), tuple(symbols[f, t, k, :nsym[f, t, k]].tolist()))
                    for t in range(2 if channels == 3 else 1) for k in range(2)) for f in range(n)]
    return (tables[0], ehuff[0]) if single else (tables, ehuff)


def _check_huffman(huffman, channels: int, who: str):
    """`huffman=` of `jpeg_file_header`: 2 (gray) or 4 (colour) (counts, symbols) pairs in the order DC 0, AC 0, DC 1, AC 1,
    each a code a baseline decoder can build: 16 counts, as many distinct symbols as they add up to, 1..12 categories 0..11
    for DC and 1..256 bytes for AC, no code past its length (T.81 C.2) and none of all ones."""
    want = 4 if channels == 3 else 2
    try:
        pairs = [(tuple(int(v) for v in counts), tuple(int(v) for v in symbols)) for counts, symbols in huffman]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: huffman must be {want} (counts, symbols) pairs of integers") from None
    if len(pairs) != want:
        raise ValueError(f"{who}: huffman must hold {want} tables for {channels} channel(s) (DC 0, AC 0" + (", DC 1, AC 1)" if want == 4 else ")")
                         + f", got {len(pairs)}")
    for k, (counts, symbols) in enumerate(pairs):
        name = f"huffman[{k}] ({'AC' if k & 1 else 'DC'} {k >> 1})"
        if len(counts) != 16 or any(not 0 <= v <= 255 for v in counts):
            raise ValueError(f"{who}: {name}: 16 counts in 0..255 are needed, got {counts}")
        if sum(counts) != len(symbols) or not symbols:
            raise ValueError(f"{who}: {name}: the counts add up to {sum(counts)} and there are {len(symbols)} symbols")
        top = 255 if k & 1 else 11
        if len(set(symbols)) != len(symbols) or any(not 0 <= v <= top for v in symbols):
            raise ValueError(f"{who}: {name}: symbols must be distinct and in 0..{top}")
        code = 0                                                 # the next code of the current length (T.81 C.2)
        for length in range(1, 17):
            code += counts[length - 1]
            if counts[length - 1] and code > (1 << length) - 1:  # the last one is `length` ones, or past them
                raise ValueError(f"{who}: {name}: the counts give a code of {length} bits that does not fit or is all ones")
            code <<= 1
    return pairs


def _segment(marker: int, body: bytes) -> bytes:
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


def _dht_segments(tables) -> bytes:
    """The DHT segments of (counts, symbols) pairs in the order DC 0, AC 0 (, DC 1, AC 1): table k has class k & 1 and
    destination k >> 1."""
    return b"".join(_segment(0xC4, bytes([(k & 1) << 4 | k >> 1]) + bytes(counts) + bytes(symbols)) for k, (counts, symbols) in enumerate(tables))


def jpeg_file_header(width: int, height: int, channels: int = 3, quality: int = 95, subsampling: str = "420",
                     restart_interval: int = 0, huffman=None) -> bytes:
    """Host only: everything of a file in front of its entropy-coded bytes - SOI, the JFIF APP0 segment, one DQT segment per
    table, SOF0, the DHT segments (DC 0, AC 0, and DC 1, AC 1 for colour), for a `restart_interval` (in MCUs) other than
    0 the DRI segment FF DD 00 04 <interval, big-endian>, where libjpeg's `write_scan_header` puts it, and SOS; the
    device's scan, which ends with EOI, follows it.  Components 1 (Y: table 0, Huffman tables 0) and, for colour, 2 and
    3 (Cb, Cr: table 1, Huffman tables 1).  `huffman=`: None for the Annex K tables, or the file's own as (counts,
    symbols) for DC 0, AC 0 and, for colour, DC 1, AC 1 - what `jpeg_optimal_tables` returns for a frame - written as four
    (two) DHT segments in the same places; tables that are no code are a ValueError."""
    who = "jpeg_file_header"
    ri = restart_interval
    if isinstance(ri, bool) or not isinstance(ri, (int, np.integer)) or not 0 <= int(ri) <= 65535:
        raise ValueError(f"{who}: restart_interval must be an integer in 0..65535, got {ri!r}")
    q = _check_quality(quality, who)
    _check_subsampling(subsampling, who)
    if isinstance(channels, bool) or channels not in (1, 3):
        raise ValueError(f"{who}: channels must be 1 or 3, got {channels!r}")
    if not 1 <= int(width) <= 65535 or not 1 <= int(height) <= 65535:
        raise ValueError(f"{who}: width and height must be in 1..65535, got {width} x {height}")
    hmax, vmax = _FACTORS[subsampling] if channels == 3 else (1, 1)
    comps = [(1, hmax, vmax, 0)] + ([(2, 1, 1, 1), (3, 1, 1, 1)] if channels == 3 else [])
    ntab = 2 if channels == 3 else 1
    tables = (STD_DC[0], STD_AC[0], STD_DC[1], STD_AC[1])[:2 * ntab] if huffman is None else _check_huffman(huffman, channels, who)
    out = bytearray(b"\xff\xd8") + _segment(0xE0, _JFIF)
    for t, table in enumerate(jpeg_quant_tables(q)[:ntab]):
        out += _segment(0xDB, bytes([t]) + bytes(int(table[z]) for z in ZIGZAG))
    out += _segment(0xC0, bytes([8]) + struct.pack(">HH", int(height), int(width)) + bytes([len(comps)])
                    + b"".join(bytes([cid, h << 4 | v, tq]) for cid, h, v, tq in comps))
    out += _dht_segments(tables)
    if int(ri):
        out += _segment(0xDD, struct.pack(">H", int(ri)))
    out += _segment(0xDA, bytes([len(comps)]) + b"".join(bytes([cid, tq * 0x11]) for cid, _, _, tq in comps) + bytes([0, 63, 0]))
    return bytes(out)


def _frame_headers(width: int, height: int, channels: int, quality: int, subsampling: str, restart_interval: int, huffman) -> List[bytes]:
    """`jpeg_file_header(..., huffman=tables)` for every frame's tables of `jpeg_optimal_tables`, which the library has
    checked: the header's other segments are the clip's, so they are made once and a frame's own DHT segments take the
    place of the Annex K ones."""
    shared = jpeg_file_header(width, height, channels, quality, subsampling, restart_interval)
    annex = _dht_segments((STD_DC[0], STD_AC[0], STD_DC[1], STD_AC[1])[:4 if channels == 3 else 2])
    if shared.count(annex) != 1:
        raise RuntimeError("jpeg_write: the header does not hold its DHT segments once")
    front, back = shared.split(annex)
    return [front + _dht_segments(tables) + back for tables in huffman]


# ----------------------------------------------------------------------------- the device forms
def _check_clip(frames_d, order, quality, subsampling, who: str, roi_levels=None, roi_block_size=0):
    """Every argument check, before the library is touched: (n, h, w, c, order code, quality, sampling code, the ROI map
    as `_check_roi` gives it)."""
    if order not in ("bgr", "rgb"):
        raise ValueError(f"{who}: order must be 'bgr' or 'rgb', got {order!r}")
    q = _check_quality(quality, who)
    scode = _check_subsampling(subsampling, who)
    if not isinstance(frames_d, torch.Tensor) or frames_d.dtype != torch.uint8:
        raise ValueError(f"{who}: frames must be a uint8 tensor")
    if frames_d.dim() not in (3, 4):
        raise ValueError(f"{who}: frames must be [n,H,W,3], [n,H,W,1] or [n,H,W], got {tuple(frames_d.shape)}")
    n, h, w = (int(v) for v in frames_d.shape[:3])
    c = int(frames_d.shape[3]) if frames_d.dim() == 4 else 1
    if c not in (1, 3):
        raise ValueError(f"{who}: {c} channels (C must be 1 or 3)")
    if h < 1 or w < 1:
        raise ValueError(f"{who}: empty frames {tuple(frames_d.shape)}")
    if h > 65535 or w > 65535 or 3 * (-(-w // 8) + 1) * (-(-h // 8) + 1) > MAX_BLOCKS:
        raise ValueError(f"{who}: a {h} x {w} frame is too large (sides up to 65535, 3 * (W/8 + 1) * (H/8 + 1) up to 2^20)")
    if n > MAX_FRAMES:
        raise ValueError(f"{who}: {n} frames in one launch (at most {MAX_FRAMES}); encode the clip in parts")
    roi = _check_roi(roi_levels, roi_block_size, n, h, w, who)
    if not frames_d.is_cuda:
        raise ValueError(f"{who}: frames must be resident on the device (got a '{frames_d.device}' tensor)")
    if not frames_d.is_contiguous():
        raise ValueError(f"{who}: frames must be contiguous")
    if roi is not None and isinstance(roi[0], torch.Tensor) and (roi[0].device != frames_d.device or not roi[0].is_contiguous()):
        raise ValueError(f"{who}: a resident roi_levels must be contiguous and on the clip's device, {frames_d.device} (got '{roi[0].device}')")
    return n, h, w, c, int(order == "bgr"), q, scode, roi


def _check_segments(n: int, h: int, w: int, c: int, subsampling: str, ri: int, who: str) -> Tuple[int, int]:
    """(the restart intervals of a frame, 1 without an interval or with one that holds the whole scan; its MCUs).  A clip
    with more (frame, interval) pairs than one launch takes is refused here, before the library is touched."""
    hmax, vmax = _FACTORS[subsampling] if c == 3 else (1, 1)
    mcus = -(-w // (8 * hmax)) * -(-h // (8 * vmax))
    segs = -(-mcus // ri) if 0 < ri < mcus else 1
    if n * segs > MAX_SEGMENTS:
        raise ValueError(f"{who}: {n} frames of {segs} restart intervals are more than {MAX_SEGMENTS} segments in one launch; encode the clip "
                         f"in parts or widen the interval")
    return segs, mcus


def _guarded(nbytes: int, guard: int, dev, fill: int = 0):
    """(a uint8 buffer of nbytes holding `fill` with `guard` bytes of 0xA5 on either side, the payload's view).  Every
    byte the kernels read from a work buffer they wrote before; `fill` is the tests' knob to show it."""
    buf = torch.full((nbytes + 2 * guard,), fill, dtype=torch.uint8, device=dev)
    if guard:
        buf[:guard] = 0xA5
        buf[guard + nbytes:] = 0xA5
    return buf, buf[guard:guard + nbytes]


def _encode_clip(frames_d: torch.Tensor, order, quality, subsampling, who: str, guard: int = 0, fill: int = 0, restart=(0, 0), roi_levels=None,
                 roi_block_size: int = 0, sizes_only: bool = False, optimize: bool = False):
    """The four calls and the two small downloads between them.  Returns None for an empty clip, else a dict: `out_buf`
    (the finished scans on the device with `guard` bytes of 0xA5 on either side), `out_off` (int64 [n + 1], frame f's scan
    is bytes out_off[f] .. out_off[f + 1] of the payload), `header`, and the work buffers with their guards (`coef_buf`,
    `bits_buf`, `words_buf`, `ffc_buf`, `sizes_buf`) with `blocks` and `chunks`; `out` is the payload of `out_buf`.

    `restart` = (restart_rows, restart_mcus).  Without an interval the layouts are: bits u32 [n, blocks + 1], words as
    `word_off` of the frames' byte counts says, ffc u32 [n, chunks + 1], sizes u32 [n].  With one the library's restart
    entry points run and everything behind the coefficients is per segment q = f * segments + s: bits u32 [n * segments,
    segment_blocks + 1] (a frame's last segment may hold fewer blocks; the elements past them repeat its bit count), a
    span of whole words for every segment in words_buf (no two segments share a word, however short they are), ffc u32
    [n * segments, chunks + 1] with `chunks` those of the longest segment, sizes u32 [n * segments] (each with the 2
    bytes of its RSTm or EOI).  A frame's finished scan is its segments back to back, so `out_off` stays per frame; the
    dict gains `restart_interval`, `segments`, `segment_blocks` and `seg_off` (int64 [n * segments + 1]).

    `roi_levels` / `roi_block_size`: the map of the module docstring; a host array is uploaded, and the transform runs
    through `elvis_jpeg_fdct_roi`.  `sizes_only=True` stops behind the second download: no stuffing pass, no output
    buffer; the dict has `file_bytes` (int64 [n], header and markers included) instead of `out_buf`, `out` and
    `out_off`.

    `optimize=True`: between the transform and the bit count the tally runs (`elvis_jpeg_tally`, which zeroes the
    histograms itself), the histograms come down - a third synchronisation, the first in order - the tables are built on
    the host (`jpeg_optimal_tables`) and their code words uploaded, and the bit count and the pack call run through the
    `_ftab` entry points with a table set per frame.  The dict has `headers` (a list, one per frame) in the place of
    `header`, and gains `hist_buf` (u32 [n, 2, 272] with its guards), `huffman` (every frame's tables) and `ehuff` (the
    uploaded words, uint32 [n, 2, 272] on the host); `file_bytes` counts every frame's own header."""
    rows, mcus = _check_restart(*restart, who)
    optimize = _check_optimize(optimize, who)
    n, h, w, c, ocode, q, scode, roi = _check_clip(frames_d, order, quality, subsampling, who, roi_levels, roi_block_size)
    ri = jpeg_restart_interval(w, h, c, subsampling, rows, mcus)
    segs, mcus_of_frame = _check_segments(n, h, w, c, subsampling, ri, who)
    if n == 0:
        return None
    if guard % 16:
        raise ValueError("guard must be a multiple of 16")
    dev = frames_d.device
    blocks = int(lib().elvis_jpeg_frame_blocks(h, w, c, scode))      # the kernels' own count sizes the buffers
    if blocks < 1:
        raise ValueError(f"{who}: the library refuses a {h} x {w} frame of {c} channel(s)")
    segb = blocks
    if ri:
        if int(lib().elvis_jpeg_segments(h, w, c, scode, ri)) != segs:
            raise ValueError(f"{who}: the library counts other than {segs} restart intervals of {ri} MCUs in a {h} x {w} frame")
        segb = blocks if segs == 1 else ri * (blocks // mcus_of_frame)
    nseg = n * segs
    tail = (ri,) if ri else ()          # the restart entry points take the interval behind `sampling`
    bits_fn, pack_fn, stuff_fn = ((lib().elvis_jpeg_bits_rst, lib().elvis_jpeg_pack_rst, lib().elvis_jpeg_stuff_rst) if ri else
                                  (lib().elvis_jpeg_bits, lib().elvis_jpeg_pack, lib().elvis_jpeg_stuff))
    stuff_tail = tail
    if optimize:                        # a table set per frame; these two take the interval always, 0 for none
        bits_fn, pack_fn, tail = lib().elvis_jpeg_bits_ftab, lib().elvis_jpeg_pack_ftab, (ri,)
    header = None if optimize else jpeg_file_header(w, h, c, q, subsampling, ri)
    extra = {}
    s = _s(frames_d)
    with torch.cuda.device(dev):
        ehuff_d = torch.from_numpy(encode_tables().view(np.int32)).to(dev)
        coef_buf, coef_d = _guarded(n * blocks * 128, guard, dev, fill)
        bits_buf, bits_d = _guarded(nseg * (segb + 1) * 4, guard, dev, fill)
        if roi is None:
            check(lib().elvis_jpeg_fdct(ptr(frames_d), ptr(coef_d), n, h, w, c, ocode, q, scode, s), dev)
        else:
            levels, by, bx, b = roi
            levels_d = levels if isinstance(levels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(levels)).to(dev)
            check(lib().elvis_jpeg_fdct_roi(ptr(frames_d), ptr(coef_d), n, h, w, c, ocode, q, scode, ptr(levels_d), by, bx, b, s), dev)
        if optimize:
            hist_buf, hist_d = _guarded(n * 2 * HUFF_WORDS * 4, guard, dev, fill)
            check(lib().elvis_jpeg_tally(ptr(coef_d), ptr(hist_d), n, h, w, c, scode, ri, s), dev)
            # a synchronisation of its own, in front of the other two: every frame's symbol counts, 2 KB a frame
            hist = hist_d.cpu().numpy().view(np.uint32).reshape(n, 2, HUFF_WORDS)
            huffman, ehuff = jpeg_optimal_tables(hist, c)
            ehuff_d = torch.from_numpy(ehuff.view(np.int32)).to(dev)
            headers = _frame_headers(w, h, c, q, subsampling, ri, huffman)
            extra = {"headers": headers, "hist_buf": hist_buf, "huffman": huffman, "ehuff": ehuff}
        check(bits_fn(ptr(coef_d), ptr(ehuff_d), ptr(bits_d), n, h, w, c, scode, *tail, s), dev)
        # the first synchronisation of a clip: every segment's bit count (a frame is one segment without an interval)
        total_bits = bits_d.view(torch.int32).view(nseg, segb + 1)[:, segb].cpu().numpy().view(np.uint32).astype(np.int64)
        stream_bytes = (total_bits + 7) // 8
        word_off = np.concatenate([[0], np.cumsum((stream_bytes + 3) // 4)]).astype(np.int64)
        total_words = int(word_off[-1])
        chunks = max(1, int(-(-int(stream_bytes.max()) // STUFF_CHUNK_BYTES)))
        word_off_d = torch.from_numpy(word_off).to(dev)
        words_buf, words_d = _guarded(total_words * 4, guard, dev, fill)
        ffc_buf, ffc_d = _guarded(nseg * (chunks + 1) * 4, guard, dev, fill)
        sizes_buf, sizes_d = _guarded(nseg * 4, guard, dev, fill)
        check(pack_fn(ptr(coef_d), ptr(ehuff_d), ptr(bits_d), ptr(word_off_d), ptr(words_d), total_words, ptr(ffc_d), chunks, ptr(sizes_d), n, h, w, c,
                      scode, *tail, s), dev)
        # the second: every segment's byte count with the stuffed zeros and its marker or EOI
        sizes = sizes_d.cpu().numpy().view(np.uint32).astype(np.int64)
        seg_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        if sizes_only:
            head_bytes = np.asarray([len(x) for x in extra["headers"]], np.int64) if optimize else len(header)
            got = {"file_bytes": head_bytes + np.diff(seg_off[::segs]), "header": header, "coef_buf": coef_buf, "bits_buf": bits_buf,
                   "words_buf": words_buf, "ffc_buf": ffc_buf, "sizes_buf": sizes_buf, "blocks": blocks, "chunks": chunks}
            if ri:
                got.update(restart_interval=ri, segments=segs, segment_blocks=segb, seg_off=seg_off)
            if optimize:
                del got["header"]
                got.update(extra)
            return got
        total = int(seg_off[-1])
        seg_off_d = torch.from_numpy(seg_off).to(dev)
        out_buf, out_d = _guarded(total, guard, dev, fill)
        check(stuff_fn(ptr(bits_d), ptr(word_off_d), ptr(words_d), total_words, ptr(ffc_d), chunks, ptr(seg_off_d), ptr(out_d), total, n, h, w, c, scode,
                       *stuff_tail, s), dev)
    got = {"out_buf": out_buf, "out": out_d, "out_off": np.ascontiguousarray(seg_off[::segs]), "header": header, "coef_buf": coef_buf,
           "bits_buf": bits_buf, "words_buf": words_buf, "ffc_buf": ffc_buf, "sizes_buf": sizes_buf, "blocks": blocks, "chunks": chunks}
    if ri:
        got.update(restart_interval=ri, segments=segs, segment_blocks=segb, seg_off=seg_off)
    if optimize:
        del got["header"]
        got.update(extra)
    return got


def _encode_to_host(frames_d, order, quality, subsampling, who: str, restart=(0, 0), roi_levels=None, roi_block_size=0,
                    optimize: bool = False) -> List[bytes]:
    got = _encode_clip(frames_d, order, quality, subsampling, who, restart=restart, roi_levels=roi_levels, roi_block_size=roi_block_size,
                       optimize=optimize)
    if got is None:
        return []
    host = got["out"].cpu().numpy()
    off = got["out_off"]
    heads = got["headers"] if "headers" in got else [got["header"]] * (off.size - 1)
    return [heads[f] + host[int(off[f]):int(off[f + 1])].tobytes() for f in range(off.size - 1)]


def encode_jpeg_device(frames_d: torch.Tensor, order: str = "bgr", quality: int = 95, subsampling: str = "420", *, restart_rows: int = 0,
                       restart_mcus: int = 0, roi_levels=None, roi_block_size: int = 0, optimize: bool = False) -> List[bytes]:
    """One complete baseline JPEG file per frame of a resident contiguous uint8 clip [n,H,W,3], [n,H,W,1] or [n,H,W].
    `order` is the channel order of a 3-channel clip ("bgr", what `save_frame` takes, or "rgb"); `quality` 1..100 and
    `subsampling` "444" | "422" | "420" are libjpeg's; quality 95 and 4:2:0, the defaults, are what `cv2.imwrite` uses.
    A gray clip is one component and `subsampling` is ignored.  `restart_rows=r` (an interval of r MCU rows, at most
    65535 MCUs) or `restart_mcus=k` (an interval of k MCUs, 1..65535), one of them, writes restart intervals: DRI in the
    header, RSTm between the intervals; the default is none.  Turn it on where the device reader will read the files.
    `roi_levels=` (uint8 [n, By, Bx], a numpy array, which is uploaded, or a contiguous tensor on the clip's device; a
    level 0..48 per cell of `roi_block_size` x `roi_block_size` luma pixels, a multiple of 8; By is H // B or ceil(H / B),
    at least 1, Bx likewise) zeroes the AC coefficients a step coarsened by the block's level would round to zero - the
    module docstring has the rule; None writes what the writer always wrote, and so does a map of zeros.
    `optimize=True` codes every frame with its own optimal Huffman tables, written into its DHT segments (libjpeg's
    `optimize_coding`; the module docstring has the steps): smaller files, the same pixels, one more synchronisation.
    A frame's bytes depend on that frame and its own map only, not on the frames it is encoded with.  ValueError before
    any launch for a bad argument; an empty clip gives []."""
    return _encode_to_host(frames_d, order, quality, subsampling, "encode_jpeg_device", (restart_rows, restart_mcus), roi_levels, roi_block_size,
                           optimize)


def save_jpeg_frames_device(frames_d: torch.Tensor, paths: Sequence, order: str = "bgr", quality: int = 95, subsampling: str = "420", *,
                            restart_rows: int = 0, restart_mcus: int = 0, roi_levels=None, roi_block_size: int = 0,
                            optimize: bool = False) -> None:
    """`encode_jpeg_device`, and frame i written to paths[i]; directories are created as `save_frame` does."""
    paths = list(paths)
    if not isinstance(frames_d, torch.Tensor) or frames_d.dim() < 1 or len(paths) != frames_d.shape[0]:
        raise ValueError(f"save_jpeg_frames_device: {len(paths)} path(s) for the clip {tuple(getattr(frames_d, 'shape', ()))}")
    for path, data in zip(paths, _encode_to_host(frames_d, order, quality, subsampling, "save_jpeg_frames_device", (restart_rows, restart_mcus),
                                                 roi_levels, roi_block_size, optimize)):
        os.makedirs(os.path.dirname(os.fspath(path)) or ".", exist_ok=True)
        with open(path, "wb") as f:
            f.write(data)


def save_jpeg_frames(frames, paths: Sequence, device="cuda:0", *, chunk_frames=None, order: str = "bgr", quality: int = 95,
                     subsampling: str = "420", restart_rows: int = 0, restart_mcus: int = 0, roi_levels=None, roi_block_size: int = 0,
                     optimize: bool = False) -> None:
    """Host frames - uint8 (H,W,3), (H,W,1) or (H,W) arrays, a list or one [n,...] array - written as JPEGs to `paths`
    through the device.  Uploaded and encoded `chunk_frames` frames at a time, by default as many as make 32 MB (5 at
    1080p); a run of equal shapes is one clip.  The files do not depend on the chunk size.  `restart_rows` / `restart_mcus`:
    as `encode_jpeg_device` takes them.  `roi_levels` / `roi_block_size`: the same, [len(frames), By, Bx] for frames of
    one shape; every chunk takes its frames' part of the map.  `optimize`: as `encode_jpeg_device` takes it."""
    who = "save_jpeg_frames"
    paths = list(paths)
    if len(frames) != len(paths):
        raise ValueError(f"{who}: {len(frames)} frame(s) for {len(paths)} path(s)")
    if chunk_frames is not None and (isinstance(chunk_frames, bool) or int(chunk_frames) < 1):
        raise ValueError("chunk_frames must be at least 1")
    if order not in ("bgr", "rgb"):
        raise ValueError(f"{who}: order must be 'bgr' or 'rgb', got {order!r}")
    _check_quality(quality, who)
    _check_subsampling(subsampling, who)
    _check_restart(restart_rows, restart_mcus, who)
    opt_kw = {"optimize": True} if _check_optimize(optimize, who) else {}
    arrays = [np.asarray(f) for f in frames]
    for a in arrays:
        if a.dtype != np.uint8 or a.ndim not in (2, 3):
            raise ValueError(f"{who}: frames are uint8 (H,W,3), (H,W,1) or (H,W) arrays, got {a.dtype} {a.shape}")
    if roi_levels is not None or roi_block_size:
        if len({a.shape for a in arrays}) > 1:
            raise ValueError(f"{who}: roi_levels needs frames of one shape")
        if arrays:
            roi = _check_roi(roi_levels, roi_block_size, len(arrays), int(arrays[0].shape[0]), int(arrays[0].shape[1]), who)
            roi_levels = None if roi is None else roi[0]
    dev = L.resolve_device(device)
    at = 0
    with torch.cuda.device(dev):
        while at < len(arrays):
            shape = arrays[at].shape
            step = int(chunk_frames) if chunk_frames is not None else max(1, UPLOAD_CHUNK_BYTES // max(1, arrays[at].size))
            end = at + 1
            while end < len(arrays) and end - at < step and arrays[end].shape == shape:
                end += 1
            clip = torch.from_numpy(np.ascontiguousarray(np.stack(arrays[at:end], axis=0))).to(dev)
            roi_kw = {} if roi_levels is None else {"roi_levels": roi_levels[at:end], "roi_block_size": roi_block_size}
            save_jpeg_frames_device(clip, paths[at:end], order, quality, subsampling, restart_rows=restart_rows, restart_mcus=restart_mcus, **roi_kw,
                                    **opt_kw)
            at = end


def jpeg_roundtrip_device(frames_d: torch.Tensor, quality: int = 95, subsampling: str = "420", order: str = "bgr", *, restart_rows: int = 0,
                          restart_mcus: int = 0, roi_levels=None, roi_block_size: int = 0, optimize: bool = False):
    """An intra codec in the loop: `encode_jpeg_device` at `quality`, then `jpeg.decode_jpeg_device` of those files.
    Returns (the decoded resident clip, uint8 [n,H,W,C] in the clip's own channel count and `order`; the bytes of every
    frame's file, int64 [n]) - the pixels a client would see and the rate they cost.  `restart_rows=1` gives the reader a
    segment per MCU row to decode side by side: the same pixels, sooner, for a few more bytes.  `roi_levels` /
    `roi_block_size`, `optimize`: as `encode_jpeg_device` takes them (`optimize=True`: the same pixels for fewer bytes)."""
    from .jpeg import decode_jpeg_device
    files = _encode_to_host(frames_d, order, quality, subsampling, "jpeg_roundtrip_device", (restart_rows, restart_mcus), roi_levels, roi_block_size,
                            optimize)
    if not files:
        raise ValueError("jpeg_roundtrip_device: no frames")
    c = int(frames_d.shape[3]) if frames_d.dim() == 4 else 1
    decoded = decode_jpeg_device(files, frames_d.device, order, c)
    return decoded, np.asarray([len(f) for f in files], dtype=np.int64)


def jpeg_encoded_sizes_device(frames_d: torch.Tensor, quality: int = 95, subsampling: str = "420", order: str = "bgr", *, restart_rows: int = 0,
                              restart_mcus: int = 0, roi_levels=None, roi_block_size: int = 0, optimize: bool = False) -> np.ndarray:
    """int64 [n]: the length of every file `encode_jpeg_device` would return with the same arguments - header, entropy-coded
    bytes with their stuffed zeros, restart markers and EOI - without producing the files: the transform, the bit lengths
    and the pack call run, and the second small download, the pack call's sizes, ends it.  No stuffing pass, no output
    buffer, no download of a scan.  With `optimize=True` the tally and the table builder run as well and every frame's
    own header, whose DHT segments differ in length, is counted.  An empty clip gives an empty array."""
    got = _encode_clip(frames_d, order, quality, subsampling, "jpeg_encoded_sizes_device", restart=(restart_rows, restart_mcus),
                       roi_levels=roi_levels, roi_block_size=roi_block_size, sizes_only=True, optimize=optimize)
    return np.zeros(0, np.int64) if got is None else got["file_bytes"].astype(np.int64)


def jpeg_quality_for_bytes(frames_d: torch.Tensor, target_bytes: int, quality_max: int = 100, subsampling: str = "420", order: str = "bgr", *,
                           restart_rows: int = 0, restart_mcus: int = 0, roi_levels=None, roi_block_size: int = 0, optimize: bool = False):
    """The quality whose files fit `target_bytes`, the budget of the whole clip (bitrate * n / fps / 8): (quality, the
    sizes at that quality as `jpeg_encoded_sizes_device` gives them, int64 [n]; whether they fit).  The search: quality
    1 is probed, and if the clip's bytes exceed the target the answer is (1, sizes, False); else lo = 1, hi =
    `quality_max`, and while lo < hi, mid = (lo + hi + 1) // 2 is probed: lo = mid where it fits, hi = mid - 1 where it
    does not; (lo, sizes(lo), True).  At most 8 probes, each a `jpeg_encoded_sizes_device`.  The quality returned always
    fits.  Sizes are not strictly monotone in the quality, so it need not be the largest one that does.  `optimize=True`
    probes the sizes of the optimised files, headers of their own included."""
    who = "jpeg_quality_for_bytes"
    if isinstance(target_bytes, bool) or not isinstance(target_bytes, (int, np.integer)) or int(target_bytes) < 0:
        raise ValueError(f"{who}: target_bytes must be a non-negative integer, got {target_bytes!r}")
    top = _check_quality(quality_max, who)
    kw = dict(restart_rows=restart_rows, restart_mcus=restart_mcus, roi_levels=roi_levels, roi_block_size=roi_block_size)
    if _check_optimize(optimize, who):          # the default probe is the call it always was
        kw["optimize"] = True
    probed = {}

    def fits(q: int) -> bool:
        probed[q] = jpeg_encoded_sizes_device(frames_d, q, subsampling, order, **kw)
        return int(probed[q].sum()) <= int(target_bytes)

    if not fits(1):
        return 1, probed[1], False
    lo, hi = 1, top
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo, probed[lo], True


def jpeg_roundtrip_at_bytes_device(frames_d: torch.Tensor, target_bytes: int, quality_max: int = 95, subsampling: str = "420", order: str = "bgr", *,
                                   restart_rows: int = 0, restart_mcus: int = 0, roi_levels=None, roi_block_size: int = 0, optimize: bool = False):
    """An intra codec at a rate: `jpeg_quality_for_bytes` inside 1..`quality_max`, then `jpeg_roundtrip_device` at the
    quality found (quality 1 where even that does not fit).  Returns (the decoded resident clip, the bytes of every
    frame's file, int64 [n]; the quality; whether the files fit `target_bytes`).  `optimize`: on the search and on the
    round trip alike."""
    kw = dict(restart_rows=restart_rows, restart_mcus=restart_mcus, roi_levels=roi_levels, roi_block_size=roi_block_size)
    if _check_optimize(optimize, "jpeg_roundtrip_at_bytes_device"):
        kw["optimize"] = True
    quality, _, fits = jpeg_quality_for_bytes(frames_d, target_bytes, quality_max, subsampling, order, **kw)
    decoded, sizes = jpeg_roundtrip_device(frames_d, quality, subsampling, order, **kw)
    return decoded, sizes, quality, fits
