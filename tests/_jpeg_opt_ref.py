"""Per-frame optimised Huffman tables of the device JPEG writer (elvis_amd/jpeg_write.py `optimize=True`,
csrc/jpeg_write.hip `jpeg_bits_kernel` in its tally mode, csrc/jpeg_encode.h `jpeg_gen_optimal_table`) stated on top of
tests/_jpeg_write_ref.py (planes, FDCT, quantiser, header), tests/_jpeg_restart_ref.py (intervals, DRI) and
tests/_jpeg_roi_ref.py (the dead zone), which are imported, not edited.  Importable without a GPU.

The rule (libjpeg jchuff.c `encode_mcu_gather` / `htest_one_block`, `jpeg_gen_optimal_table`; T.81 K.2).  The symbols of
a frame's scan are counted per table class (0 luma / gray, 1 chroma) into hist [2, 272]: entry c for a DC difference of
category c, entry 16 + s for the AC symbol s = (run << 4) | category, ZRL F0 and EOB 00 - over every block the scan
codes, dummy blocks included, with the DC predictors reset at every restart interval and the coefficients as the ROI dead
zone left them.  A table is made of the 16 DC or the 256 AC counts: freq[256] = 1 is a reserved symbol; c1 is the
non-zero entry of smallest frequency, ties to the largest index, c2 the same over the rest; freq[c1] += freq[c2], freq[c2]
= 0, the code sizes along both `others` chains go up by one and the chains are linked; when no c2 is left the lengths are
counted (up to 32), and for i = 32 .. 17, while bits[i] > 0: j = i - 2 downwards to bits[j] != 0, bits[i] -= 2, bits[i -
1] += 1, bits[j + 1] += 2, bits[j] -= 1; the reserved symbol leaves the longest length that is not empty; the symbols are
listed by the length the merge gave them, by value within a length.  The file has the four (gray: two) tables as DHT
segments where the Annex K ones stand otherwise - DC 0, AC 0, DC 1, AC 1, in front of DRI and SOS - and its scan is coded
with them.  Against a libjpeg-turbo PIL with `optimize=True` those segments, their position and everything behind SOS are
equal byte for byte (tests/test_jpeg_opt_host.py).  `mutant=` switches on one named deviation.

    python tests/_jpeg_opt_ref.py dump FILE      writes every case of the corpus for tools/jpeg_opt_check.cpp
"""
from __future__ import annotations

import struct
import sys
from dataclasses import dataclass
from functools import lru_cache
from typing import List, Optional, Sequence, Tuple

import numpy as np

if __name__ == "__main__":          # run as a script: the package lies beside tests/
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import _jpeg_ref as R
import _jpeg_restart_ref as S
import _jpeg_roi_ref as X
import _jpeg_write_ref as W

MUTANTS = ("ties_to_smallest_index", "no_reserved_symbol", "limit_without_j_plus_1", "order_by_frequency", "dc_not_reset",
           "dummies_not_counted", "zrl_not_counted")
HUFF_WORDS = 272
SIZES = ((1, 1), (8, 8), (9, 17), (17, 33), (40, 56), (37, 53))          # (w, h)
QUALITIES = (30, 75, 95, 100)
CONTENTS = ("flat", "ramp", "noise", "smooth_noise")
SETTINGS = ((0, 0), (1, 0), (2, 0), (0, 3))                                # (restart_rows, restart_mcus)
FIXTURE_SEED = 1234


# ----------------------------------------------------------------------------- the symbols of a block
def block_events(blk: Sequence[int], pred: int) -> List[Tuple[int, int, int]]:
    """[(index into the 272 entries of the block's table class, the magnitude bits, how many of them)] (T.81 F.1.2)."""
    cat, extra = W._magnitude(blk[0] - pred)
    out = [(cat, extra, cat)]
    run = 0
    for v in blk[1:]:
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((16 + 0xF0, 0, 0))
            run -= 16
        cat, extra = W._magnitude(v)
        out.append((16 + (run << 4 | cat), extra, cat))
        run = 0
    if run:
        out.append((16, 0, 0))
    return out


def scan_events(blocks: np.ndarray, comp: np.ndarray, bpm: int, step: int, reset: bool = True):
    """Per interval of `step` MCUs a list of (table class, events of a block): the DC prediction is per component and
    starts at 0 in every interval (`reset=False`: in the first only)."""
    rows, comps = blocks.tolist(), comp.tolist()
    mcus = len(rows) // bpm
    out = []
    pred = [0, 0, 0]
    for m in range(0, mcus, step):
        if reset:
            pred = [0, 0, 0]
        interval = []
        for b in range(m * bpm, min(m + step, mcus) * bpm):
            c = comps[b]
            interval.append((min(c, 1), block_events(rows[b], pred[c])))
            pred[c] = rows[b][0]
        out.append(interval)
    return out


def histogram(blocks: np.ndarray, comp: np.ndarray, dummy: np.ndarray, bpm: int, step: int, mutant: Optional[str] = None) -> np.ndarray:
    """int64 [2, 272]: the counts of the symbols the scan holds."""
    hist = np.zeros((2, HUFF_WORDS), np.int64)
    b = 0
    for interval in scan_events(blocks, comp, bpm, step, reset=mutant != "dc_not_reset"):
        for t, events in interval:
            skip = mutant == "dummies_not_counted" and bool(dummy[b])
            b += 1
            if skip:
                continue
            for index, _, _ in events:
                if mutant == "zrl_not_counted" and index == 16 + 0xF0:
                    continue
                hist[t, index] += 1
    return hist


# ----------------------------------------------------------------------------- the table rule
def gen_optimal_table(freq_in: Sequence[int], mutant: Optional[str] = None):
    """jpeg_gen_optimal_table: (counts of the lengths 1..16, symbols in code order, the longest length before limiting)
    of up to 256 counts by symbol value; None for a histogram without a symbol."""
    given = [int(v) for v in freq_in]
    freq = given + [0] * (257 - len(given))
    if not any(freq):
        return None
    if mutant != "no_reserved_symbol":
        freq[256] = 1
    codesize, others = [0] * 257, [-1] * 257

    def least(skip: int) -> int:
        best, v = -1, None
        for i in range(257):
            if freq[i] and i != skip and (v is None or (freq[i] < v if mutant == "ties_to_smallest_index" else freq[i] <= v)):
                best, v = i, freq[i]
        return best

    while True:
        c1 = least(-1)
        c2 = least(c1)
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    prelimit = max(codesize)
    assert prelimit <= 32, prelimit
    bits = [0] * 33
    for size in codesize:
        if size:
            bits[size] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            if mutant != "limit_without_j_plus_1":
                bits[j + 1] += 2
            bits[j] -= 1
    if mutant != "no_reserved_symbol":
        i = 16
        while bits[i] == 0:
            i -= 1
        bits[i] -= 1
    if mutant == "order_by_frequency":
        order = sorted((j for j in range(256) if codesize[j]), key=lambda j: (codesize[j], -given[j] if j < len(given) else 0, j))
    else:
        order = [j for size in range(1, 33) for j in range(256) if codesize[j] == size]
    return tuple(bits[1:17]), tuple(order), prelimit


def frame_tables(hist: np.ndarray, channels: int, mutant: Optional[str] = None):
    """((counts, symbols) for DC 0, AC 0 and, for colour, DC 1, AC 1; the longest length before limiting of each)."""
    tables, prelimit = [], []
    for t in range(2 if channels == 3 else 1):
        for lo, hi in ((0, 16), (16, HUFF_WORDS)):
            counts, symbols, longest = gen_optimal_table(hist[t, lo:hi], mutant)
            tables.append((counts, symbols))
            prelimit.append(longest)
    return tuple(tables), tuple(prelimit)


def code_words(tables, channels: int) -> np.ndarray:
    """uint32 [2, 272]: (code << 5) | length by class and entry, 0 where a table has no such symbol (T.81 C.2)."""
    tab = np.zeros((2, HUFF_WORDS), np.uint32)
    for t in range(2 if channels == 3 else 1):
        for kind in range(2):
            counts, symbols = tables[2 * t + kind]
            for bitstring, sym in R.code_strings(counts, symbols).items():
                tab[t, 16 * kind + sym] = int(bitstring, 2) << 5 | len(bitstring)
    return tab


def dht_segments(tables) -> bytes:
    return b"".join(R.dht(k & 1, k >> 1, *table) for k, table in enumerate(tables))


def header(width: int, height: int, channels: int, subsampling: str, qtables, ri: int, tables) -> bytes:
    """The header of tests/_jpeg_restart_ref.py with the file's own tables in the place of the Annex K ones."""
    head = S.header(width, height, channels, subsampling, qtables, ri)
    _, dc, ac = R.std_tables()
    std = b"".join(R.dht(0, t, *dc[t]) + R.dht(1, t, *ac[t]) for t in range(len(qtables)))
    assert head.count(std) == 1
    return head.replace(std, dht_segments(tables))


def code_scan(intervals, words: np.ndarray) -> bytes:
    """Everything between SOS and EOI: every interval coded with `words`, filled with 1 bits, stuffed, RSTm between."""
    scan = bytearray()
    table = [[(int(e) >> 5, int(e) & 31) for e in row] for row in words]
    for s, interval in enumerate(intervals):
        bits: List[str] = []
        for t, events in interval:
            for index, extra, n in events:
                code, length = table[t][index]
                if length:
                    bits.append(format(code, f"0{length}b"))
                if n:
                    bits.append(format(extra, f"0{n}b"))
        text = "".join(bits)
        text += "1" * (-len(text) % 8)
        raw = int(text, 2).to_bytes(len(text) // 8, "big") if text else b""
        if s:
            scan += bytes([0xFF, 0xD0 + ((s - 1) & 7)])
        scan += raw.replace(b"\xff", b"\xff\x00")
    return bytes(scan)


@dataclass
class Encoded:
    data: bytes                 # the whole file
    scan: bytes                 # everything between SOS and EOI
    dht: bytes                  # the DHT segments, back to back
    tables: tuple               # (counts, symbols) for DC 0, AC 0 (, DC 1, AC 1)
    prelimit: tuple             # the longest code length of each table before limiting
    hist: np.ndarray            # int64 [2, 272]
    words: np.ndarray           # uint32 [2, 272]
    blocks: np.ndarray          # int16 [blocks, 64]
    dummy: np.ndarray
    comp: np.ndarray
    ri: int
    standard: bytes             # the same frame's file with the Annex K tables


def encode(frame: np.ndarray, quality: int = 95, subsampling: str = "420", order: str = "rgb", restart_rows: int = 0, restart_mcus: int = 0,
           levels=None, B: int = 8, mutant: Optional[str] = None) -> Encoded:
    """One uint8 frame (H,W), (H,W,1) or (H,W,3) as a baseline JPEG file with its own optimal Huffman tables."""
    a = np.asarray(frame)
    channels = 1 if a.ndim == 2 else a.shape[2]
    h, w = a.shape[:2]
    if levels is None:
        blocks, dummy, comp, qtables = W.quantised_blocks(a, quality, subsampling, order)
        standard = S.encode(a, quality, subsampling, order, restart_rows, restart_mcus).data
    else:
        blocks, dummy, comp, qtables, _ = X.quantised_blocks(a, quality, subsampling, order, levels, B)
        standard = X.encode(a, quality, subsampling, order, levels, B, restart_rows, restart_mcus).data
    mcux, mcuy, bpm = S.mcu_grid(w, h, channels, subsampling)
    mcus = mcux * mcuy
    ri = S.restart_interval(w, h, channels, subsampling, restart_rows, restart_mcus)
    step = ri if ri else mcus
    hist = histogram(blocks, comp, dummy, bpm, step, mutant)
    tables, prelimit = frame_tables(hist, channels, mutant)
    words = code_words(tables, channels)
    scan = code_scan(scan_events(blocks, comp, bpm, step), words)
    data = header(w, h, channels, subsampling, qtables, ri, tables) + scan + b"\xff\xd9"
    return Encoded(data, scan, dht_segments(tables), tables, prelimit, hist, words, blocks.astype(np.int16), dummy, comp, ri, standard)


def walk(data: bytes):
    """([(marker, the segment's bytes)] of a file up to and with SOS, everything behind SOS)."""
    at, seen = 2, []
    while True:
        assert data[at] == 0xFF
        m = data[at + 1]
        (ln,) = struct.unpack(">H", data[at + 2:at + 4])
        seen.append((m, data[at:at + 2 + ln]))
        at += 2 + ln
        if m == 0xDA:
            return seen, data[at:]


def dht_and_tail(data: bytes):
    """(the markers from the first DHT segment on, the DHT segments back to back, everything behind SOS)."""
    seen, tail = walk(data)
    markers = [m for m, _ in seen]
    return markers[markers.index(0xC4):], b"".join(seg for m, seg in seen if m == 0xC4), tail


# ----------------------------------------------------------------------------- the corpus
def make_frame(kind: str, h: int, w: int, c: int, seed: int) -> np.ndarray:
    if kind == "smooth_noise":
        rng = np.random.default_rng(seed)
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([96 + 60 * np.sin((xx + 3 * k) / 9.0) + 50 * np.cos((yy - 2 * k) / 7.0) for k in range(c)], axis=2)
        return np.clip(np.rint(base + rng.normal(0, 6, size=(h, w, c))), 0, 255).astype(np.uint8)
    return R.make_content(kind, h, w, c, seed)


@dataclass(frozen=True)
class Case:
    name: str
    w: int
    h: int
    sampling: str              # "gray" | "444" | "422" | "420"
    quality: int
    kind: str
    seed: int
    restart_rows: int
    restart_mcus: int

    @property
    def channels(self) -> int:
        return 1 if self.sampling == "gray" else 3

    @property
    def subsampling(self) -> str:
        return "420" if self.sampling == "gray" else self.sampling

    def frame(self) -> np.ndarray:
        """uint8 [h, w, channels], RGB."""
        if self.kind.startswith("fixture"):
            return fixture_frame(int(self.kind[7:]))[:, :, None]
        return make_frame(self.kind, self.h, self.w, self.channels, self.seed)

    @property
    def restart(self) -> dict:
        return {"restart_rows": self.restart_rows} if self.restart_rows else ({"restart_mcus": self.restart_mcus} if self.restart_mcus else {})

    @property
    def pil_restart(self) -> dict:
        return ({"restart_marker_rows": self.restart_rows} if self.restart_rows else
                ({"restart_marker_blocks": self.restart_mcus} if self.restart_mcus else {}))


@lru_cache(maxsize=None)
def cases() -> Tuple[Case, ...]:
    """Every size x sampling x restart setting with the quality and the content cycling, and at 40 x 56 and 37 x 53 every
    sampling x quality x content with the restart setting cycling (a case the first part already has is not repeated):
    every value of every axis meets every value of every other."""
    out, k = [], 0

    def add(w, h, s, q, kind, setting):
        nonlocal k
        rows, mcus = setting
        name = f"w{w}-h{h}-{s}-q{q}-{kind}-" + (f"rows{rows}" if rows else (f"mcus{mcus}" if mcus else "none"))
        if not any(c.name == name for c in out):
            out.append(Case(name, w, h, s, q, kind, 1500 + k, rows, mcus))
        k += 1

    for w, h in SIZES:
        for s in R.SAMPLINGS:
            for setting in SETTINGS:
                add(w, h, s, QUALITIES[(k + k // 4) % 4], CONTENTS[(k // 2 + k // 16) % 4], setting)
    for w, h in ((40, 56), (37, 53)):
        for s in R.SAMPLINGS:
            for q in QUALITIES:
                for kind in CONTENTS:
                    add(w, h, s, q, kind, SETTINGS[(k + k // 4) % 4])
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


FIXTURE = Case("fixture16-gray-q75", 520, 520, "gray", 75, "fixture16", 0, 0, 0)
FIXTURE17 = Case("fixture17-gray-q75", 664, 664, "gray", 75, "fixture17", 0, 0, 0)


def case(name: str) -> Case:
    return next(c for c in cases() + (FIXTURE, FIXTURE17) if c.name == name)


@lru_cache(maxsize=None)
def encoded(name: str, order: str = "rgb") -> Encoded:
    """The statement's file for a case by name, computed once."""
    c = case(name)
    frame = c.frame()
    return encode(frame[:, :, ::-1] if order == "bgr" and c.channels == 3 else frame, c.quality, c.subsampling, order, **c.restart)


def pil_encode(c: Case, optimize: bool = True) -> bytes:
    """PIL's file of the case with `optimize=True` and its restart setting."""
    import io
    from PIL import Image
    a = c.frame()
    img = Image.fromarray(a[:, :, 0] if c.channels == 1 else a)
    buf = io.BytesIO()
    kw = {} if c.channels == 1 else {"subsampling": R._PIL_SUB[c.subsampling]}
    img.save(buf, "JPEG", quality=c.quality, optimize=optimize, **kw, **c.pil_restart)
    return buf.getvalue()


# ----------------------------------------------------------------------------- the length-limit fixture
def fibonacci(count: int) -> List[int]:
    """1, 2, 3, 5, 8, ..."""
    out = [1, 2]
    while len(out) < count:
        out.append(out[-1] + out[-2])
    return out[:count]


def fixture_symbols(count: int) -> List[Tuple[int, int]]:
    """(run, category): (r, 1) for r = 0..11, then (r, 2) for r = 0.."""
    return ([(r, 1) for r in range(12)] + [(r, 2) for r in range(count - 12)])[:count]


@lru_cache(maxsize=None)
def fixture_frame(count: int = 16) -> np.ndarray:
    """A gray frame for quality 75 whose AC table reaches a length above 16 before limiting: every 8 x 8 block holds one AC
    coefficient, of magnitude Q (category 1) or 3 Q (category 2) at zig-zag position r + 1 - the symbol (r, category) - made
    by adding that DCT basis function to 128 and rounding; symbol k of `fixture_symbols` is held by the k-th of 1, 2, 3, 5,
    8, ... blocks, shuffled over the smallest square grid that takes them (65 x 65 blocks for 16 symbols, 83 x 83 for 17);
    the blocks left over are flat 128."""
    qt = W.quant_tables(75)[0]
    counts = fibonacci(count)
    side = int(np.ceil(np.sqrt(sum(counts))))
    which = np.full(side * side, -1, np.int64)
    which[:sum(counts)] = np.repeat(np.arange(count), counts)
    which = np.random.default_rng(FIXTURE_SEED).permutation(which).reshape(side, side)
    xs = (2 * np.arange(8) + 1) * np.pi / 16
    tiles = [np.full((8, 8), 128, np.uint8)]
    for run, cat in fixture_symbols(count):
        nat = R.ZIGZAG[run + 1]
        v, u = nat // 8, nat % 8
        cu, cv = (2 ** -0.5 if u == 0 else 1.0), (2 ** -0.5 if v == 0 else 1.0)
        amp = (1 if cat == 1 else 3) * int(qt[nat])
        basis = 0.25 * cu * cv * np.outer(np.cos(xs * v), np.cos(xs * u))
        tiles.append(np.clip(np.rint(128 + amp * basis), 0, 255).astype(np.uint8))
    tiles = np.stack(tiles)
    frame = tiles[which + 1]                                    # [side, side, 8, 8]
    return np.ascontiguousarray(frame.transpose(0, 2, 1, 3).reshape(side * 8, side * 8))


def fibonacci_histogram(symbols: int, entries: int = 256) -> np.ndarray:
    """`symbols` counts 1, 2, 3, 5, ... spread over `entries`: with the reserved symbol the longest code before limiting
    has `symbols` bits (two of the lightest leaves) for symbols >= 2."""
    freq = np.zeros(entries, np.int64)
    at = np.linspace(0, entries - 1, symbols).astype(np.int64)
    freq[at] = fibonacci(symbols)
    return freq


# ----------------------------------------------------------------------------- the corpus for the host check
def dump(path: str) -> None:
    """Every case, and the fixture, as tools/jpeg_opt_check.cpp reads it: the shape and the settings with the interval in
    MCUs, the statement's quantised blocks, its histograms, its tables (counts u8 [2, 2, 16], symbols u8 [2, 2, 256], how
    many i32 [2, 2]), its code words, and everything between SOS and the end of the file."""
    todo = cases() + (FIXTURE,)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(todo)))
        for c in todo:
            e = encoded(c.name)
            counts, symbols, nsym = np.zeros((2, 2, 16), np.uint8), np.zeros((2, 2, 256), np.uint8), np.zeros((2, 2), "<i4")
            for k, (cnt, sym) in enumerate(e.tables):
                counts[k >> 1, k & 1] = cnt
                symbols[k >> 1, k & 1, :len(sym)] = sym
                nsym[k >> 1, k & 1] = len(sym)
            fh.write(struct.pack("<I", len(c.name)) + c.name.encode())
            fh.write(struct.pack("<5I", c.h, c.w, c.channels, W.SUBSAMPLINGS.index(c.subsampling), e.ri))
            for blob in (e.blocks.astype("<i2").tobytes(), e.hist.astype("<u4").tobytes(), counts.tobytes(), symbols.tobytes(), nsym.tobytes(),
                         e.words.astype("<u4").tobytes(), e.scan + b"\xff\xd9"):
                fh.write(struct.pack("<I", len(blob)) + blob)
    print(f"{len(todo)} cases -> {path}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(__doc__)
