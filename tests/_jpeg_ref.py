"""The device JPEG reader's contract (elvis_amd/jpeg.py, csrc/jpeg_read.hip, csrc/jpeg_decode.h) stated in
pure Python and numpy, and the corpus the host tests, the GPU tests and tools/jpeg_decode_check.cpp share.  Importable
without a GPU.

The statement: the marker walk of a baseline file, the entropy decode of ITU-T T.81 F.2.2 one bit string at a time, the
slow integer IDCT of libjpeg's jidctint.c in exact integers, libjpeg's fancy chroma upsampling (plain replication where
the chroma plane is at most 2 samples wide, as libjpeg chooses), and its fixed-point colour conversion.  The result of a
well-formed file equals `np.asarray(Image.open(f).convert("RGB"))` of a PIL built on libjpeg-turbo with default
settings, bit for bit.  `mutant=` switches on one named deviation.

What PIL does with corrupt data - warnings and partial pictures - is NOT reproduced: every defect of the entropy-coded
data is one of four status codes per segment, the first defect of a segment ends it, the first defective segment in
file order gives the file's status, and the reader raises IOError naming the file.  Bits left over at a segment's end
are ignored, as libjpeg ignores them.  A segment's coefficient blocks hold what was stored before the defect; the
blocks behind it stay zero.

`write_jpeg` is a small baseline writer - coefficients, tables and a restart interval in, bytes out - for the streams
PIL never writes.

    python tests/_jpeg_ref.py dump FILE      writes every case of the corpus for tools/jpeg_decode_check.cpp
"""
from __future__ import annotations

import io
import struct
import sys
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

if __name__ == "__main__":          # run as a script: the package lies beside tests/
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OK, E_CODE, E_INDEX, E_BITS, E_RANGE = range(5)
STATUS_NAMES = ("ok", "no Huffman code of up to 16 bits matches", "coefficient index past 63",
                "the bits run out before the segment's MCUs are done", "dequantised coefficient outside [-32768, 32767]")
MUTANTS = ("h2v2_round_swapped", "h2v1_first", "column_no_round", "g_no_round", "extend_off_by_one", "dc_no_reset",
           "zigzag_transposed")
# natural (row-major) index of zig-zag position k
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


def have_turbo() -> bool:
    """Whether PIL is the second oracle: an IJG libjpeg 7+ upsamples differently."""
    try:
        from PIL import features
        return bool(features.check_feature("libjpeg_turbo"))
    except Exception:
        return False


# ----------------------------------------------------------------------------- the marker walk
@dataclass
class Walk:
    width: int
    height: int
    comps: List[Tuple[int, int, int, int]]              # (id, h, v, quantisation table) in frame order
    scan: List[Tuple[int, int, int]]                    # (index into comps, DC table, AC table) in scan order
    qt: Dict[int, np.ndarray]                           # natural order, int
    dc: Dict[int, Tuple[List[int], List[int]]]          # (16 counts, values)
    ac: Dict[int, Tuple[List[int], List[int]]]
    ri: int
    segments: List[bytes]                               # entropy-coded bytes between the markers, fill FFs trimmed
    offsets: List[int] = field(default_factory=list)    # where each segment starts in the file


def walk(data: bytes) -> Walk:
    """A well-formed baseline file's tables and segments (the reader's own parser, `jpeg.parse_jpeg`, is the strict one)."""
    assert data[:2] == b"\xff\xd8"
    at, w = 2, Walk(0, 0, [], [], {}, {}, {}, 0, [])
    while True:
        assert data[at] == 0xFF
        while data[at + 1] == 0xFF:
            at += 1
        m = data[at + 1]
        (ln,) = struct.unpack(">H", data[at + 2:at + 4])
        body = data[at + 4:at + 2 + ln]
        at += 2 + ln
        if m == 0xDB:
            p = 0
            while p < len(body):
                prec, t = body[p] >> 4, body[p] & 15
                n = 128 if prec else 64
                vals = np.frombuffer(body[p + 1:p + 1 + n], dtype=">u2" if prec else np.uint8).astype(np.int64)
                nat = np.zeros(64, np.int64)
                nat[list(ZIGZAG)] = vals
                w.qt[t] = nat
                p += 1 + n
        elif m == 0xC4:
            p = 0
            while p < len(body):
                cls, t = body[p] >> 4, body[p] & 15
                counts = list(body[p + 1:p + 17])
                values = list(body[p + 17:p + 17 + sum(counts)])
                (w.ac if cls else w.dc)[t] = (counts, values)
                p += 17 + sum(counts)
        elif m in (0xC0, 0xC1):
            w.height, w.width = struct.unpack(">HH", body[1:5])
            for c in range(body[5]):
                cid, hv, tq = body[6 + 3 * c:9 + 3 * c]
                w.comps.append((cid, hv >> 4, hv & 15, tq))
        elif m == 0xDD:
            (w.ri,) = struct.unpack(">H", body)
        elif m == 0xDA:
            for c in range(body[0]):
                cid, tt = body[1 + 2 * c:3 + 2 * c]
                w.scan.append(([k[0] for k in w.comps].index(cid), tt >> 4, tt & 15))
            break
    start = at
    while True:
        if data[at] == 0xFF and data[at + 1] != 0:
            end = at
            while data[at + 1] == 0xFF:
                at += 1
            w.segments.append(data[start:end])
            w.offsets.append(start)
            if 0xD0 <= data[at + 1] <= 0xD7:
                at += 2
                start = at
                continue
            assert data[at + 1] == 0xD9
            return w
        at += 2 if data[at] == 0xFF else 1


# ----------------------------------------------------------------------------- geometry shared with the device
@dataclass
class Geometry:
    ncomp: int
    hmax: int
    vmax: int
    mcux: int
    mcuy: int
    samp: List[Tuple[int, int]]     # per component in frame order (a single component counts as 1x1)
    base: List[int]                 # first block of the component among the frame's blocks
    blocks: int

    def grid(self, c: int) -> Tuple[int, int]:
        return self.mcuy * self.samp[c][1], self.mcux * self.samp[c][0]


def geometry(width: int, height: int, comps) -> Geometry:
    samp = [(1, 1)] if len(comps) == 1 else [(c[1], c[2]) for c in comps]
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    mcux, mcuy = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    base, at = [], 0
    for h, v in samp:
        base.append(at)
        at += mcux * h * mcuy * v
    return Geometry(len(comps), hmax, vmax, mcux, mcuy, samp, base, at)


# ----------------------------------------------------------------------------- step 1: the entropy decode
def code_strings(counts, values) -> Dict[str, int]:
    """The canonical code of a (16 counts, values) table as bit strings (T.81 C.2)."""
    table, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            if k < len(values):
                table[format(code, f"0{ln}b")] = values[k]
            k += 1
            code += 1
        code <<= 1
    return table


def unstuff(seg: bytes) -> bytes:
    """FF 00 is one FF data byte; an FF followed by anything else, or by nothing, ends the data."""
    out, i = bytearray(), 0
    while i < len(seg):
        b = seg[i]
        if b == 0xFF:
            if i + 1 < len(seg) and seg[i + 1] == 0:
                out.append(0xFF)
                i += 2
                continue
            break
        out.append(b)
        i += 1
    return bytes(out)


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


class _Bits:
    def __init__(self, payload: bytes):
        self.bits = "".join(format(b, "08b") for b in payload)
        self.pos = 0

    def symbol(self, table: Dict[str, int]) -> int:
        for ln in range(1, 17):
            if self.pos + ln > len(self.bits):
                raise _Stop(E_BITS)
            s = table.get(self.bits[self.pos:self.pos + ln])
            if s is not None:
                self.pos += ln
                return s
        raise _Stop(E_CODE)

    def receive(self, t: int) -> int:
        if t == 0:
            return 0
        if self.pos + t > len(self.bits):
            raise _Stop(E_BITS)
        v = int(self.bits[self.pos:self.pos + t], 2)
        self.pos += t
        return v


def _extend(v: int, t: int, mutant) -> int:
    if t == 0:
        return 0
    if v >= 1 << (t - 1):
        return v
    return v - (1 << t) + (0 if mutant == "extend_off_by_one" else 1)


def entropy_decode(w: Walk, mutant: Optional[str] = None, symbols: Optional[list] = None):
    """Dequantised coefficients int64 [blocks, 64] in natural order, in the device's block order (component by component,
    each a row-major grid of whole MCUs), and one (status, MCUs done) per segment.  `symbols`, if a list, counts the
    Huffman symbols decoded in its element 0."""
    g = geometry(w.width, w.height, w.comps)
    coef = np.zeros((g.blocks, 64), np.int64)
    total = g.mcux * g.mcuy
    per = w.ri if w.ri else total
    zz = [(z % 8) * 8 + z // 8 for z in ZIGZAG] if mutant == "zigzag_transposed" else ZIGZAG
    tables = [(code_strings(*w.dc[d]), code_strings(*w.ac[a])) for _, d, a in w.scan]
    status, pred, nsym = [], [0] * len(w.scan), 0
    for s, seg in enumerate(w.segments):
        bits = _Bits(unstuff(seg))
        first = s * per
        count = max(0, min(per, total - first))
        if mutant != "dc_no_reset":
            pred = [0] * len(w.scan)
        done, code = 0, OK
        try:
            for m in range(first, first + count):
                my, mx = divmod(m, g.mcux)
                for k, (ci, _, _) in enumerate(w.scan):
                    h, v = g.samp[ci]
                    q = w.qt[w.comps[ci][3]]
                    for vy in range(v):
                        for hx in range(h):
                            blk = coef[g.base[ci] + (my * v + vy) * g.mcux * h + mx * h + hx]
                            t = bits.symbol(tables[k][0]) & 15
                            nsym += 1
                            pred[k] += _extend(bits.receive(t), t, mutant)
                            val = pred[k] * int(q[0])
                            if not -32768 <= val <= 32767:
                                raise _Stop(E_RANGE)
                            blk[0] = val
                            i = 1
                            while i <= 63:
                                rs = bits.symbol(tables[k][1])
                                nsym += 1
                                r, sz = rs >> 4, rs & 15
                                if sz == 0:
                                    if r != 15:
                                        break
                                    i += 16
                                    continue
                                i += r
                                if i > 63:
                                    raise _Stop(E_INDEX)
                                val = _extend(bits.receive(sz), sz, mutant) * int(q[zz[i]])
                                if not -32768 <= val <= 32767:
                                    raise _Stop(E_RANGE)
                                blk[zz[i]] = val
                                i += 1
                done += 1
        except _Stop as stop:
            code = stop.status
        status.append((code, done))
    if symbols is not None:
        symbols[0] = nsym
    return coef, status, g


# ----------------------------------------------------------------------------- step 2: the IDCT
def _pass(v, s: int, rounding: bool = True):
    """One 8-point pass over the last axis, descaled by s bits."""
    v0, v1, v2, v3, v4, v5, v6, v7 = (v[..., i] for i in range(8))
    z1 = (v2 + v6) * 4433
    t2 = z1 - v6 * 15137
    t3 = z1 + v2 * 6270
    t0 = (v0 + v4) << 13
    t1 = (v0 - v4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = v7, v5, v3, v1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], axis=-1)
    return (out + ((1 << (s - 1)) if rounding else 0)) >> s


def idct_blocks(coef: np.ndarray, mutant: Optional[str] = None, clamps: Optional[set] = None) -> np.ndarray:
    """int64 [n, 64] dequantised coefficients -> uint8 [n, 8, 8] samples.  Exact: |coefficient| <= 32768 keeps every
    intermediate far inside int64."""
    b = coef.reshape(-1, 8, 8).astype(np.int64)
    ws = _pass(b.transpose(0, 2, 1), 11, mutant != "column_no_round").transpose(0, 2, 1)   # columns first
    x = _pass(ws, 18)
    x = ((x + 512) % 1024) - 512 + 128
    if clamps is not None:
        if (x < 0).any():
            clamps.add("idct-low")
        if (x > 255).any():
            clamps.add("idct-high")
    return np.clip(x, 0, 255).astype(np.uint8)


def planes_from_blocks(samples: np.ndarray, g: Geometry) -> List[np.ndarray]:
    planes = []
    for c in range(g.ncomp):
        rows, cols = g.grid(c)
        blk = samples[g.base[c]:g.base[c] + rows * cols].reshape(rows, cols, 8, 8)
        planes.append(blk.transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8))
    return planes


# ----------------------------------------------------------------------------- step 3: chroma upsampling
def _neighbours(p: np.ndarray, axis: int, first_zero: bool = False):
    before = np.concatenate([np.take(p, [0], axis), np.take(p, range(p.shape[axis] - 1), axis)], axis)
    after = np.concatenate([np.take(p, range(1, p.shape[axis]), axis), np.take(p, [p.shape[axis] - 1], axis)], axis)
    if first_zero:
        before = before.copy()
        before[(slice(None),) * axis + (0,)] = 0
    return before, after


def upsample_h2v1(p: np.ndarray, mutant: Optional[str] = None) -> np.ndarray:
    """Fancy (triangle) upsampling of a [rows, cw] plane to [rows, 2 cw]; the first output of a row is p[0] and the last
    p[last], which is what a replicated neighbour gives.  libjpeg replicates instead where cw <= 2."""
    p = p.astype(np.int64)
    if p.shape[1] <= 2:
        return np.repeat(p, 2, axis=1)
    left, right = _neighbours(p, 1, first_zero=mutant == "h2v1_first")
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    return out


def upsample_h2v2(p: np.ndarray, mutant: Optional[str] = None) -> np.ndarray:
    p = p.astype(np.int64)
    if p.shape[1] <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    above, below = _neighbours(p, 0)
    r = np.empty((2 * p.shape[0], p.shape[1]), np.int64)
    r[0::2] = 3 * p + above
    r[1::2] = 3 * p + below
    left, right = _neighbours(r, 1)
    ke, ko = (7, 8) if mutant == "h2v2_round_swapped" else (8, 7)
    out = np.empty((r.shape[0], 2 * r.shape[1]), np.int64)
    out[:, 0::2] = (3 * r + left + ke) >> 4
    out[:, 1::2] = (3 * r + right + ko) >> 4
    return out


# ----------------------------------------------------------------------------- step 4: colour
def colour(y, cb, cr, mutant: Optional[str] = None, clamps: Optional[set] = None) -> np.ndarray:
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    gg = y + ((-22554 * cb - 46802 * cr + (0 if mutant == "g_no_round" else 32768)) >> 16)
    rgb = np.stack([r, gg, b], axis=-1)
    if clamps is not None:
        if (rgb < 0).any():
            clamps.add("colour-low")
        if (rgb > 255).any():
            clamps.add("colour-high")
    return np.clip(rgb, 0, 255).astype(np.uint8)


@dataclass
class Decoded:
    status: int                              # the first defective segment's code, or OK
    pixels: np.ndarray                       # uint8 [H, W, channels]
    seg_status: List[Tuple[int, int]]        # (code, MCUs done) per segment
    coef: np.ndarray                         # int64 [blocks, 64]
    geometry: Geometry
    clamps: set = field(default_factory=set)
    symbols: int = 0


def decode(data: bytes, order: str = "rgb", channels: int = 3, mutant: Optional[str] = None) -> Decoded:
    w = walk(data)
    nsym = [0]
    coef, seg_status, g = entropy_decode(w, mutant, nsym)
    clamps = set()
    planes = planes_from_blocks(idct_blocks(coef, mutant, clamps), g)
    H, W = w.height, w.width
    if g.ncomp == 1:
        gray = planes[0][:H, :W]
        pixels = gray[:, :, None] if channels == 1 else np.repeat(gray[:, :, None], 3, axis=2)
    else:
        assert channels == 3
        full = [planes[0][:H, :W]]
        for c in (1, 2):
            ph, pw = -(-H * g.samp[c][1] // g.vmax), -(-W * g.samp[c][0] // g.hmax)
            p = planes[c][:ph, :pw]
            if (g.hmax, g.vmax) == (2, 1):
                p = upsample_h2v1(p, mutant)
            elif (g.hmax, g.vmax) == (2, 2):
                p = upsample_h2v2(p, mutant)
            full.append(p[:H, :W])
        pixels = colour(full[0], full[1], full[2], mutant, clamps)
        if order == "bgr":
            pixels = pixels[:, :, ::-1]
    status = next((c for c, _ in seg_status if c), OK)
    return Decoded(status, np.ascontiguousarray(pixels), seg_status, coef, g, clamps, nsym[0])


def decode_with_pil(data: bytes, order: str = "rgb", channels: int = 3) -> np.ndarray:
    from PIL import Image
    img = Image.open(io.BytesIO(data))
    if channels == 1:
        return np.asarray(img.convert("L"))[:, :, None]
    rgb = np.asarray(img.convert("RGB"))
    return np.ascontiguousarray(rgb[:, :, ::-1]) if order == "bgr" else rgb


# ----------------------------------------------------------------------------- the writer
class _BitWriter:
    def __init__(self):
        self.bits: List[str] = []

    def put(self, v: int, n: int):
        if n:
            self.bits.append(format(v, f"0{n}b"))

    def bytes(self) -> bytes:
        s = "".join(self.bits)
        s += "1" * (-len(s) % 8)
        raw = int(s, 2).to_bytes(len(s) // 8, "big") if s else b""
        return raw.replace(b"\xff", b"\xff\x00")


def _magnitude(v: int) -> Tuple[int, int]:
    """(category, the category's bits) of a value."""
    t = abs(v).bit_length()
    return t, (v if v >= 0 else v + (1 << t) - 1)


def block_symbols(block: Sequence[int], pred: int) -> Tuple[list, int]:
    """The symbols of one block of quantised coefficients in natural order: ("dc" | "ac", symbol, bits, bit count)."""
    zzv = [int(block[z]) for z in ZIGZAG]
    t, bits = _magnitude(zzv[0] - pred)
    out = [("dc", t, bits, t)]
    run = 0
    last = max([k for k in range(1, 64) if zzv[k]], default=0)
    for k in range(1, last + 1):
        if zzv[k] == 0:
            run += 1
            continue
        while run > 15:
            out.append(("ac", 0xF0, 0, 0))
            run -= 16
        t, bits = _magnitude(zzv[k])
        out.append(("ac", run << 4 | t, bits, t))
        run = 0
    if last < 63:
        out.append(("ac", 0x00, 0, 0))
    return out, zzv[0]


def _segment(marker: int, body: bytes) -> bytes:
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


def dqt(t: int, natural, sixteen: bool = False) -> bytes:
    vals = [int(natural[z]) for z in ZIGZAG]
    body = bytes([(16 if sixteen else 0) | t]) + (b"".join(struct.pack(">H", v) for v in vals) if sixteen else bytes(vals))
    return _segment(0xDB, body)


def dht(cls: int, t: int, counts, values) -> bytes:
    return _segment(0xC4, bytes([cls << 4 | t]) + bytes(counts) + bytes(values))


JFIF = _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")


def write_jpeg(width: int, height: int, comps, qt: Dict[int, Sequence[int]], dc: Dict[int, tuple], ac: Dict[int, tuple],
               coef: Optional[List[np.ndarray]] = None, ri: int = 0, *, sof: int = 0xC0, sixteen: Sequence[int] = (),
               scan_tables=None, jfif: bool = True, fill: int = 0, edit=None, raw_segments: Optional[Dict[int, bytes]] = None,
               extra: bytes = b"", precision: int = 8) -> bytes:
    """A baseline file.  comps: (id, h, v, quantisation table) per component; coef[c]: quantised coefficients int
    [block rows, block columns, 64] in natural order over whole MCUs; scan_tables: (DC, AC) table per component, by
    default (0, 0) for the first and (1, 1) for the others.  `fill` FF bytes go in front of every RSTn and of EOI;
    `edit(segment index, symbols)` may change a segment's symbol list; `raw_segments` replaces whole segments' bytes;
    `extra` goes between the JFIF header and the tables."""
    g = geometry(width, height, comps)
    if scan_tables is None:
        scan_tables = [(0, 0)] + [(1, 1)] * (len(comps) - 1)
    out = bytearray(b"\xff\xd8")
    if jfif:
        out += JFIF
    out += extra
    for t, table in qt.items():
        out += dqt(t, table, t in sixteen)
    out += _segment(sof, bytes([precision]) + struct.pack(">HH", height, width) + bytes([len(comps)])
                    + b"".join(bytes([cid, h << 4 | v, tq]) for cid, h, v, tq in comps))
    for t, (counts, values) in dc.items():
        out += dht(0, t, counts, values)
    for t, (counts, values) in ac.items():
        out += dht(1, t, counts, values)
    if ri:
        out += _segment(0xDD, struct.pack(">H", ri))
    out += _segment(0xDA, bytes([len(comps)]) + b"".join(bytes([c[0], d << 4 | a]) for c, (d, a) in zip(comps, scan_tables))
                    + bytes([0, 63, 0]))
    codes = {("dc", t): {s: k for k, s in code_strings(*tab).items()} for t, tab in dc.items()}
    codes.update({("ac", t): {s: k for k, s in code_strings(*tab).items()} for t, tab in ac.items()})
    total = g.mcux * g.mcuy
    per = ri if ri else total
    nseg = -(-total // per)
    for s in range(nseg):
        syms, pred = [], [0] * len(comps)
        for m in range(s * per, min(total, (s + 1) * per)):
            my, mx = divmod(m, g.mcux)
            for c in range(len(comps)):
                h, v = g.samp[c]
                for vy in range(v):
                    for hx in range(h):
                        bs, pred[c] = block_symbols(coef[c][my * v + vy, mx * h + hx], pred[c])
                        syms += [(kind, scan_tables[c][kind == "ac"], sym, bits, n) for kind, sym, bits, n in bs]
        if edit is not None:
            syms = edit(s, syms)
        bw = _BitWriter()
        for kind, t, sym, bits, n in syms:
            code = codes[(kind, t)][sym]
            bw.put(int(code, 2), len(code))
            bw.put(bits, n)
        body = bw.bytes()
        if raw_segments and s in raw_segments:
            body = raw_segments[s]
        out += body + b"\xff" * fill
        out += bytes([0xFF, 0xD0 + s % 8]) if s + 1 < nseg else b"\xff\xd9"
    return bytes(out)


# ----------------------------------------------------------------------------- the corpus
WIDTHS = (1, 7, 8, 9, 16, 17, 33, 53)
HEIGHTS = (1, 8, 15, 16, 17, 37)
SAMPLINGS = ("gray", "444", "422", "420")
QUALITIES = (30, 75, 95, 100)
CONTENTS = ("flat", "noise", "ramp", "checker")
_PIL_SUB = {"444": 0, "422": 1, "420": 2}


def make_content(kind: str, h: int, w: int, c: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "flat":
        a = np.empty((h, w, c), np.uint8)
        a[:] = rng.integers(0, 256, size=c, dtype=np.uint8)
    elif kind == "noise":
        a = rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
    elif kind == "ramp":
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([(xx * 255 // max(1, w - 1) + k * 60 + yy * (k + 1) * 3) % 256 for k in range(c)], axis=2).astype(np.uint8)
    elif kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([(((yy >> k) + xx) & 1) * 255 for k in range(c)], axis=2).astype(np.uint8)
    else:
        raise ValueError(kind)
    return a


def pil_file(w: int, h: int, sampling: str, quality: int, kind: str, seed: int, **save) -> bytes:
    from PIL import Image
    c = 1 if sampling == "gray" else 3
    a = make_content(kind, h, w, c, seed)
    img = Image.fromarray(a[:, :, 0] if c == 1 else a)
    buf = io.BytesIO()
    if c == 3:
        save = dict(save, subsampling=_PIL_SUB[sampling])
    img.save(buf, "JPEG", quality=quality, **save)
    return buf.getvalue()


@dataclass(frozen=True)
class FileCase:
    name: str
    data: bytes
    w: int
    h: int
    c: int                    # components: 1 or 3
    pil_written: bool = True


@lru_cache(maxsize=None)
def pil_files() -> Tuple[FileCase, ...]:
    out, k = [], 0

    def add(name, w, h, sampling, quality, kind, **save):
        nonlocal k
        out.append(FileCase(name, pil_file(w, h, sampling, quality, kind, 100 + k, **save), w, h, 1 if sampling == "gray" else 3))
        k += 1

    for w in WIDTHS:                                   # every size, the other axes cycling
        for h in HEIGHTS:
            s, q, c = SAMPLINGS[k % 4], QUALITIES[(k // 4 + k) % 4], CONTENTS[(k // 3) % 4]
            add(f"shape-w{w}-h{h}-{s}-q{q}-{c}", w, h, s, q, c)
    for s in SAMPLINGS:                                # every sampling x quality x content at the odd size
        for q in QUALITIES:
            for c in CONTENTS:
                add(f"full-{s}-q{q}-{c}", 53, 37, s, q, c)
    for s in SAMPLINGS:                                # the small planes: chroma at most 2 samples wide
        for w in (1, 2, 3, 4, 5):
            add(f"narrow-w{w}-{s}", w, 17, s, 95, "noise")
    for s in SAMPLINGS:
        add(f"optimize-{s}", 33, 17, s, 75, "noise", optimize=True)
        add(f"restart-blocks1-{s}", 33, 37, s, 75, "noise", restart_marker_blocks=1)
        add(f"restart-blocks3-{s}", 53, 17, s, 95, "ramp", restart_marker_blocks=3)
        add(f"restart-rows1-{s}", 53, 37, s, 75, "checker", restart_marker_rows=1)
    return tuple(out)


@lru_cache(maxsize=None)
def std_tables():
    """The tables PIL writes without `optimize` (Annex K), read from one of its files."""
    w = walk(pil_file(16, 16, "444", 75, "noise", 1))
    return w.qt, w.dc, w.ac


ONES_CODE = ([1] * 7 + [2] + [0] * 8)        # a complete code of 9 symbols: the last is eight 1 bits
SIXTEEN_CODE = ([1] * 16)                    # codes 0, 10, 110, ...: the last has 16 bits


def _random_coef(rng, rows: int, cols: int, density: float, amp: int) -> np.ndarray:
    c = rng.integers(-amp, amp + 1, size=(rows, cols, 64))
    c[rng.random((rows, cols, 64)) > density] = 0
    c[..., 0] = rng.integers(-amp, amp + 1, size=(rows, cols))
    return c


def _std_file(w, h, comps, seed, ri=0, density=0.2, amp=40, coef=None, **kw) -> bytes:
    qt, dc, ac = std_tables()
    g = geometry(w, h, comps)
    rng = np.random.default_rng(seed)
    if coef is None:
        coef = [_random_coef(rng, *g.grid(c), density, amp) for c in range(len(comps))]
    tabs = sorted({c[3] for c in comps})
    q = kw.pop("qt", {t: qt[min(t, 1)] // 4 + 1 for t in tabs})
    n = 1 if len(comps) == 1 else 2
    return write_jpeg(w, h, comps, q, kw.pop("dc", {t: dc[t] for t in range(n)}), kw.pop("ac", {t: ac[t] for t in range(n)}), coef, ri, **kw)


YCC = [(1, 1, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
YCC420 = [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
YCC422 = [(1, 2, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
GRAY = [(1, 1, 1, 0)]


@lru_cache(maxsize=None)
def written_files() -> Tuple[FileCase, ...]:
    """Streams from the statement's writer that PIL never emits."""
    out = []

    def add(name, data, w, h, c):
        out.append(FileCase(name, data, w, h, c, False))

    qt, dc, ac = std_tables()
    # a 16-bit code: category 11 of the DC table and symbol 0x11 of the AC table get the longest code
    dc16 = (SIXTEEN_CODE, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15, 11])
    ac16 = (SIXTEEN_CODE, [0x00, 0x01, 0x02, 0x03, 0x04, 0x12, 0x21, 0xF0, 0x05, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x11])
    coef = np.zeros((2, 2, 64), np.int64)
    coef[0, 0, 0], coef[0, 1, 0], coef[1, 0, 0], coef[1, 1, 0] = 1500, -200, 3, 1027
    coef[0, 0, ZIGZAG[2]], coef[1, 1, ZIGZAG[2]], coef[0, 1, 1] = 1, -1, 9
    add("code-16-bits", write_jpeg(16, 16, GRAY, {0: np.ones(64, np.int64)}, {0: dc16}, {0: ac16}, [coef]), 16, 16, 1)
    # (15,0) runs: coefficients far apart, one of them behind 33 zeros
    coef = np.zeros((1, 3, 64), np.int64)
    coef[0, 0, ZIGZAG[17]], coef[0, 0, ZIGZAG[51]], coef[0, 1, ZIGZAG[62]], coef[0, 2, ZIGZAG[16]] = 5, -7, 3, -2
    coef[0, :, 0] = (10, -10, 40)
    add("zrl-runs", _std_file(17, 8, GRAY, 0, coef=[coef]), 17, 8, 1)
    # coefficient 63 set: no EOB
    coef = _random_coef(np.random.default_rng(5), 2, 2, 0.3, 20)
    coef[..., 63] = ((3, -1), (2, 7))
    add("no-eob", _std_file(9, 16, GRAY, 0, coef=[coef]), 9, 16, 1)
    # FF 00 as the first and as the last data byte of every segment: DC category 0 and EOB are both eight 1 bits
    ones_dc = (ONES_CODE, [1, 2, 3, 4, 5, 6, 7, 8, 0])
    ones_ac = (ONES_CODE, [0x01, 0x02, 0x11, 0x03, 0x21, 0x12, 0x04, 0xF0, 0x00])
    coef = np.zeros((1, 4, 64), np.int64)
    data = write_jpeg(32, 8, GRAY, {0: np.full(64, 2, np.int64)}, {0: ones_dc}, {0: ones_ac}, [coef], ri=1)
    assert walk(data).segments[0] == b"\xff\x00\xff\x00"
    add("ff00-first-and-last", data, 32, 8, 1)
    # fill FFs before RSTn and before EOI; 11 intervals, so RSTn wraps past 7
    add("fill-and-wrap", _std_file(53, 33, YCC420, 7, ri=1, fill=2), 53, 33, 3)
    add("wrap-444", _std_file(53, 15, YCC, 8, ri=1, fill=1), 53, 15, 3)
    # SOF1 with a 16-bit table
    q16 = {0: np.concatenate([np.full(63, 20), [300]]).astype(np.int64), 1: qt[1]}
    add("sof1-16-bit-table", _std_file(17, 17, YCC422, 9, sof=0xC1, sixteen=(0,), qt=q16, amp=3, density=0.1), 17, 17, 3)
    # component ids in another order (still Y, Cb, Cr by position) and other table numbers
    comps = [(7, 2, 2, 2), (1, 1, 1, 3), (4, 1, 1, 3)]
    add("other-ids-and-tables", _std_file(33, 16, comps, 10, ri=2, dc={1: dc[0], 3: dc[1]}, ac={0: ac[0], 2: ac[1]},
                                          scan_tables=[(1, 0), (3, 2), (3, 2)]), 33, 16, 3)
    # a gray file that declares 2x2 sampling: a single component is not interleaved, its blocks run row by row
    add("gray-declares-2x2", _std_file(17, 17, [(1, 2, 2, 0)], 11, ri=2), 17, 17, 1)
    return tuple(out)


@lru_cache(maxsize=None)
def files() -> Tuple[FileCase, ...]:
    return pil_files() + written_files()


SEGMENT_COUNTS = (1, 63, 64, 65, 130)


@lru_cache(maxsize=None)
def extra_files() -> Tuple[FileCase, ...]:
    """The larger cases of the GPU tests and the host check: segment counts around the width of a wave in one launch,
    and one long serial segment (256 x 256, 4:2:0, noise, quality 95, no restart markers)."""
    out = [FileCase(f"segments-{n}", _std_file(8 * n, 8, GRAY, 50 + n, ri=1, density=0.3), 8 * n, 8, 1, False) for n in SEGMENT_COUNTS]
    out.append(FileCase("long-segment", pil_file(256, 256, "420", 95, "noise", 60), 256, 256, 3))
    return tuple(out)


@lru_cache(maxsize=None)
def decoded(name: str, order: str = "rgb", channels: int = 3) -> Decoded:
    """The statement's result for a case of the corpus by name, computed once."""
    case = next(c for c in files() + extra_files() + malformed_files() if c.name == name)
    return decode(case.data, order, channels)


@dataclass(frozen=True)
class BadFile:
    name: str
    data: bytes
    status: int               # what the device reports (0: the host refuses the file)
    w: int = 0
    h: int = 0
    c: int = 0
    error: type = IOError
    match: str = ""


def _cut_segment(data: bytes, index: int, drop: int) -> bytes:
    """The file with the last `drop` bytes of segment `index` removed."""
    w = walk(data)
    end = w.offsets[index] + len(w.segments[index])
    return data[:end - drop] + data[end:]


@lru_cache(maxsize=None)
def malformed_files() -> Tuple[BadFile, ...]:
    """Files the host accepts and only the device can tell, then files the host refuses."""
    out = []
    qt, dc, ac = std_tables()
    # sixteen 1 bits: no code of the standard DC table
    out.append(BadFile("no-code", _std_file(16, 8, GRAY, 20, ri=1, raw_segments={1: b"\xff\x00\xff\x00"}), E_CODE, 16, 8, 1))

    def past_63(s, syms):
        return syms[:1] + [("ac", 0, 0xF1, 1, 1)] * 4 + [("ac", 0, 0x01, 1, 1)] if s == 2 else syms
    out.append(BadFile("index-past-63", _std_file(33, 8, GRAY, 21, ri=1, edit=past_63), E_INDEX, 33, 8, 1))
    out.append(BadFile("zrl-then-store-past-63", _std_file(8, 8, GRAY, 22, edit=lambda s, syms: syms[:1] + [("ac", 0, 0xF0, 0, 0)] * 3 + [("ac", 0, 0xF1, 1, 1)]),
                       E_INDEX, 8, 8, 1))
    good = _std_file(33, 17, YCC420, 23, ri=1)
    out.append(BadFile("bits-run-out", _cut_segment(good, 3, 2), E_BITS, 33, 17, 3))
    out.append(BadFile("empty-segment", _cut_segment(good, 1, len(walk(good).segments[1])), E_BITS, 33, 17, 3))
    big = {0: np.full(64, 65535, np.int64)}
    out.append(BadFile("dc-out-of-range", _std_file(16, 8, GRAY, 24, sof=0xC1, sixteen=(0,), qt=big, amp=3, density=0.0), E_RANGE, 16, 8, 1))
    acbig = {0: np.concatenate([[1], np.full(63, 40000)]).astype(np.int64)}
    out.append(BadFile("ac-out-of-range", _std_file(8, 8, GRAY, 25, sof=0xC1, sixteen=(0,), qt=acbig, amp=2, density=0.5), E_RANGE, 8, 8, 1))
    # two defects: the first in segment order wins
    two = _std_file(53, 8, GRAY, 26, ri=1, edit=lambda s, syms: past_63(2, syms) if s == 4 else syms, raw_segments={5: b"\xff\x00\xff\x00"})
    out.append(BadFile("two-defects", two, E_INDEX, 53, 8, 1))
    # ---- refused by parse_jpeg: valid JPEG that is not built (ValueError naming the feature)
    base = _std_file(16, 16, YCC, 30)
    sof_at = base.index(b"\xff\xc0")

    def patched(at, byte):
        return base[:at] + bytes([byte]) + base[at + 1:]

    def refuse(name, data, match):
        out.append(BadFile(name, data, 0, error=ValueError, match=match))

    refuse("progressive", pil_file(16, 16, "444", 75, "noise", 3, progressive=True), "progressive")
    refuse("lossless", patched(sof_at + 1, 0xC3), "lossless")
    refuse("arithmetic", patched(sof_at + 1, 0xC9), "arithmetic")
    sof1 = patched(sof_at + 1, 0xC1)
    refuse("twelve-bit", sof1[:sof_at + 4] + b"\x0c" + sof1[sof_at + 5:], "12-bit")
    refuse("two-components", _std_file(16, 16, YCC[:2], 31), "2 components")
    refuse("four-components", _std_file(8, 8, YCC + [(4, 1, 1, 0)], 32, scan_tables=[(0, 0), (1, 1), (1, 1), (0, 0)]), "4 components")
    refuse("sampling-1x2", _std_file(16, 16, [(1, 1, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)], 33), "sampling")
    refuse("chroma-2x1", _std_file(16, 16, [(1, 2, 2, 0), (2, 2, 1, 1), (3, 1, 1, 1)], 34), "sampling")
    sos_at = base.index(b"\xff\xda")
    refuse("two-scans", base[:-2] + base[sos_at:], "more than one scan")
    refuse("dnl", base[:-2] + _segment(0xDC, struct.pack(">H", 16)) + b"\xff\xd9", "DNL")
    refuse("height-0", base[:sof_at + 5] + b"\x00\x00" + base[sof_at + 7:], "height 0")
    adobe = _segment(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x00")
    refuse("adobe-transform-0", _std_file(16, 16, YCC, 35, extra=adobe), "Adobe")
    refuse("rgb-ids", _std_file(16, 16, [(82, 1, 1, 0), (71, 1, 1, 1), (66, 1, 1, 1)], 36, jfif=False), "RGB")
    # ---- refused by parse_jpeg: broken at marker level (IOError naming the file)

    def broken(name, data):
        out.append(BadFile(name, data, 0))

    broken("no-soi", b"\x00\x00" + base[2:])
    broken("no-sof", base[:sof_at] + base[sof_at + 2 + struct.unpack(">H", base[sof_at + 2:sof_at + 4])[0]:])
    broken("no-sos", base[:sos_at] + b"\xff\xd9")
    broken("no-eoi", base[:-2])
    broken("length-past-the-end", base[:sof_at - 20])
    dqt_at = base.index(b"\xff\xdb")
    broken("quantisation-table-not-defined", base[:dqt_at] + base[dqt_at + 2 + struct.unpack(">H", base[dqt_at + 2:dqt_at + 4])[0]:])
    dht_at = base.index(b"\xff\xc4")
    broken("huffman-table-not-defined", base[:dht_at] + base[dht_at + 2 + struct.unpack(">H", base[dht_at + 2:dht_at + 4])[0]:])
    broken("huffman-over-subscribed", _std_file(8, 8, GRAY, 38, dc={0: ([3] + [0] * 15, [0, 1, 2])}, coef=[np.zeros((1, 1, 64), np.int64)]))
    many = ([0] * 7 + [255, 2] + [0] * 7, list(range(256)) + [0])
    broken("huffman-more-than-256", _std_file(8, 8, GRAY, 39, ac={0: many}, coef=[np.zeros((1, 1, 64), np.int64)]))
    rst = _std_file(33, 8, GRAY, 40, ri=1)
    broken("rst-out-of-sequence", rst.replace(b"\xff\xd1", b"\xff\xd3", 1))
    broken("segment-count", rst.replace(b"\xff\xd3", b"", 1))
    broken("ff-ff-00-in-the-data", rst.replace(b"\xff\xd1", b"\xff\xd1\xff\xff\x00", 1))
    return tuple(out)


def device_bad_files() -> Tuple[BadFile, ...]:
    return tuple(b for b in malformed_files() if b.status)


# ----------------------------------------------------------------------------- the corpus for the host check
def dump(path: str) -> None:
    """Every well-formed and every device-level malformed file as tools/jpeg_decode_check.cpp reads them: the buffers
    the entry points get (the file's own bytes, the segment table, the frame descriptor, the Huffman and quantisation
    tables) and what the statement says of them (status words and coefficients)."""
    from elvis_amd import jpeg
    cases = [(f.name, f.data) for f in files() + extra_files()] + [(b.name, b.data) for b in device_bad_files()]
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for name, data in cases:
            info = jpeg.parse_jpeg(data, name)
            plan = jpeg.plan_clip([info], [len(data)])
            d = decoded(name)
            want_status = np.asarray(d.seg_status, dtype=np.uint32).reshape(-1)
            want_coef = np.zeros((plan.stride_blocks, 64), np.int16)
            want_coef[:d.coef.shape[0]] = d.coef
            fh.write(struct.pack("<I", len(name)) + name.encode())
            for blob in (data, plan.segs.tobytes(), plan.fd.tobytes(), plan.huff.tobytes(), plan.qt.tobytes(),
                         want_status.tobytes(), want_coef.tobytes()):
                fh.write(struct.pack("<I", len(blob)) + blob)
    print(f"{len(cases)} cases -> {path}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(__doc__)
