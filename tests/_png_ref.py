"""The device PNG writer's stream (elvis_amd/png.py, csrc/png.hip) stated in numpy and Python ints - what the
device files are compared with bit for bit - and the case matrix, importable without a GPU.

The statement takes ONLY the literal code lengths from png.py's builder (any complete code of lengths <= 15 is valid; the
builder's properties are tested on their own in tests/test_png_host.py).  Everything else is written out here: the five
filters on raw neighbours, the min(v, 256 - v) heuristic, the segments, the canonical codes and the LSB-first bit
packing, the block header, the stored-block flush, and - from zlib, an oracle independent of the build - the Adler-32
trailer and the chunk CRC-32s.  `mutant=` switches on one named deviation; the host tests show that each of them yields
a file that zlib or PIL rejects or decodes to other pixels.
"""
from __future__ import annotations

import struct
import zlib
from dataclasses import dataclass, field
from functools import lru_cache
from typing import List, Optional

import numpy as np

from elvis_amd import png

MUTANTS = ("paeth_tie", "average_round", "no_flush", "bfinal_wrong", "code_not_reversed")
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def png_rows(frame: np.ndarray, order: str) -> np.ndarray:
    """[H, W * C] raw bytes of one frame ([H,W], [H,W,1] or [H,W,3]) in PNG channel order."""
    f = np.asarray(frame)
    if f.ndim == 2:
        f = f[:, :, None]
    if f.shape[2] == 3 and order == "bgr":
        f = f[:, :, ::-1]
    return np.ascontiguousarray(f).reshape(f.shape[0], -1)


def all_filters(raw: np.ndarray, bpp: int, mutant: Optional[str] = None) -> np.ndarray:
    """[5, H, R]: the row bytes under filter 0..4, predictors on the raw neighbours, 0 left of the row and above row 0."""
    x = raw.astype(np.int64)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp] if bpp < x.shape[1] else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp] if bpp < x.shape[1] else 0
    avg = (a + b + 1) // 2 if mutant == "average_round" else (a + b) // 2
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    if mutant == "paeth_tie":
        paeth = np.where((pc <= pa) & (pc <= pb), c, np.where(pb <= pa, b, a))
    else:
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - avg, x - paeth]) & 255


def choose_types(filtered: np.ndarray, filt) -> np.ndarray:
    """[H] filter types: the forced one, or per row the least sum of min(v, 256 - v) with ties to the lower type."""
    h = filtered.shape[1]
    if filt != "adaptive":
        return np.full(h, int(filt), dtype=np.int64)
    cost = np.minimum(filtered, 256 - filtered).sum(axis=2)
    return np.argmin(cost, axis=0)          # the first minimum


def filtered_stream(raw: np.ndarray, bpp: int, filt, mutant: Optional[str] = None):
    """(types [H], stream uint8 [H, R + 1]: every row's type byte and its filtered bytes)."""
    filtered = all_filters(raw, bpp, mutant)
    types = choose_types(filtered, filt)
    rows = filtered[types, np.arange(raw.shape[0])]
    return types, np.concatenate([types[:, None], rows], axis=1).astype(np.uint8)


def canonical(lengths) -> List[int]:
    """RFC 1951 3.2.2: codes in symbol order within a length, most significant bit first."""
    lens = [int(l) for l in lengths]
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for l in lens:
        out.append(nxt[l] if l else 0)
        if l:
            nxt[l] += 1
    return out


def rev(value: int, nbits: int) -> int:
    return int(format(value, f"0{nbits}b")[::-1], 2) if nbits else 0


class BitWriter:
    """LSB-first bits in a Python int."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value: int, nbits: int) -> None:
        self.acc |= value << self.n
        self.n += nbits

    def pad_to_byte(self) -> None:
        self.n = (self.n + 7) // 8 * 8

    def tobytes(self) -> bytes:
        assert self.n % 8 == 0
        return self.acc.to_bytes(self.n // 8, "little")


def pack_segment(data: np.ndarray, lengths, final: bool, mutant: Optional[str] = None) -> bytes:
    """One segment: a dynamic-Huffman block of literals only (flat 4-bit code-length code, HLIT 257, one distance code of
    length 0), EOB, and unless it is the frame's last the empty stored block that ends it on a byte boundary."""
    lens = [int(l) for l in lengths]
    codes = canonical(lens)
    w = BitWriter()
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(0, 5)                      # HLIT = 257
    w.put(0, 5)                      # HDIST = 1
    w.put(15, 4)                     # HCLEN = 19
    for s in CL_ORDER:
        w.put(4 if s < 16 else 0, 3)
    for l in lens + [0]:             # the literal lengths and the distance code's 0, code-length symbol l = code l of 4 bits
        w.put(rev(l, 4), 4)
    assert w.n == png.HEADER_BITS
    table = [(c if mutant == "code_not_reversed" else rev(c, l), l) for c, l in zip(codes, lens)]
    row = BitWriter()                # packed apart from the header so that no int grows past a segment
    for v in data.reshape(-1).tolist():
        row.put(*table[v])
    row.put(*table[256])
    w.put(row.acc, row.n)
    if not final and mutant != "no_flush":
        w.put(0, 3)
        w.pad_to_byte()
        w.put(0xFFFF0000, 32)
    w.pad_to_byte()
    return w.tobytes()


def chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


@dataclass
class Encoded:
    file: bytes
    types: np.ndarray                 # [H]
    stream: bytes                     # the filtered stream, type bytes included
    payloads: List[bytes]             # the data of every IDAT chunk
    chunk_offsets: List[int]          # of every IDAT chunk in the file
    lengths: np.ndarray = field(default=None)


def encode(frame: np.ndarray, order: str = "bgr", filt="adaptive", segment_rows: int = 16, mutant: Optional[str] = None,
           lengths=None) -> Encoded:
    """The whole file of one frame."""
    raw = png_rows(frame, order)
    h, r = raw.shape
    c = 1 if np.asarray(frame).ndim == 2 else np.asarray(frame).shape[2]
    w_px = r // c
    types, stream = filtered_stream(raw, c, filt, mutant)
    nseg = (h + segment_rows - 1) // segment_rows
    if lengths is None:
        hist = np.bincount(stream.reshape(-1), minlength=257).astype(np.int64)
        hist[256] = nseg
        lengths = png.limited_code_lengths(hist)
    final_at = 0 if mutant == "bfinal_wrong" and nseg > 1 else nseg - 1
    payloads = []
    for s in range(nseg):
        body = pack_segment(stream[s * segment_rows:(s + 1) * segment_rows], lengths, s == final_at, mutant)
        if s == 0:
            body = b"\x78\x01" + body
        if s == nseg - 1:
            body += struct.pack(">I", zlib.adler32(stream.tobytes()))
        payloads.append(body)
    out = png.PNG_SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w_px, h, 8, 2 if c == 3 else 0, 0, 0, 0))
    offsets = []
    for body in payloads:
        offsets.append(len(out))
        out += chunk(b"IDAT", body)
    out += chunk(b"IEND", b"")
    return Encoded(out, types, stream.tobytes(), payloads, offsets, np.asarray(lengths))


def parse_chunks(data: bytes):
    """[(kind, body, stored crc, offset)] of a PNG file; asserts the signature and that the chunks tile the file."""
    assert data[:8] == png.PNG_SIGNATURE
    at, out = 8, []
    while at < len(data):
        (n,) = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        out.append((kind, body, crc, at))
        at += 12 + n
    assert at == len(data)
    return out


def decode_with_pil(data: bytes, order: str = "bgr") -> np.ndarray:
    """[H,W] or [H,W,3] in the caller's channel order."""
    import io
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        im.load()
        a = np.asarray(im)
    if a.ndim == 3 and order == "bgr":
        a = a[:, :, ::-1]
    return np.ascontiguousarray(a)


# ----------------------------------------------------------------------------- contents
CONTENTS = ("zeros", "full", "noise", "hramp", "vramp", "diag", "hot", "limit")


def make_content(kind: str, n: int, h: int, w: int, c: int, seed: int) -> np.ndarray:
    """uint8 [n, h, w, c]."""
    rng = np.random.default_rng(1000 + seed)
    y, x, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    frames = []
    for f in range(n):
        if kind == "zeros":
            a = np.zeros((h, w, c), dtype=np.int64)
        elif kind == "full":
            a = np.full((h, w, c), 255, dtype=np.int64)
        elif kind == "noise":                      # every symbol, and the file is larger than the pixels
            a = rng.integers(0, 256, size=(h, w, c))
        elif kind == "hramp":
            a = x * 3 + ch * 40 + f
        elif kind == "vramp":
            a = y * 5 + ch * 40 + f
        elif kind == "diag":                       # an exact diagonal plane (Paeth predicts it) over a level with noise (Average)
            a = np.where(y < (h + 1) // 2, 3 * x + 5 * y + 17 * ch + f, 128 + rng.integers(-20, 21, size=(h, w, c)))
        elif kind == "hot":
            a = np.zeros((h, w, c), dtype=np.int64)
            a[h // 2, w // 2, :] = 255 - f
        elif kind == "limit":                      # Fibonacci counts: an unconstrained Huffman tree is deeper than 15
            fib = [1, 1]
            while sum(fib) + fib[-1] + fib[-2] <= h * w * c:
                fib.append(fib[-1] + fib[-2])
            # under filter 0 with three segments the stream's own symbols complete the series: EOB is the 3, and the h
            # type bytes 0 make up the first count above h together with pixels of value 0
            zero_at = next(i for i, k in enumerate(fib) if k > h)
            vals = np.concatenate([np.full(k - h if i == zero_at else k, 0 if i == zero_at else 7 + 9 * i + f)
                                   for i, k in enumerate(fib) if i != 3])
            a = np.full(h * w * c, 7 + 9 * (len(fib) - 1) + f)
            a[:vals.size] = vals
            a = rng.permutation(a).reshape(h, w, c)
        else:
            raise ValueError(kind)
        frames.append((a & 255).astype(np.uint8))
    return np.stack(frames)


@dataclass(frozen=True)
class Case:
    name: str
    n: int
    h: int
    w: int
    c: int
    order: str
    filt: object
    segment_rows: int
    content: str
    offset: int = 0          # the clip starts this many bytes past a dword
    squeeze: bool = False    # gray as [n, H, W]
    seed: int = 0

    def frames(self) -> np.ndarray:
        a = make_content(self.content, self.n, self.h, self.w, self.c, self.seed)
        return a[:, :, :, 0] if self.squeeze else a


WIDTHS = (1, 2, 5, 63, 64, 65, 257)
HEIGHTS = (1, 15, 16, 17, 33)
FILTERS = ("adaptive", 0, 1, 2, 3, 4)


def _cases() -> List[Case]:
    out = []
    k = 0
    # every width with every height; the other axes go round so that each value meets many shapes
    for w in WIDTHS:
        for h in HEIGHTS:
            c = (1, 3)[k % 2]
            seg = (1, 2, 16, h + 1)[(k // 2) % 4]
            out.append(Case(f"shape-w{w}-h{h}", (1, 3)[(k // 3) % 2], h, w, c, ("bgr", "rgb")[(k // 2) % 2], FILTERS[k % 6], seg,
                            ("noise", "diag", "hramp", "vramp")[k % 4], squeeze=(c == 1 and k % 4 == 0), seed=k))
            k += 1
    # every content under every filter, colour and gray, on a shape that is no multiple of anything
    for content in CONTENTS:
        for filt in FILTERS:
            c = (3, 1)[k % 2]
            out.append(Case(f"content-{content}-f{filt}", 1 + (k % 5 == 0) * 2, 33, 65, c, ("bgr", "rgb")[k % 3 == 0], filt,
                            (16, 2, 34, 1)[k % 4], content, seed=k))
            k += 1
    # the clip 1..3 bytes past a dword
    for off in (1, 2, 3):
        out.append(Case(f"offset-{off}", 3, 17, 63, (3, 1, 3)[off - 1], "bgr", "adaptive", 16, "diag", offset=off, seed=k))
        k += 1
    # paths of the kernels that no shape above takes: a row wider than one LDS tile (4096 bytes), one byte wider, and a
    # segment whose bits overflow the LDS bit buffer more than once
    out.append(Case("wide-rgb", 1, 3, 1400, 3, "bgr", "adaptive", 2, "diag", seed=k))
    out.append(Case("wide-gray-4097", 2, 2, 4097, 1, "rgb", 4, 16, "noise", seed=k + 1))
    out.append(Case("wide-bgr-noise", 1, 2, 1400, 3, "bgr", 4, 16, "noise", seed=k + 4))
    out.append(Case("wide-1080p-row", 1, 3, 1920, 3, "bgr", "adaptive", 16, "noise", seed=k + 5))
    out.append(Case("long-segment-noise", 1, 40, 257, 3, "rgb", "adaptive", 41, "noise", seed=k + 2))
    out.append(Case("limit-colour", 3, 33, 257, 3, "bgr", 0, 16, "limit", seed=k + 3))
    return out


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


@lru_cache(maxsize=None)
def expected(index: int) -> List[Encoded]:
    """The statement's files of case `index`, one per frame; computed once and shared."""
    case = CASES[index]
    return [encode(f, case.order, case.filt, case.segment_rows) for f in case.frames()]
