"""The device PNG reader's contract (elvis_amd/png.py, csrc/png_read.hip, csrc/inflate.h) stated in pure
Python, and the corpus the host and GPU tests and tools/png_inflate_check.cpp share.  Importable without a GPU.

The statement: the chunk walk, an inflater in the manner of zlib's contrib/puff (canonical count / symbol tables, one
bit at a time) that returns the reader's status codes, the bytes produced, the bytes consumed and the token count, the
unfilter, and a small fixed-Huffman token writer for streams no encoder emits.  zlib and PIL are the oracles of the
statement itself (tests/test_png_read_host.py).  `mutant=` switches on one named deviation.

    python tests/_png_read_ref.py dump FILE      writes every stream of the corpus for tools/png_inflate_check.cpp
"""
from __future__ import annotations

import io
import struct
import sys
import zlib
from dataclasses import dataclass
from functools import lru_cache
from typing import List, Optional, Sequence, Tuple

import numpy as np

if __name__ == "__main__":          # run as a script: the package lies beside tests/
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from _png_ref import BitWriter, chunk, encode, make_content, parse_chunks

OK, E_INPUT, E_HEADER, E_BTYPE, E_STORED, E_LENS, E_SYMBOL, E_DIST, E_LONG, E_SHORT, E_ADLER, E_CRC, E_FILTER = range(13)
MUTANTS = ("paeth_tie", "average_round", "no_wrap", "dist_extra_first", "code_not_reversed")
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


# ----------------------------------------------------------------------------- the inflater
class _Stop(Exception):
    def __init__(self, status):
        self.status = status


class _Bits:
    """LSB-first reader; bits past the end are zeros, and `over` says that some were taken."""

    def __init__(self, data: bytes):
        self.data, self.pos = data, 0          # pos in bits

    def peek(self, n: int) -> int:
        byte, shift = self.pos >> 3, self.pos & 7
        word = int.from_bytes(self.data[byte:byte + 4], "little")
        return (word >> shift) & ((1 << n) - 1)

    def take(self, n: int) -> int:
        v = self.peek(n)
        self.pos += n
        return v

    @property
    def over(self) -> bool:
        return self.pos > 8 * len(self.data)

    def check(self) -> None:
        if self.over:
            raise _Stop(E_INPUT)


class _Code:
    """count[len] and the symbols in canonical order; refuses what the reader refuses."""

    def __init__(self, lens: Sequence[int], is_dist: bool = False):
        self.count = [0] * 16
        for l in lens:
            self.count[l] += 1
        total = len(lens) - self.count[0]
        self.count[0] = 0
        left = 1
        for l in range(1, 16):
            left = (left << 1) - self.count[l]
            if left < 0:
                raise _Stop(E_LENS)
        if left > 0 and not (is_dist and (total == 0 or (total == 1 and self.count[1] == 1))):
            raise _Stop(E_LENS)
        self.symbols = [s for l in range(1, 16) for s, sl in enumerate(lens) if sl == l]

    def decode(self, bits: _Bits, mutant: Optional[str] = None) -> int:
        """puff's walk over the next 15 bits; nothing is consumed where they are no code."""
        word = bits.peek(15)
        code = first = index = 0
        for l in range(1, 16):
            if mutant == "code_not_reversed":
                code |= (word >> (15 - l)) & 1
            else:
                code |= (word >> (l - 1)) & 1
            c = self.count[l]
            if code - c < first:
                bits.pos += l
                bits.check()
                return self.symbols[index + code - first]
            index += c
            first = (first + c) << 1
            code <<= 1
        raise _Stop(E_INPUT if 8 * len(bits.data) < bits.pos + 15 else E_SYMBOL)


@dataclass
class Inflated:
    status: int
    out: bytes          # the bytes produced, also on an error
    consumed: int       # whole bytes the decoder took bits from, never more than the stream has
    adler: int          # of `out`
    tokens: int         # literals and matches


def inflate(stream: bytes, cap: int, mutant: Optional[str] = None) -> Inflated:
    """The zlib stream `stream` into at most `cap` bytes, with the reader's status: the first defect in stream order."""
    bits = _Bits(stream)
    out = bytearray()
    tokens = 0
    status = OK
    try:
        cmf, flg = bits.take(8), bits.take(8)
        bits.check()
        if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf * 256 + flg) % 31 or flg & 32:
            raise _Stop(E_HEADER)
        final = 0
        fixed = None
        while not final:
            final, btype = bits.take(1), bits.take(2)
            bits.check()
            if btype == 3:
                raise _Stop(E_BTYPE)
            if btype == 0:
                bits.pos = (bits.pos + 7) // 8 * 8
                length, nlen = bits.take(16), bits.take(16)
                bits.check()
                if length ^ 0xFFFF != nlen:
                    raise _Stop(E_STORED)
                at = bits.pos // 8
                if length > len(stream) - at:
                    raise _Stop(E_INPUT)
                if length > cap - len(out):
                    raise _Stop(E_LONG)
                out += stream[at:at + length]
                bits.pos += 8 * length
                continue
            if btype == 1:
                if fixed is None:
                    fixed = (_Code(FIXED_LENS), _Code([5] * 32, True))
                lit, dist = fixed
            else:
                nlit, ndist, ncode = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                bits.check()
                if nlit > 286 or ndist > 30:
                    raise _Stop(E_LENS)
                cl = [0] * 19
                for i in range(ncode):
                    cl[CL_ORDER[i]] = bits.take(3)
                bits.check()
                clcode = _Code(cl)
                lens: List[int] = []
                while len(lens) < nlit + ndist:
                    try:
                        sym = clcode.decode(bits)
                    except _Stop as stop:
                        raise _Stop(E_INPUT if stop.status == E_INPUT else E_LENS)
                    rep, val = 1, sym
                    if sym == 16:
                        rep, val = 3 + bits.take(2), lens[-1] if lens else 0
                    elif sym == 17:
                        rep, val = 3 + bits.take(3), 0
                    elif sym == 18:
                        rep, val = 11 + bits.take(7), 0
                    bits.check()
                    if (sym == 16 and not lens) or len(lens) + rep > nlit + ndist:
                        raise _Stop(E_LENS)
                    lens += [val] * rep
                if lens[256] == 0:
                    raise _Stop(E_LENS)
                lit, dist = _Code(lens[:nlit]), _Code(lens[nlit:], True)
            while True:
                sym = lit.decode(bits, mutant)
                if sym < 256:
                    if len(out) >= cap:
                        raise _Stop(E_LONG)
                    out.append(sym)
                    tokens += 1
                    continue
                if sym == 256:
                    break
                sym -= 257
                if sym >= 29:
                    raise _Stop(E_SYMBOL)
                if mutant == "dist_extra_first":
                    dsym = dist.decode(bits, mutant)
                    if dsym >= 30:
                        raise _Stop(E_SYMBOL)
                    d = DIST_BASE[dsym] + bits.take(DIST_EXTRA[dsym])
                    length = LEN_BASE[sym] + bits.take(LEN_EXTRA[sym])
                else:
                    length = LEN_BASE[sym] + bits.take(LEN_EXTRA[sym])
                    dsym = dist.decode(bits, mutant)
                    if dsym >= 30:
                        raise _Stop(E_SYMBOL)
                    d = DIST_BASE[dsym] + bits.take(DIST_EXTRA[dsym])
                bits.check()
                if d > len(out):
                    raise _Stop(E_DIST)
                if length > cap - len(out):
                    raise _Stop(E_LONG)
                start = len(out) - d
                for j in range(length):
                    if mutant == "no_wrap":
                        out.append(out[start + j] if start + j < start + d else 0)
                    else:
                        out.append(out[start + j % d])
                tokens += 1
        if len(out) < cap:
            raise _Stop(E_SHORT)
        bits.pos = (bits.pos + 7) // 8 * 8
        stored = 0
        for _ in range(4):
            stored = stored << 8 | bits.take(8)
        bits.check()
        if stored != zlib.adler32(bytes(out)):
            raise _Stop(E_ADLER)
    except _Stop as stop:
        status = stop.status
    return Inflated(status, bytes(out), min(len(stream), (bits.pos + 7) // 8), zlib.adler32(bytes(out)), tokens)


# ----------------------------------------------------------------------------- the fixed-Huffman token writer
def _rev(value: int, nbits: int) -> int:
    return int(format(value, f"0{nbits}b")[::-1], 2) if nbits else 0


def _fixed_lit(w: BitWriter, sym: int) -> None:
    if sym < 144:
        w.put(_rev(0x30 + sym, 8), 8)
    elif sym < 256:
        w.put(_rev(0x190 + sym - 144, 9), 9)
    elif sym < 280:
        w.put(_rev(sym - 256, 7), 7)
    else:
        w.put(_rev(0xC0 + sym - 280, 8), 8)


def length_symbol(length: int, code: Optional[int] = None) -> Tuple[int, int, int]:
    """(symbol - 257, extra bits, their value); `code` picks one where two codes reach the length (258 = code 284 + 31)."""
    if code is None:
        code = max(i for i in range(29) if LEN_BASE[i] <= length)
    return code, LEN_EXTRA[code], length - LEN_BASE[code]


def fixed_block(w: BitWriter, tokens, final: bool = True) -> None:
    """One fixed-Huffman block.  A token is a literal (int), a match (length, distance), a match with the length code
    named (length, distance, code), ("lit", symbol) for any literal/length symbol, or ("dist", length, distance symbol)."""
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    for t in tokens:
        if isinstance(t, int):
            _fixed_lit(w, t)
        elif t[0] == "lit":
            _fixed_lit(w, t[1])
        elif t[0] == "dist":
            code, nbits, extra = length_symbol(t[1])
            _fixed_lit(w, 257 + code)
            w.put(extra, nbits)
            w.put(_rev(t[2], 5), 5)
        else:
            code, nbits, extra = length_symbol(t[0], t[2] if len(t) > 2 else None)
            _fixed_lit(w, 257 + code)
            w.put(extra, nbits)
            dsym = max(i for i in range(30) if DIST_BASE[i] <= t[1])
            w.put(_rev(dsym, 5), 5)
            w.put(t[1] - DIST_BASE[dsym], DIST_EXTRA[dsym])
    _fixed_lit(w, 256)


def apply_tokens(tokens) -> bytes:
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def zlib_wrap(body: bytes, content: bytes) -> bytes:
    return b"\x78\x01" + body + struct.pack(">I", zlib.adler32(content))


def fixed_stream(tokens) -> Tuple[bytes, bytes]:
    """(zlib stream of one fixed-Huffman block, the bytes it decodes to)."""
    w = BitWriter()
    fixed_block(w, tokens)
    w.pad_to_byte()
    content = apply_tokens(tokens)
    return zlib_wrap(w.tobytes(), content), content


@lru_cache(maxsize=None)
def handbuilt() -> Tuple[bytes, bytes]:
    """32768 random literals, every length code at its least and greatest extra bits, every distance code likewise, then
    the matches at the limits: zlib's own encoder never emits a distance above 32506."""
    rng = np.random.default_rng(77)
    tokens: list = [int(v) for v in rng.integers(0, 256, size=32768)]
    for code in range(29):
        for extra in sorted({0, (1 << LEN_EXTRA[code]) - 1}):
            tokens.append((LEN_BASE[code] + extra, 1 + code, code))
    for dsym in range(30):
        for extra in sorted({0, (1 << DIST_EXTRA[dsym]) - 1}):
            tokens.append((3 + dsym % 4, DIST_BASE[dsym] + extra))
    tokens += [(258, 32768), (258, 1), (3, 32768), (5, 2), (7, 3)]
    return fixed_stream(tokens)


# ----------------------------------------------------------------------------- the PNG layer
def filter_rows(raw: np.ndarray, bpp: int, types: Sequence[int]) -> bytes:
    """The filtered stream of raw rows [H, R] under the given type per row (type bytes included)."""
    x = raw.astype(np.int64)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    f = np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]) & 255
    t = np.asarray(types, dtype=np.int64)
    rows = f[t, np.arange(x.shape[0])]
    return np.concatenate([t[:, None], rows], axis=1).astype(np.uint8).tobytes()


def unfilter(stream: bytes, h: int, w: int, bpp: int, mutant: Optional[str] = None) -> np.ndarray:
    """Raw rows uint8 [h, w * bpp] of a filtered stream of h * (1 + w * bpp) bytes, per the PNG specification: bytes left of
    the row and above row 0 are 0, Average floors, Paeth takes the nearest of a, b, c with ties in that order.  A type
    above 4 is taken as 0 (the reader reports it)."""
    rb = w * bpp
    data = np.frombuffer(stream, dtype=np.uint8).reshape(h, rb + 1)
    out = np.zeros((h, rb), dtype=np.int64)
    prev = np.zeros(rb, dtype=np.int64)
    for r in range(h):
        ft, x = int(data[r, 0]), data[r, 1:].astype(np.int64)
        if ft == 1:
            row = np.cumsum(x.reshape(w, bpp), axis=0).reshape(-1) & 255
        elif ft == 2:
            row = (x + prev) & 255
        elif ft in (3, 4):
            row = np.zeros(rb, dtype=np.int64)
            xs, ps = x.tolist(), prev.tolist()
            rs = [0] * rb
            for i in range(rb):
                a = rs[i - bpp] if i >= bpp else 0
                b = ps[i]
                if ft == 3:
                    pred = (a + b + 1) >> 1 if mutant == "average_round" else (a + b) >> 1
                else:
                    c = ps[i - bpp] if i >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    if mutant == "paeth_tie":
                        pred = c if pc <= pa and pc <= pb else (b if pb <= pa else a)
                    else:
                        pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                rs[i] = (xs[i] + pred) & 255
            row = np.asarray(rs, dtype=np.int64)
        else:
            row = x
        out[r] = row
        prev = row
    return out.astype(np.uint8)


@dataclass
class Walked:
    width: int
    height: int
    color_type: int
    bpp: int
    stream: bytes                 # the IDAT payloads, behind one another
    crc_bad_at: Optional[int]     # offset in `stream` where the first chunk with a wrong CRC begins (0 before the first IDAT)


def walk(data: bytes) -> Walked:
    """The chunk walk of a supported file: IHDR, the IDAT stream, every chunk's CRC."""
    assert data[:8] == SIGNATURE
    at, stream, bad, ihdr = 8, b"", None, None
    while at < len(data):
        (n,) = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        if zlib.crc32(kind + body) != crc and bad is None:
            bad = len(stream)
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        if kind == b"IDAT":
            stream += body
        at += 12 + n
        if kind == b"IEND":
            break
    w, h, depth, ctype = ihdr[:4]
    assert depth == 8 and ctype in (0, 2, 6) and ihdr[6] == 0
    return Walked(w, h, ctype, {0: 1, 2: 3, 6: 4}[ctype], stream, bad)


@dataclass
class Decoded:
    status: int
    pixels: Optional[np.ndarray]   # [H, W, channels] where status is 0


def decode(data: bytes, order: str = "bgr", channels: int = 3, mutant: Optional[str] = None) -> Decoded:
    """The whole reader on one file; the first defect in stream order wins: a chunk whose CRC is wrong and whose payload
    begins at or before the byte the inflater stopped at, then a filter type above 4 in a row that was produced, then
    the inflater's own status."""
    wk = walk(data)
    rowlen = 1 + wk.width * wk.bpp
    cap = wk.height * rowlen
    inf = inflate(wk.stream, cap, mutant)
    status = inf.status
    bad_rows = [r for r in range(wk.height) if r * rowlen < len(inf.out) and inf.out[r * rowlen] > 4]
    if bad_rows:
        status = E_FILTER
    if wk.crc_bad_at is not None and (inf.status in (OK, E_SHORT, E_ADLER) or wk.crc_bad_at <= inf.consumed):
        status = E_CRC
    if status:
        return Decoded(status, None)
    raw = unfilter(inf.out, wk.height, wk.width, wk.bpp, mutant).reshape(wk.height, wk.width, wk.bpp)
    if wk.bpp == 1:
        px = np.repeat(raw, channels, axis=2)
    else:
        assert channels == 3
        px = raw[:, :, :3][:, :, ::-1] if order == "bgr" else raw[:, :, :3]
    return Decoded(OK, np.ascontiguousarray(px))


def decode_with_pil(data: bytes, order: str = "bgr", channels: int = 3) -> np.ndarray:
    """What `frameio.load_frame` does ([H,W,3], gray replicated, alpha dropped), or the gray plane [H,W,1]."""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        if channels == 1:
            assert im.mode == "L"
            return np.asarray(im, dtype=np.uint8)[:, :, None].copy()
        rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return np.ascontiguousarray(rgb[:, :, ::-1] if order == "bgr" else rgb)


# ----------------------------------------------------------------------------- the corpus
COLOR_TYPE = {1: 0, 3: 2, 4: 6}
WIDTHS = (1, 2, 5, 63, 64, 65, 257)
HEIGHTS = (1, 2, 63, 64, 65, 129)
CONTENTS = ("zeros", "noise", "hramp", "vramp", "diag", "hot")      # flat, noise, ramps, diag, hot
FILTERS = (0, 1, 2, 3, 4, "mix", "pil")
STREAMS = ("stored", "fixed", "huffman", "rle", "l1", "l6", "l9", "w9", "sync", "full", "pil1", "pil6", "own")
CUTS = ("one", 1, 7, 4096, "empty-first", "empty-middle", "empty-last", "ancillary")


def compress(stream: bytes, how: str) -> bytes:
    if how in ("sync", "full"):
        co = zlib.compressobj(6)
        out = b""
        for at in range(0, len(stream), 1000):
            out += co.compress(stream[at:at + 1000]) + co.flush(zlib.Z_SYNC_FLUSH if how == "sync" else zlib.Z_FULL_FLUSH)
        return out + co.flush()
    co = {"stored": lambda: zlib.compressobj(0), "fixed": lambda: zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED),
          "huffman": lambda: zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY),
          "rle": lambda: zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE), "l1": lambda: zlib.compressobj(1),
          "l6": lambda: zlib.compressobj(6), "l9": lambda: zlib.compressobj(9), "w9": lambda: zlib.compressobj(6, zlib.DEFLATED, 9)}[how]()
    return co.compress(stream) + co.flush()


def cut_idat(stream: bytes, cut) -> List[bytes]:
    """The IDAT chunks (and, for "ancillary", the chunks in front of them) of a stream."""
    if cut == "one" or cut == "ancillary":
        parts = [stream]
    elif isinstance(cut, int):
        parts = [stream[at:at + cut] for at in range(0, len(stream), cut)]
    else:
        half = len(stream) // 2
        parts = {"empty-first": [b"", stream], "empty-middle": [stream[:half], b"", stream[half:]], "empty-last": [stream, b""]}[cut]
    out = [chunk(b"IDAT", p) for p in parts]
    if cut == "ancillary":
        out = [chunk(b"gAMA", struct.pack(">I", 45455)), chunk(b"tEXt", b"Comment\x00a text chunk in front of the data"),
               chunk(b"pHYs", struct.pack(">IIB", 2835, 2835, 1))] + out
    return out


def png_file(w: int, h: int, c: int, idat_chunks: Sequence[bytes], depth: int = 8, ctype: Optional[int] = None, lace: int = 0,
             extra: Sequence[bytes] = ()) -> bytes:
    ihdr = chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, COLOR_TYPE[c] if ctype is None else ctype, 0, 0, lace))
    return SIGNATURE + ihdr + b"".join(extra) + b"".join(idat_chunks) + chunk(b"IEND", b"")


@dataclass(frozen=True)
class FileCase:
    name: str
    data: bytes
    h: int
    w: int
    c: int                 # channels of the file: 1, 3 or 4


@dataclass(frozen=True)
class StreamCase:
    name: str
    stream: bytes
    cap: int               # the exact output size of a well-formed stream
    status: int = OK       # what zlib must agree with: 0, or a defect


def _pil_file(px: np.ndarray, level: int) -> bytes:
    from PIL import Image
    mode = {1: "L", 3: "RGB", 4: "RGBA"}[px.shape[2]]
    buf = io.BytesIO()
    Image.fromarray(px[:, :, 0] if px.shape[2] == 1 else px, mode).save(buf, "PNG", compress_level=level)
    return buf.getvalue()


def make_file(w: int, h: int, c: int, content: str, filt, how: str, cut, seed: int) -> bytes:
    px = make_content(content, 1, h, w, c, seed)[0]
    if how in ("pil1", "pil6") or filt == "pil":
        data = _pil_file(px, 1 if how == "pil1" else 6)
    elif how == "own" and c != 4:
        data = encode(px if c == 3 else px[:, :, 0], "rgb", "adaptive" if filt == "mix" else filt, 16).file
    else:
        types = [(r + seed) % 5 for r in range(h)] if filt == "mix" else [int(filt)] * h
        stream = compress(filter_rows(px.reshape(h, w * c), c, types), "l6" if how == "own" else how)
        return png_file(w, h, c, cut_idat(stream, cut))
    if cut == "one":
        return data
    # a file from another writer, its IDAT stream cut again
    chunks = parse_chunks(data)
    stream = b"".join(body for kind, body, _, _ in chunks if kind == b"IDAT")
    return png_file(w, h, c, cut_idat(stream, cut))


@lru_cache(maxsize=None)
def files() -> Tuple[FileCase, ...]:
    out, k = [], 0
    # every width with every height; the other axes go round so that each value meets many shapes
    for w in WIDTHS:
        for h in HEIGHTS:
            c = (1, 3, 4)[k % 3]
            big = w * h * c > 40000
            content = ("hramp", "diag", "vramp")[k % 3] if big else CONTENTS[k % 6]
            filt, how, cut = FILTERS[k % 7], STREAMS[(k // 2) % 13], CUTS[(k // 3) % 8]
            out.append(FileCase(f"shape-w{w}-h{h}-c{c}-{content}-f{filt}-{how}-cut{cut}", make_file(w, h, c, content, filt, how, cut, k), h, w, c))
            k += 1
    # every filter, stream kind and cut on a shape that is a multiple of nothing, every content among them
    for filt in FILTERS:
        for c in (1, 3, 4):
            content = CONTENTS[k % 6]
            out.append(FileCase(f"filter-{filt}-c{c}-{content}", make_file(65, 33, c, content, filt, ("l6", "huffman")[k % 2], "one", k), 33, 65, c))
            k += 1
    for how in STREAMS:
        c = (3, 1, 4)[k % 3]
        out.append(FileCase(f"stream-{how}-c{c}", make_file(65, 33, c, ("diag", "noise")[k % 2], ("mix", 4)[k % 2], how, "one", k), 33, 65, c))
        k += 1
    for cut in CUTS:
        c = (3, 4, 1)[k % 3]
        out.append(FileCase(f"cut-{cut}-c{c}", make_file(63, 17, c, "diag", "mix", ("l6", "pil6", "own")[k % 3], cut, k), 17, 63, c))
        k += 1
    # a stored payload over 65535 bytes: several stored blocks
    out.append(FileCase("stored-long", make_file(257, 129, 3, "noise", 0, "stored", 4096, k), 129, 257, 3))
    return tuple(out)


FILE_IDS = [f.name for f in files()]

BASE = bytes([0]) + bytes((i * 7 + i // 5) & 255 for i in range(120)) * 3        # a gray row: type 0, 360 bytes


def _dynamic_nineteen_ones() -> bytes:
    w = BitWriter()
    w.put(1, 1)
    w.put(2, 2)
    w.put(0, 5)
    w.put(0, 5)
    w.put(15, 4)
    for _ in range(19):
        w.put(1, 3)
    w.pad_to_byte()
    return b"\x78\x01" + w.tobytes() + b"\x00" * 8


@lru_cache(maxsize=None)
def malformed_streams() -> Tuple[StreamCase, ...]:
    """One defect each; zlib.decompress rejects every one (tests/test_png_read_host.py)."""
    good = compress(BASE, "l6")
    stored = compress(BASE, "stored")
    at = stored.index(struct.pack("<HH", len(BASE), len(BASE) ^ 0xFFFF))
    out = [
        StreamCase("truncated-5", good[:-5], len(BASE), E_INPUT),
        StreamCase("adler-flipped", good[:-1] + bytes([good[-1] ^ 1]), len(BASE), E_ADLER),
        StreamCase("btype-3", b"\x78\x01\x07" + b"\x00" * 8, len(BASE), E_BTYPE),
        StreamCase("stored-nlen", stored[:at + 2] + bytes([stored[at + 2] ^ 1]) + stored[at + 3:], len(BASE), E_STORED),
        StreamCase("dist-3-after-2", fixed_stream_raw([0, 1, ("raw", 3, 3)]), 8, E_DIST),
        StreamCase("dist-4-after-3", fixed_stream_raw([0, 1, 2, ("raw", 3, 4)]), 8, E_DIST),
        StreamCase("litlen-286", fixed_stream_raw([0, 1, ("lit", 286)]), 8, E_SYMBOL),
        StreamCase("dist-code-30", fixed_stream_raw([0, 1, 2, ("dist", 3, 30)]), 8, E_SYMBOL),
        StreamCase("nineteen-ones", _dynamic_nineteen_ones(), 8, E_LENS),
        StreamCase("one-byte", good[:1], len(BASE), E_INPUT),
        StreamCase("bad-header", b"\x78\x02" + good[2:], len(BASE), E_HEADER),
        StreamCase("too-long", good, len(BASE) - 1, E_LONG),
        StreamCase("too-short", good, len(BASE) + 1, E_SHORT),
    ]
    return tuple(out)


def fixed_stream_raw(tokens) -> bytes:
    """A fixed-Huffman zlib stream whose tokens need not be followable: ("raw", length, distance) is a match that is
    written but not applied."""
    w = BitWriter()
    fixed_block(w, [(t[1], t[2]) if not isinstance(t, int) and t[0] == "raw" else t for t in tokens])
    w.pad_to_byte()
    return b"\x78\x01" + w.tobytes() + b"\x00\x00\x00\x01"


@lru_cache(maxsize=None)
def good_streams() -> Tuple[StreamCase, ...]:
    """Every file's IDAT stream, the hand-built one, and an empty output."""
    out = []
    for fc in files():
        wk = walk(fc.data)
        out.append(StreamCase(fc.name, wk.stream, fc.h * (1 + fc.w * wk.bpp)))
    stream, content = handbuilt()
    out.append(StreamCase("handbuilt", stream, len(content)))
    out.append(StreamCase("empty", zlib.compress(b""), 0))
    return tuple(out)


@lru_cache(maxsize=None)
def inflated(name: str) -> Inflated:
    """The statement's result for a stream of the corpus by name; computed once and shared."""
    for sc in good_streams() + malformed_streams():
        if sc.name == name:
            return inflate(sc.stream, sc.cap)
    raise KeyError(name)


@dataclass(frozen=True)
class BadFile:
    name: str
    data: bytes
    status: int            # the reader's status; 0 where parse_png refuses the file
    error: type            # IOError from the device, or ValueError before any launch
    match: str = ""


@lru_cache(maxsize=None)
def malformed_files() -> Tuple[BadFile, ...]:
    """The malformed streams as one-row gray files, and the defects of the PNG layer."""
    out = []
    for sc in malformed_streams():
        out.append(BadFile("stream-" + sc.name, png_file(sc.cap - 1, 1, 1, [chunk(b"IDAT", sc.stream)]), sc.status, IOError))
    px = make_content("diag", 1, 9, 11, 3, 5)[0].reshape(9, 33)
    good = png_file(11, 9, 3, cut_idat(compress(filter_rows(px, 3, [r % 5 for r in range(9)]), "l6"), 7))
    chunks = parse_chunks(good)
    third = chunks[3][3]                                    # the third IDAT chunk
    n = len(chunks[3][1])
    crc_at = third + 8 + n + 3
    out.append(BadFile("crc-off-by-one", good[:crc_at] + bytes([(good[crc_at] + 1) & 255]) + good[crc_at + 1:], E_CRC, IOError))
    rows = bytearray(filter_rows(px, 3, [r % 5 for r in range(9)]))
    rows[4 * 34] = 5
    out.append(BadFile("filter-5", png_file(11, 9, 3, [chunk(b"IDAT", compress(bytes(rows), "l6"))]), E_FILTER, IOError))
    short = filter_rows(px[:8], 3, [r % 5 for r in range(8)])
    out.append(BadFile("one-row-short", png_file(11, 9, 3, [chunk(b"IDAT", compress(short, "l6"))]), E_SHORT, IOError))
    out.append(BadFile("stream-of-one-byte", png_file(11, 9, 3, [chunk(b"IDAT", b"\x78")]), E_INPUT, IOError))
    out.append(BadFile("bad-signature", b"\x89PNX" + good[4:], 0, ValueError, "signature"))
    body = compress(b"\x00" * (9 * (1 + 11 * 6)), "l6")
    out.append(BadFile("sixteen-bit", png_file(11, 9, 3, [chunk(b"IDAT", body)], depth=16), 0, ValueError, "bit depth 16"))
    out.append(BadFile("palette", png_file(11, 9, 1, [chunk(b"IDAT", compress(b"\x00" * 108, "l6"))], ctype=3,
                                           extra=[chunk(b"PLTE", bytes(range(12)))]), 0, ValueError, "palette"))
    out.append(BadFile("gray-alpha", png_file(11, 9, 1, [chunk(b"IDAT", compress(b"\x00" * (9 * 23), "l6"))], ctype=4), 0, ValueError,
                       "gray\\+alpha"))
    out.append(BadFile("interlaced", png_file(11, 9, 3, [chunk(b"IDAT", body)], lace=1), 0, ValueError, "interlaced"))
    out.append(BadFile("truncated-file", good[:-20], 0, IOError))
    return tuple(out)


def dump(path: str) -> int:
    """Every stream of the corpus with the statement's result, little-endian: count, then per case name length, name, stream
    length, stream, cap, status, bytes produced, bytes consumed, Adler-32, the bytes produced."""
    cases = good_streams() + malformed_streams()
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for sc in cases:
            r = inflated(sc.name)
            name = sc.name.encode()
            f.write(struct.pack("<I", len(name)) + name + struct.pack("<I", len(sc.stream)) + sc.stream)
            f.write(struct.pack("<IIIII", sc.cap, r.status, len(r.out), r.consumed, r.adler) + r.out)
    return len(cases)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        print(f"{dump(sys.argv[2])} streams written to {sys.argv[2]}")
    else:
        sys.exit(__doc__)
