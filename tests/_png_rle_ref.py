"""The device PNG writer's run-length stream (`deflate="rle"`: elvis_amd/png.py, csrc/png.hip, csrc/png_rle.h)
stated in numpy and Python ints - what the device files are compared with bit for bit - and its case matrix, importable
without a GPU.  Filters, filter choice, segments, chunk framing, Adler-32 and CRC-32 are tests/_png_ref.py's, imported and
not restated; this file states what differs, the contents of a segment's dynamic-Huffman block:

  tokens   a row's type byte is one literal; the row's filtered bytes are cut into spans of 4096 bytes, each tokenised on
           its own; a run of L equal bytes v inside a span is the literal v, (L - 1) // 258 matches of length 258 and, with
           r = (L - 1) % 258, one match of length r if r >= 3, else r literals v; every match has distance 1
  symbols  286 literal/length symbols by RFC 1951's table, extra bits behind the code LSB first; one distance code of
           length 1, so one distance bit, 0, ends every match
  header   HLIT field 29, HDIST field 0, HCLEN field 15, the flat 4-bit code-length code, 286 lengths and the distance
           length 1: 1222 bits

Only the code lengths come from png.py's builder, as in _png_ref.  `mutant=` switches on one named deviation; the host
tests show that zlib rejects each of them or that it gives other bytes.

    python tests/_png_rle_ref.py dump FILE      writes the spans of the edge cases with their tokens for tools/png_rle_check.cpp
"""
from __future__ import annotations

import struct
import sys
import zlib
from dataclasses import dataclass
from functools import lru_cache
from typing import List, Optional, Tuple

import numpy as np

if __name__ == "__main__":          # run as a script: the package lies beside tests/
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import _png_ref as R
from elvis_amd import png

MUTANTS = ("remainder_2_dropped", "no_distance_bit", "distance_length_0", "runs_cross_type_byte")
SPAN = 4096
HEADER_BITS = 1222
# RFC 1951 3.2.5: the length symbols 257..285
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)

# stated here, not imported: the build has to agree
assert (png.RLE_SPAN, png.RLE_HEADER_BITS, png.RLE_SYMBOLS, tuple(png.RLE_LENGTH_EXTRA)) == (SPAN, HEADER_BITS, 286, LENGTH_EXTRA)

# a token: (position in its span, symbol, extra value, extra bits); a literal has symbol < 256 and no extra bits
Token = Tuple[int, int, int, int]


def length_symbol(length: int) -> Tuple[int, int, int]:
    """(symbol, extra value, extra bits) of a match length 3..258: the last row of the table whose base is not above it."""
    assert 3 <= length <= 258
    k = max(i for i, base in enumerate(LENGTH_BASE) if base <= length)
    assert length - LENGTH_BASE[k] < 1 << LENGTH_EXTRA[k]
    return 257 + k, length - LENGTH_BASE[k], LENGTH_EXTRA[k]


def span_tokens(span, mutant: Optional[str] = None) -> List[Token]:
    """The tokens of one span (at most 4096 bytes), in stream order."""
    data = [int(v) for v in span]
    assert len(data) <= SPAN
    out, i = [], 0
    while i < len(data):
        v, j = data[i], i
        while j < len(data) and data[j] == v:
            j += 1
        out.append((i, v, 0, 0))
        at, rest = i + 1, j - i - 1
        for _ in range(rest // 258):
            out.append((at,) + length_symbol(258))
            at += 258
        r = rest % 258
        if r >= 3:
            out.append((at,) + length_symbol(r))
        elif not (mutant == "remainder_2_dropped" and r == 2):
            out.extend((at + k, v, 0, 0) for k in range(r))
        i = j
    return out


def row_tokens(row, mutant: Optional[str] = None) -> List[Token]:
    """One row of the filtered stream, type byte first: the type byte is a literal of its own, then the spans."""
    row = [int(v) for v in row]
    if mutant == "runs_cross_type_byte":        # the type byte joins the run behind it
        return span_tokens(row[:SPAN], mutant) + [t for a in range(SPAN, len(row), SPAN) for t in span_tokens(row[a:a + SPAN], mutant)]
    out = [(0, row[0], 0, 0)]
    for a in range(1, len(row), SPAN):
        out.extend(span_tokens(row[a:a + SPAN], mutant))
    return out


def segment_tokens(rows: np.ndarray, mutant: Optional[str] = None) -> List[Token]:
    return [t for row in rows for t in row_tokens(row, mutant)]


def token_histogram(tokens: List[Token]) -> np.ndarray:
    """int64 [286]: how often every literal/length symbol occurs; EOB is not counted."""
    return np.bincount([t[1] for t in tokens], minlength=286).astype(np.int64)


def header(w: R.BitWriter, lengths, final: bool, mutant: Optional[str] = None) -> None:
    lens = [int(l) for l in lengths]
    assert len(lens) == 286
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(29, 5)                     # HLIT: 286 literal/length codes
    w.put(0, 5)                      # HDIST: 1 distance code
    w.put(15, 4)                     # HCLEN: 19 code-length codes
    for s in R.CL_ORDER:
        w.put(4 if s < 16 else 0, 3)
    for l in lens + [0 if mutant == "distance_length_0" else 1]:
        w.put(R.rev(l, 4), 4)


def pack_segment(tokens: List[Token], lengths, final: bool, mutant: Optional[str] = None) -> bytes:
    """One segment: the dynamic-Huffman block of its tokens, EOB, and unless it is the frame's last the empty stored block
    that ends it on a byte boundary."""
    lens = [int(l) for l in lengths]
    codes = R.canonical(lens)
    w = R.BitWriter()
    header(w, lens, final, mutant)
    assert w.n == HEADER_BITS == png.RLE_HEADER_BITS
    body = R.BitWriter()
    for _, sym, extra, nextra in tokens:
        assert lens[sym] > 0
        body.put(R.rev(codes[sym], lens[sym]), lens[sym])
        if sym > 256:
            body.put(extra, nextra)
            if mutant != "no_distance_bit":
                body.put(0, 1)       # the one distance code, length 1
    body.put(R.rev(codes[256], lens[256]), lens[256])
    w.put(body.acc, body.n)
    if not final:
        w.put(0, 3)
        w.pad_to_byte()
        w.put(0xFFFF0000, 32)
    w.pad_to_byte()
    return w.tobytes()


def encode(frame: np.ndarray, order: str = "bgr", filt="adaptive", segment_rows: int = 16, mutant: Optional[str] = None) -> R.Encoded:
    """The whole file of one frame under deflate="rle"."""
    raw = R.png_rows(frame, order)
    h, r = raw.shape
    c = 1 if np.asarray(frame).ndim == 2 else np.asarray(frame).shape[2]
    types, stream = R.filtered_stream(raw, c, filt)
    nseg = (h + segment_rows - 1) // segment_rows
    tokens = [segment_tokens(stream[s * segment_rows:(s + 1) * segment_rows], mutant) for s in range(nseg)]
    hist = sum(token_histogram(t) for t in tokens)
    hist[256] = nseg
    lengths = png.limited_code_lengths(hist, symbols=286)
    payloads = []
    for s in range(nseg):
        body = pack_segment(tokens[s], lengths, s == nseg - 1, mutant)
        if s == 0:
            body = b"\x78\x01" + body
        if s == nseg - 1:
            body += struct.pack(">I", zlib.adler32(stream.tobytes()))
        payloads.append(body)
    out = png.PNG_SIGNATURE + R.chunk(b"IHDR", struct.pack(">IIBBBBB", r // c, h, 8, 2 if c == 3 else 0, 0, 0, 0))
    offsets = []
    for body in payloads:
        offsets.append(len(out))
        out += R.chunk(b"IDAT", body)
    out += R.chunk(b"IEND", b"")
    return R.Encoded(out, types, stream.tobytes(), payloads, offsets, np.asarray(lengths))


def segment_stats(enc: R.Encoded, h: int, rowlen: int, segment_rows: int) -> np.ndarray:
    """What phase 1 leaves for one frame: u32 [segments, 290] from the statement's filtered stream."""
    nseg = (h + segment_rows - 1) // segment_rows
    stream = np.frombuffer(enc.stream, dtype=np.uint8).reshape(h, rowlen)
    st = np.zeros((nseg, png.RLE_STATS_STRIDE), dtype=np.uint32)
    for s in range(nseg):
        rows = stream[s * segment_rows:(s + 1) * segment_rows]
        d = rows.reshape(-1).astype(np.int64)
        st[s, :286] = token_histogram(segment_tokens(rows))
        st[s, 286] = d.sum() % 65521
        st[s, 287] = int(((d.size - np.arange(d.size)) * d).sum() % 65521)
        st[s, 288] = d.size
    return st


# ----------------------------------------------------------------------------- contents and cases
RLE_CONTENTS = ("rect", "period9", "step1")


def make_content(kind: str, n: int, h: int, w: int, c: int, seed: int) -> np.ndarray:
    """uint8 [n, h, w, c]: _png_ref's kinds, a 0 / 255 rectangle mask, and the period-9 pattern aabbbcccc along a row (runs
    of 2, 3 and 4: two literals, a literal and two more, a literal and a match of 3)."""
    if kind == "rect":
        a = np.zeros((n, h, w, c), dtype=np.uint8)
        for f in range(n):
            a[f, h // 4:max(h // 4 + 1, 3 * h // 4), (w // 3 + f) % w:max(w // 3 + 1, 2 * w // 3), :] = 255
        return a
    if kind == "period9":
        vals = np.array([10, 10, 77, 77, 77, 200, 200, 200, 200], dtype=np.int64)
        y, x, ch = np.meshgrid(np.arange(h), np.arange(w * c), np.arange(1), indexing="ij")
        rows = vals[(x[:, :, 0] + y[:, :, 0]) % 9]
        return np.stack([((rows + f) & 255).astype(np.uint8).reshape(h, w, c) for f in range(n)])
    if kind == "step1":                        # under filter 1 every byte of a gray row is 1, and so is the type byte
        return np.stack([np.broadcast_to(((np.arange(w) + 1) & 255).astype(np.uint8)[None, :, None], (h, w, c)).copy() for f in range(n)])
    return R.make_content(kind, n, h, w, c, seed)


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
    offset: int = 0
    seed: int = 0

    def frames(self) -> np.ndarray:
        return make_content(self.content, self.n, self.h, self.w, self.c, self.seed)


RUN_WIDTHS = (1, 2, 3, 4, 258, 259, 260, 261, 262, 517, 518, 519, 520)     # flat rows: R = 0, 1, 2, 3, 257..261, 516..519
SPAN_WIDTHS = (4095, 4096, 4097, 4098, 4099, 4096 + 259)                    # the second span holds 1, 2, 3 and 259 bytes
HEIGHTS = (1, 15, 16, 17, 33)
FILTERS = ("adaptive", 0, 1, 2, 3, 4)
CONTENTS = ("zeros", "full", "rect", "noise", "hramp", "vramp", "diag", "period9")


def _cases() -> List[Case]:
    out = []
    # run edges: gray, forced filter 0, flat rows
    for i, w in enumerate(RUN_WIDTHS):
        out.append(Case(f"run-w{w}", 1, 2, w, 1, "rgb", 0, 16, ("full", "zeros")[i % 2]))
    # span edges: one row wider than a span; RGB 1366 is 4098 bytes
    for i, w in enumerate(SPAN_WIDTHS):
        out.append(Case(f"span-w{w}", 1, 1, w, 1, "rgb", 0, 16, ("full", "rect", "zeros")[i % 3]))
    out.append(Case("span-rgb-1366", 1, 2, 1366, 3, "bgr", "adaptive", 16, "rect"))
    out.append(Case("span-rgb-1366-period9", 1, 1, 1366, 3, "rgb", 0, 16, "period9"))
    # segments: every height with segment_rows 1, 16, H + 1
    k = 0
    for h in HEIGHTS:
        for seg in (1, 16, h + 1):
            out.append(Case(f"seg-h{h}-s{seg}", (1, 3)[k % 2], h, (37, 65)[k % 2], (1, 3)[(k // 2) % 2], ("bgr", "rgb")[k % 2],
                            FILTERS[k % 6], seg, ("rect", "period9", "diag", "zeros")[k % 4], seed=k))
            k += 1
    # every content under every filter and adaptive; a forced type 1 on flat 1s makes a type byte equal its neighbour
    for content in CONTENTS:
        for filt in FILTERS:
            out.append(Case(f"content-{content}-f{filt}", 1 + (k % 5 == 0) * 2, 17, 41, (3, 1)[k % 2], ("bgr", "rgb")[k % 3 == 0], filt,
                            (16, 5, 18, 1)[k % 4], content, seed=k))
            k += 1
    # a forced type 1 on a ramp of step 1: the type byte equals the run behind it and stays a literal of its own
    out.append(Case("type-byte-run", 1, 3, 300, 1, "rgb", 1, 2, "step1"))
    # the clip 1..3 bytes past a dword
    for off in (1, 2, 3):
        out.append(Case(f"offset-{off}", 3, 17, 63, (3, 1, 3)[off - 1], "bgr", "adaptive", 16, ("rect", "period9", "diag")[off - 1],
                        offset=off, seed=k))
        k += 1
    return out


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


@lru_cache(maxsize=None)
def expected(index: int) -> List[R.Encoded]:
    """The statement's files of case `index`, one per frame; computed once and shared."""
    case = CASES[index]
    return [encode(f, case.order, case.filt, case.segment_rows) for f in case.frames()]


# ----------------------------------------------------------------------------- the corpus of tools/png_rle_check.cpp
def check_spans() -> List[np.ndarray]:
    """Spans for the host walk of csrc/png_rle.h: every run length 1..520 alone and between other bytes, full spans, runs
    that end at the span's last byte, the period-9 pattern and noise."""
    rng = np.random.default_rng(11)
    spans = [np.full(n, 7, dtype=np.uint8) for n in range(1, 521)]
    spans += [np.concatenate([[1], np.full(n, 0), [2, 2]]).astype(np.uint8) for n in (1, 2, 3, 4, 258, 259, 260, 261, 262, 517, 518, 519, 520)]
    spans += [np.full(n, 255, dtype=np.uint8) for n in (4095, 4096)]
    spans += [np.concatenate([rng.integers(0, 256, size=4096 - n), np.full(n, 9)]).astype(np.uint8) for n in (1, 2, 3, 4, 259, 260, 261)]
    spans.append(np.array([10, 10, 77, 77, 77, 200, 200, 200, 200] * 455, dtype=np.uint8))
    spans.append(rng.integers(0, 256, size=4096, dtype=np.uint8))
    spans.append(rng.integers(0, 2, size=4096, dtype=np.uint8) * 255)
    return spans


def dump(path: str) -> None:
    """u32 count, then per span: u32 n, the n bytes, u32 tokens, and per token u32 position, symbol, extra value, extra bits
    (all little-endian)."""
    spans = check_spans()
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(spans)))
        for span in spans:
            tokens = span_tokens(span)
            f.write(struct.pack("<I", span.size) + span.tobytes() + struct.pack("<I", len(tokens)))
            for t in tokens:
                f.write(struct.pack("<4I", *t))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(__doc__)
