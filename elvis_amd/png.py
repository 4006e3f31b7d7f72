"""PNG frames written by the device: row filters, filter choice, symbol statistics, Huffman bit packing, Adler-32 and
CRC-32 run as HIP kernels (csrc/png.hip); the host plans the layout between the two phases and writes 45 bytes of
headers per file.  Stands where the reference's client side ends, `cv2.imwrite(...png)` (elvis.py:131-135, 4566-4579).

  encode_png_device(frames_d)            resident clip -> one complete PNG file (bytes) per frame
  save_frames_device(frames_d, paths)    the same, one download, written to `paths`
  save_frames(frames, paths, device)     host arrays, uploaded in chunks of 32 MB

The files are decodable by any PNG reader; their bytes are this build's own, NOT cv2's or PIL's (DESIGN.md 7 has the
stream: literal-only dynamic-Huffman deflate, one block and one IDAT chunk per `segment_rows` rows, one length-limited
literal code per frame).  Opt-in: `frameio.save_frame` / `save_mask` stay PIL and every directory driver writes through
PIL unless it is called with `png_writer="device"`.

`deflate="rle"` on the three functions (`png_writer="device-rle"` on the drivers) is the stream for masks and flat or
stretched frames, whose filtered bytes are nearly all 0 and which literals cannot bring under a bit a byte: a run of equal
bytes inside a 4096-byte span of a row becomes its first byte and distance-1 matches of up to 258 (csrc/png_rle.h has the
rule, include/elvis_amd.h the contract, tests/_png_rle_ref.py states it).  286 symbols, a 1222-bit block header with one
distance code of length 1, 1160 bytes of statistics a segment; everything else - filters, segments, chunks, checksums,
the two phases - is the literal path's.  The default, "literal", and its bytes are unchanged.

Synchronisation: one per clip, as for the inpainter.  Phase 1 (`elvis_png_stats`) leaves every segment's histogram and
Adler partial on the device; they are downloaded with one blocking copy on the current stream (1040 bytes a segment),
the codes, bit lengths, chunk offsets and Adler trailers are worked out here, and phase 2 (`elvis_png_pack`) writes the
chunks into one exactly sized buffer.  The host never passes over pixel or stream bytes.  tests/_png_ref.py states the
stream in numpy and Python ints; the device files equal it bit for bit.

PNG frames read by the device (csrc/png_read.hip, csrc/inflate.h), where the reference's client side starts with
`cv2.imread` (elvis.py:123-128):

  parse_png(data)                        host: signature, chunk headers and IHDR only -> PngInfo
  decode_png_device(files, device)       PNG files in memory -> resident u8 [n,H,W,channels]
  load_frames_device(paths, device)      the same from disk, uploaded in chunks
  inflate_device(streams, sizes, device) the inflater alone, on arbitrary zlib streams

8-bit, non-interlaced, colour type 0, 2 or 6 (alpha dropped); any number of IDAT chunks, any zlib stream.  The host
uploads the file bytes as they are with a table of chunk spans; IDAT gather, chunk CRC-32s, inflate, Adler-32 and the
unfilter run on the device, and one download of the per-frame status words ends a clip: IOError("Failed to load frame:
<path>") for a corrupt file, as `frameio.load_frame`.  Unsupported files raise ValueError before any launch.  Opt-in
too: `frameio.load_frame` stays PIL, and the directory drivers read through PIL unless called with
`png_reader="device"`.  tests/_png_read_ref.py states the decoder; zlib and PIL are the oracles.
"""
from __future__ import annotations

import os
import struct
import zlib
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib, ptr
from .ops import _s

MAX_CODE_LEN = 15
EOB = 256
HEADER_BITS = 1106          # 3 + 5 + 5 + 4 + 19 * 3 + 258 * 4
HEADER_WORDS = 35
STATS_STRIDE = 260          # 256 bins, Adler A, Adler B, length, 0
FRAME_TAB = 304             # 257 code entries, the Adler trailer, 35 header words, padding
TAB_ADLER, TAB_HEADER = 257, 258
ADLER_MOD = 65521
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
FILE_HEAD, FILE_TAIL = 33, 12   # signature + IHDR chunk, IEND chunk
UPLOAD_CHUNK_BYTES = 32 << 20
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_IEND = struct.pack(">I", 0) + b"IEND" + struct.pack(">I", zlib.crc32(b"IEND"))
DEFLATES = ("literal", "rle")
# deflate="rle": literals and distance-1 matches (csrc/png_rle.h, include/elvis_amd.h "PNG writer")
RLE_SPAN = 4096                 # filtered bytes of a row tokenised on their own: the pack kernel's staging tile
RLE_SYMBOLS = 286               # literals, EOB, the length symbols 257..285
RLE_HEADER_BITS = 1222          # 3 + 5 + 5 + 4 + 19 * 3 + 287 * 4
RLE_HEADER_WORDS = 39
RLE_STATS_STRIDE = 290          # 286 bins, Adler A, Adler B, length, 0
RLE_FRAME_TAB = 328             # 286 code entries, the Adler trailer, 39 header words, padding
RLE_TAB_ADLER, RLE_TAB_HEADER = 286, 287
# RFC 1951 3.2.5: extra bits of the length symbols 257..285
RLE_LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)


# ----------------------------------------------------------------------------- the literal code (host)
def limited_code_lengths(hist, max_len: int = MAX_CODE_LEN, symbols: int = 257) -> np.ndarray:
    """Code lengths (uint8 [symbols], 0 = unused) of a complete prefix code for the `symbols`-bin histogram `hist` (257:
    256 literals and EOB; 286: the length symbols too), none longer than `max_len`: package-merge, so the lengths are
    optimal under the limit and their Kraft sum is exactly 1.  Deterministic: equal counts are ordered by symbol value,
    a leaf before a package of the same weight.  EOB is always coded; a histogram with a single used symbol gets a
    second one (EOB, or literal 0 when the one symbol is EOB itself) so that the code stays complete."""
    h = np.array(hist, dtype=np.int64).reshape(-1)
    if symbols <= EOB or h.size != symbols or (h < 0).any():
        raise ValueError(f"limited_code_lengths: the histogram has {symbols} non-negative bins")
    if h[EOB] == 0:
        h[EOB] = 1
    if np.count_nonzero(h) == 1:
        h[0] = 1
    used = np.flatnonzero(h)
    n = used.size
    if n > (1 << max_len):
        raise ValueError(f"limited_code_lengths: {n} symbols do not fit in {max_len} bits")
    order = used[np.argsort(h[used], kind="stable")]          # by (count, symbol)
    leaf_w = h[order]
    leaf_v = np.eye(n, dtype=np.int32)
    pack_w = np.zeros(0, dtype=np.int64)
    pack_v = np.zeros((0, n), dtype=np.int32)
    for level in range(max_len):
        w = np.concatenate([leaf_w, pack_w])
        v = np.concatenate([leaf_v, pack_v])
        idx = np.argsort(w, kind="stable")                    # leaves come first among equal weights
        w, v = w[idx], v[idx]
        if level == max_len - 1:
            break
        m = w.size // 2 * 2
        pack_w = w[0:m:2] + w[1:m:2]
        pack_v = v[0:m:2] + v[1:m:2]
    lens = np.zeros(symbols, dtype=np.uint8)
    lens[order] = v[:2 * n - 2].sum(axis=0)
    if int(lens.max()) > max_len or sum(1 << (max_len - int(l)) for l in lens[lens > 0]) != 1 << max_len:
        raise RuntimeError("limited_code_lengths: the code is not complete")
    return lens


def canonical_codes(lengths) -> np.ndarray:
    """Deflate's canonical codes (RFC 1951 3.2.2) of a length table, most significant bit first, as uint32."""
    lens = np.asarray(lengths, dtype=np.int64)
    count = np.bincount(lens, minlength=MAX_CODE_LEN + 2)
    count[0] = 0
    nxt = np.zeros(MAX_CODE_LEN + 2, dtype=np.int64)
    code = 0
    for b in range(1, MAX_CODE_LEN + 1):
        code = (code + int(count[b - 1])) << 1
        nxt[b] = code
    codes = np.zeros(lens.size, dtype=np.uint32)
    for s, l in enumerate(lens):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


def reverse_bits(value: int, nbits: int) -> int:
    out = 0
    for _ in range(nbits):
        out = (out << 1) | (value & 1)
        value >>= 1
    return out


def code_entries(lengths) -> np.ndarray:
    """What the pack kernel looks up per symbol: (code, bit-reversed so that it goes out LSB first) << 4 | length."""
    codes = canonical_codes(lengths)
    return np.array([(reverse_bits(int(c), int(l)) << 4) | int(l) for c, l in zip(codes, lengths)], dtype=np.uint32)


def block_header_bits(lengths, final: bool = False) -> Tuple[int, int]:
    """The header of a dynamic-Huffman block for the literal code `lengths` [257] and no distance code, as (bits packed
    LSB first into a Python int, bit count = 1106): BFINAL, BTYPE 2, HLIT 257, HDIST 1, HCLEN 19, a flat code-length
    code (4 bits for the symbols 0..15, none for 16..18), then the 257 lengths and the single distance length 0 as
    4-bit codes."""
    acc, n = 0, 0

    def put(v, k):
        nonlocal acc, n
        acc |= v << n
        n += k

    put(1 if final else 0, 1)
    put(2, 2)
    put(0, 5)
    put(0, 5)
    put(15, 4)
    for s in _CL_ORDER:
        put(0 if s >= 16 else 4, 3)
    for l in list(lengths) + [0]:
        put(reverse_bits(int(l), 4), 4)
    assert n == HEADER_BITS
    return acc, n


def block_header_bits_rle(lengths, final: bool = False) -> Tuple[int, int]:
    """The header of a dynamic-Huffman block of the run-length stream for the literal/length code `lengths` [286], as
    (bits packed LSB first into a Python int, bit count = 1222): BFINAL, BTYPE 2, HLIT field 29 (286 codes), HDIST field
    0 (one distance code), HCLEN field 15, the flat 4-bit code-length code of `block_header_bits`, then the 286 lengths
    and the distance length 1 as 4-bit codes.  One distance code of length 1 is the one incomplete distance set that
    deflate allows; every match's distance is that code's single bit, 0."""
    if len(lengths) != RLE_SYMBOLS:
        raise ValueError(f"block_header_bits_rle: {RLE_SYMBOLS} code lengths, got {len(lengths)}")
    acc, n = 0, 0

    def put(v, k):
        nonlocal acc, n
        acc |= v << n
        n += k

    put(1 if final else 0, 1)
    put(2, 2)
    put(RLE_SYMBOLS - 257, 5)
    put(0, 5)
    put(15, 4)
    for s in _CL_ORDER:
        put(0 if s >= 16 else 4, 3)
    for l in list(lengths) + [1]:
        put(reverse_bits(int(l), 4), 4)
    assert n == RLE_HEADER_BITS
    return acc, n


def adler_combine(partials, start: Tuple[int, int] = (1, 0)) -> int:
    """Adler-32 of a stream from its pieces' partials (A = sum d_i, B = sum (len - i) d_i, len), in stream order."""
    a, b = start
    for pa, pb, ln in partials:
        b = (b + int(ln) % ADLER_MOD * a + int(pb)) % ADLER_MOD
        a = (a + int(pa)) % ADLER_MOD
    return (b << 16) | a


def ihdr_chunk(width: int, height: int, channels: int) -> bytes:
    body = b"IHDR" + struct.pack(">IIBBBBB", width, height, 8, 2 if channels == 3 else 0, 0, 0, 0)
    return struct.pack(">I", 13) + body + struct.pack(">I", zlib.crc32(body))


@dataclass
class PngPlan:
    """Where everything goes, from the statistics of phase 1 alone."""
    lengths: np.ndarray       # uint8 [n, 257]; [n, 286] for the run-length stream
    frame_tab: np.ndarray     # uint32 [n, FRAME_TAB]; [n, RLE_FRAME_TAB]
    chunks: np.ndarray        # int64 [n * segments, 2]: byte offset of the chunk in the output buffer, length of its data
    file_offsets: np.ndarray  # int64 [n + 1]: file f is bytes file_offsets[f] .. file_offsets[f + 1]
    adler: np.ndarray         # uint32 [n]


def plan_layout(stats: np.ndarray) -> PngPlan:
    """Codes, bit lengths, chunk offsets, file sizes and Adler trailers from stats u32 [n, segments, 260]."""
    st = np.asarray(stats, dtype=np.uint32)
    if st.ndim != 3 or st.shape[2] != STATS_STRIDE or st.shape[1] < 1:
        raise ValueError(f"plan_layout: stats must be [n, segments, {STATS_STRIDE}], got {st.shape}")
    n, nseg, _ = st.shape
    hist = st[:, :, :256].astype(np.int64)
    lengths = np.zeros((n, 257), dtype=np.uint8)
    frame_tab = np.zeros((n, FRAME_TAB), dtype=np.uint32)
    frame_hist = np.concatenate([hist.sum(axis=1), np.full((n, 1), nseg, dtype=np.int64)], axis=1)
    for f in range(n):
        lengths[f] = limited_code_lengths(frame_hist[f])
        frame_tab[f, :257] = code_entries(lengths[f])
        acc, _ = block_header_bits(lengths[f])
        frame_tab[f, TAB_HEADER:TAB_HEADER + HEADER_WORDS] = [(acc >> (32 * k)) & 0xFFFFFFFF for k in range(HEADER_WORDS)]
    ll = lengths.astype(np.int64)
    bits = HEADER_BITS + np.einsum("fsk,fk->fs", hist, ll[:, :256]) + ll[:, 256:257]
    chunks, file_offsets, adler = _lay_out(bits, st[:, :, 256:259])
    frame_tab[:, TAB_ADLER] = adler
    return PngPlan(lengths, frame_tab, chunks, file_offsets, adler)


def plan_layout_rle(stats: np.ndarray) -> PngPlan:
    """`plan_layout` for the run-length stream, from stats u32 [n, segments, 290]: one 286-symbol literal/length code per
    frame from its token histogram (EOB count = segments), the 1222-bit header, and a segment's bits as header + sum
    hist[s] * (len[s] + extra[s]) + one distance bit per match + EOB."""
    st = np.asarray(stats, dtype=np.uint32)
    if st.ndim != 3 or st.shape[2] != RLE_STATS_STRIDE or st.shape[1] < 1:
        raise ValueError(f"plan_layout_rle: stats must be [n, segments, {RLE_STATS_STRIDE}], got {st.shape}")
    n, nseg, _ = st.shape
    hist = st[:, :, :RLE_SYMBOLS].astype(np.int64)
    hist[:, :, EOB] = 0                                        # the device counts no EOB
    lengths = np.zeros((n, RLE_SYMBOLS), dtype=np.uint8)
    frame_tab = np.zeros((n, RLE_FRAME_TAB), dtype=np.uint32)
    frame_hist = hist.sum(axis=1)
    frame_hist[:, EOB] = nseg
    for f in range(n):
        lengths[f] = limited_code_lengths(frame_hist[f], symbols=RLE_SYMBOLS)
        frame_tab[f, :RLE_SYMBOLS] = code_entries(lengths[f])
        acc, _ = block_header_bits_rle(lengths[f])
        frame_tab[f, RLE_TAB_HEADER:RLE_TAB_HEADER + RLE_HEADER_WORDS] = [(acc >> (32 * k)) & 0xFFFFFFFF for k in range(RLE_HEADER_WORDS)]
    cost = lengths.astype(np.int64)
    cost[:, 257:] += np.asarray(RLE_LENGTH_EXTRA, dtype=np.int64) + 1      # a match: its extra bits and the distance bit
    bits = RLE_HEADER_BITS + np.einsum("fsk,fk->fs", hist, cost) + cost[:, EOB:EOB + 1]
    chunks, file_offsets, adler = _lay_out(bits, st[:, :, RLE_SYMBOLS:RLE_SYMBOLS + 3])
    frame_tab[:, RLE_TAB_ADLER] = adler
    return PngPlan(lengths, frame_tab, chunks, file_offsets, adler)


def _lay_out(bits: np.ndarray, partials: np.ndarray):
    """Chunk table, file offsets and Adler trailers from every segment's block bits [n, segments] (header to EOB) and its
    Adler partial (A, B, length) [n, segments, 3]."""
    n, nseg = bits.shape
    bits = bits.copy()
    bits[:, :-1] += 3                                          # the empty stored block's header
    data_len = (bits + 7) // 8 + 4                             # + 00 00 FF FF, or the Adler-32 on the last
    data_len[:, 0] += 2                                        # 78 01
    chunk_len = data_len + 12
    file_len = FILE_HEAD + chunk_len.sum(axis=1) + FILE_TAIL
    file_offsets = np.concatenate([[0], np.cumsum(file_len)]).astype(np.int64)
    within = np.cumsum(chunk_len, axis=1) - chunk_len
    chunk_off = file_offsets[:-1, None] + FILE_HEAD + within
    chunks = np.stack([chunk_off, data_len], axis=2).reshape(n * nseg, 2).astype(np.int64)
    a = np.ones(n, dtype=np.int64)
    b = np.zeros(n, dtype=np.int64)
    sa, sb, sl = (partials[:, :, k].astype(np.int64) for k in range(3))
    for s in range(nseg):
        b = (b + sl[:, s] % ADLER_MOD * a + sb[:, s]) % ADLER_MOD
        a = (a + sa[:, s]) % ADLER_MOD
    adler = ((b << 16) | a).astype(np.uint32)
    return np.ascontiguousarray(chunks), file_offsets, adler


# ----------------------------------------------------------------------------- the device forms
def _filter_code(filter) -> int:
    if isinstance(filter, str):
        if filter == "adaptive":
            return -1
    elif isinstance(filter, (int, np.integer)) and not isinstance(filter, bool) and 0 <= int(filter) <= 4:
        return int(filter)
    raise ValueError(f"png: filter must be 'adaptive' or 0..4, got {filter!r}")


def _check_deflate(deflate, who: str) -> bool:
    """deflate= of the writers: "literal" (the default: every byte its own Huffman code) or "rle" (literals and distance-1
    matches, for masks and flat frames).  True for "rle"."""
    if not isinstance(deflate, str) or deflate not in DEFLATES:
        raise ValueError(f"{who}: deflate must be one of {DEFLATES}, got {deflate!r}")
    return deflate == "rle"


def _check_clip(frames_d, order, filter, segment_rows, who: str):
    """Every argument check, before the library is touched: (n, h, w, c, order code, filter code, segment_rows)."""
    if order not in ("bgr", "rgb"):
        raise ValueError(f"{who}: order must be 'bgr' or 'rgb', got {order!r}")
    fcode = _filter_code(filter)
    if isinstance(segment_rows, bool) or not isinstance(segment_rows, (int, np.integer)) or int(segment_rows) < 1:
        raise ValueError(f"{who}: segment_rows must be an integer >= 1, got {segment_rows!r}")
    if not isinstance(frames_d, torch.Tensor) or frames_d.dtype != torch.uint8:
        raise ValueError(f"{who}: frames must be a uint8 tensor")
    if frames_d.dim() not in (3, 4):
        raise ValueError(f"{who}: frames must be [n,H,W,3], [n,H,W,1] or [n,H,W], got {tuple(frames_d.shape)}")
    if not frames_d.is_cuda:
        raise ValueError(f"{who}: frames must be resident on the device (got a '{frames_d.device}' tensor)")
    if not frames_d.is_contiguous():
        raise ValueError(f"{who}: frames must be contiguous")
    n, h, w = (int(v) for v in frames_d.shape[:3])
    c = int(frames_d.shape[3]) if frames_d.dim() == 4 else 1
    if c not in (1, 3):
        raise ValueError(f"{who}: {c} channels (C must be 1 or 3)")
    if h < 1 or w < 1:
        raise ValueError(f"{who}: empty frames {tuple(frames_d.shape)}")
    if n * h * (w * c + 1) >= 1 << 31:
        raise ValueError(f"{who}: n * H * (W * C + 1) = {n * h * (w * c + 1)} is 2^31 or more; encode the clip in parts")
    return n, h, w, c, int(order == "bgr"), fcode, int(segment_rows)


def _encode_clip(frames_d: torch.Tensor, order, filter, segment_rows, who: str, guard: int = 0, deflate: str = "literal"):
    """Both phases.  Returns (the output buffer on the device with `guard` bytes of 0xA5 on either side, the plan, the
    filter types u8 [n, H] on the device); (None, None, None) for an empty clip."""
    rle = _check_deflate(deflate, who)
    n, h, w, c, ocode, fcode, rows = _check_clip(frames_d, order, filter, segment_rows, who)
    if n == 0:
        return None, None, None
    if guard % 4:
        raise ValueError("guard must be a multiple of 4")
    dev = frames_d.device
    nseg = (h + rows - 1) // rows
    with torch.cuda.device(dev):
        stride = RLE_STATS_STRIDE if rle else STATS_STRIDE
        stats_fn, pack_fn = (lib().elvis_png_stats_rle, lib().elvis_png_pack_rle) if rle else (lib().elvis_png_stats, lib().elvis_png_pack)
        types = torch.empty(n * h, dtype=torch.uint8, device=dev)
        stats_d = torch.empty(n * nseg * stride, dtype=torch.int32, device=dev)
        check(stats_fn(ptr(frames_d), ptr(types), ptr(stats_d), n, h, w, c, ocode, fcode, rows, _s(frames_d)), dev)
        # the one synchronisation of a clip: every segment's histogram and Adler partial
        stats = stats_d.cpu().numpy().view(np.uint32).reshape(n, nseg, stride)
        plan = plan_layout_rle(stats) if rle else plan_layout(stats)
        total = int(plan.file_offsets[-1])
        chunks_d = torch.from_numpy(plan.chunks).to(dev)
        tab_d = torch.from_numpy(plan.frame_tab.view(np.int32)).to(dev)
        out = torch.empty(total + 2 * guard, dtype=torch.uint8, device=dev)
        if guard:
            out[:guard] = 0xA5
            out[guard + total:] = 0xA5
        check(pack_fn(ptr(frames_d), ptr(types), ptr(chunks_d), ptr(tab_d), ptr(out) + guard, total, n, h, w, c, ocode, rows,
                      _s(frames_d)), dev)
    return out, plan, types.view(n, h)


def _finish_files(host: np.ndarray, plan: PngPlan, h: int, w: int, c: int) -> List[np.ndarray]:
    """The host's 45 bytes per file - signature and IHDR in front, IEND behind - written into the downloaded buffer;
    returns one view per file."""
    head = np.frombuffer(PNG_SIGNATURE + ihdr_chunk(w, h, c), dtype=np.uint8)
    tail = np.frombuffer(_IEND, dtype=np.uint8)
    files = []
    for f in range(plan.file_offsets.size - 1):
        a, b = int(plan.file_offsets[f]), int(plan.file_offsets[f + 1])
        host[a:a + FILE_HEAD] = head
        host[b - FILE_TAIL:b] = tail
        files.append(host[a:b])
    return files


def _encode_to_host(frames_d, order, filter, segment_rows, who: str, deflate: str = "literal") -> List[np.ndarray]:
    out, plan, _ = _encode_clip(frames_d, order, filter, segment_rows, who, deflate=deflate)
    if out is None:
        return []
    c = int(frames_d.shape[3]) if frames_d.dim() == 4 else 1
    return _finish_files(out.cpu().numpy(), plan, int(frames_d.shape[1]), int(frames_d.shape[2]), c)


def encode_png_device(frames_d: torch.Tensor, order: str = "bgr", filter: Union[str, int] = "adaptive",
                      segment_rows: int = 16, deflate: str = "literal") -> List[bytes]:
    """One complete PNG file per frame of a resident contiguous uint8 clip [n,H,W,3], [n,H,W,1] or [n,H,W].  `order` is
    the channel order of a 3-channel clip ("bgr", what `save_frame` takes, or "rgb"); `filter` is "adaptive" (per row
    the type with the least sum of min(v, 256 - v), ties to the lower type) or one type 0..4 for every row; a frame is
    cut into deflate blocks and IDAT chunks of `segment_rows` rows.  `deflate` is "literal" (every filtered byte its own
    Huffman code: at least a bit a byte) or "rle" (runs of equal bytes inside 4096-byte spans of a row become distance-1
    matches: the stream for masks and flat or stretched frames, whose filtered bytes are nearly all 0).  A frame's bytes
    do not depend on the frames it is encoded with.  ValueError before any launch for a bad argument; an empty clip
    gives []."""
    return [v.tobytes() for v in _encode_to_host(frames_d, order, filter, segment_rows, "encode_png_device", deflate)]


def save_frames_device(frames_d: torch.Tensor, paths: Sequence, order: str = "bgr", filter: Union[str, int] = "adaptive",
                       segment_rows: int = 16, deflate: str = "literal") -> None:
    """`encode_png_device`, one download, and frame i written to paths[i]; directories are created as `save_frame`
    does."""
    _check_deflate(deflate, "save_frames_device")
    paths = list(paths)
    if not isinstance(frames_d, torch.Tensor) or frames_d.dim() < 1 or len(paths) != frames_d.shape[0]:
        raise ValueError(f"save_frames_device: {len(paths)} path(s) for the clip {tuple(getattr(frames_d, 'shape', ()))}")
    for path, view in zip(paths, _encode_to_host(frames_d, order, filter, segment_rows, "save_frames_device", deflate)):
        os.makedirs(os.path.dirname(os.fspath(path)) or ".", exist_ok=True)
        with open(path, "wb") as f:
            f.write(memoryview(view))


def save_frames(frames, paths: Sequence, device="cuda:0", *, chunk_frames=None, order: str = "bgr",
                filter: Union[str, int] = "adaptive", segment_rows: int = 16, deflate: str = "literal") -> None:
    """Host frames - uint8 (H,W,3), (H,W,1) or (H,W) arrays, a list or one [n,...] array - written as PNGs to `paths`
    through the device.  Uploaded and encoded `chunk_frames` frames at a time, by default as many as make 32 MB (5 at
    1080p); a run of equal shapes is one clip.  The files do not depend on the chunk size."""
    _check_deflate(deflate, "save_frames")
    paths = list(paths)
    if len(frames) != len(paths):
        raise ValueError(f"save_frames: {len(frames)} frame(s) for {len(paths)} path(s)")
    if chunk_frames is not None and int(chunk_frames) < 1:
        raise ValueError("chunk_frames must be at least 1")
    _check_args_only(order, filter, segment_rows)
    arrays = [np.asarray(f) for f in frames]
    for a in arrays:
        if a.dtype != np.uint8 or a.ndim not in (2, 3):
            raise ValueError(f"save_frames: frames are uint8 (H,W,3), (H,W,1) or (H,W) arrays, got {a.dtype} {a.shape}")
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
            save_frames_device(clip, paths[at:end], order, filter, segment_rows, deflate)
            at = end


def _check_args_only(order, filter, segment_rows) -> None:
    if order not in ("bgr", "rgb"):
        raise ValueError(f"save_frames: order must be 'bgr' or 'rgb', got {order!r}")
    _filter_code(filter)
    if isinstance(segment_rows, bool) or not isinstance(segment_rows, (int, np.integer)) or int(segment_rows) < 1:
        raise ValueError(f"save_frames: segment_rows must be an integer >= 1, got {segment_rows!r}")


# ----------------------------------------------------------------------------- reading
READ_CHUNK_BYTES = 512 << 20   # decoded pixels plus filtered streams of one upload chunk (41 frames at 1080p)
STATUS_NAMES = ("ok", "input exhausted", "bad zlib header", "bad block type", "stored LEN/NLEN mismatch", "bad code-length set",
                "invalid literal/length or distance symbol", "distance too far back", "output longer than the frame",
                "output shorter than the frame", "Adler-32 mismatch", "chunk CRC mismatch", "filter type above 4")
E_CRC, E_FILTER = 11, 12
_BPP = {0: 1, 2: 3, 6: 4}


@dataclass
class PngInfo:
    width: int
    height: int
    color_type: int                       # 0 gray, 2 RGB, 6 RGBA
    bpp: int                              # bytes per pixel: 1, 3 or 4
    chunks: List[Tuple[int, int, bool]]   # every chunk, IHDR and IEND included: (offset of its type field, data length, is IDAT)


def _corrupt(name) -> IOError:
    return IOError(f"Failed to load frame: {name}")


def parse_png(data, name="<bytes>") -> PngInfo:
    """Host only: the signature, the 8-byte chunk headers and IHDR of one PNG file; no stream byte is read.  ValueError
    (naming `name` and the property) for a file that is no PNG or not of the supported kind - 8-bit, non-interlaced,
    colour type 0, 2 or 6; IOError("Failed to load frame: <name>") where the chunks do not tile the file up to IEND,
    IHDR is not first, or there is no IDAT."""
    mv = memoryview(data)
    if len(mv) < 8 or bytes(mv[:8]) != PNG_SIGNATURE:
        raise ValueError(f"{name}: not a PNG file (bad signature)")
    at, chunks, ihdr, ended = 8, [], None, False
    while at + 12 <= len(mv):
        (length,) = struct.unpack(">I", mv[at:at + 4])
        kind = bytes(mv[at + 4:at + 8])
        if length >= 1 << 31 or at + 12 + length > len(mv):
            raise _corrupt(name)
        if ihdr is None:
            if kind != b"IHDR" or length != 13:
                raise _corrupt(name)
            ihdr = struct.unpack(">IIBBBBB", mv[at + 8:at + 21])
        chunks.append((at + 4, length, kind == b"IDAT"))
        at += 12 + length
        if kind == b"IEND":
            ended = True
            break
    if ihdr is None or not ended or not any(c[2] for c in chunks):
        raise _corrupt(name)
    w, h, depth, ctype, comp, filt, lace = ihdr
    if ctype == 3:
        raise ValueError(f"{name}: palette PNG (colour type 3) is not supported")
    if ctype == 4:
        raise ValueError(f"{name}: gray+alpha PNG (colour type 4) is not supported")
    if ctype not in _BPP:
        raise ValueError(f"{name}: colour type {ctype} is not supported")
    if depth != 8:
        raise ValueError(f"{name}: bit depth {depth} is not supported (8-bit only)")
    if lace != 0:
        raise ValueError(f"{name}: interlaced PNG is not supported")
    if comp != 0 or filt != 0 or w < 1 or h < 1:
        raise _corrupt(name)
    return PngInfo(int(w), int(h), int(ctype), _BPP[ctype], chunks)


def _check_read_args(order, channels, who: str) -> None:
    if order not in ("bgr", "rgb"):
        raise ValueError(f"{who}: order must be 'bgr' or 'rgb', got {order!r}")
    if isinstance(channels, bool) or channels not in (1, 3):
        raise ValueError(f"{who}: channels must be 1 or 3, got {channels!r}")


def _check_infos(infos: Sequence[PngInfo], names: Sequence, channels: int, who: str, size=None) -> Tuple[int, int]:
    """One size for all files, gray files only for channels=1, the size limit: (H, W)."""
    for info, name in zip(infos, names):
        if size is None:
            size = (info.height, info.width)
        if (info.height, info.width) != size:
            raise ValueError(f"{who}: {name} is {info.height}x{info.width}, the files before it {size[0]}x{size[1]}")
        if channels == 1 and info.bpp != 1:
            raise ValueError(f"{who}: {name} is a colour file; channels=1 is for gray files only")
    h, w = size
    total = len(infos) * h * (w * max(i.bpp for i in infos) + 1)
    if total >= 1 << 31:
        raise ValueError(f"{who}: n * H * (W * bpp + 1) = {total} is 2^31 or more; decode the clip in parts")
    return h, w


@dataclass
class _Pending:
    """A launched clip whose status words are still on the device."""
    status_d: torch.Tensor               # i32 [4 n + 2 n + nchunks]
    n: int
    caps: List[int]
    rowlens: List[int]
    chunk_frame: np.ndarray              # [nchunks] the frame of every chunk
    chunk_stream_end: np.ndarray         # [nchunks] where the chunk's payload ends in its frame's stream (0 before the first IDAT)


def _launch_decode(files: Sequence, infos: Sequence[PngInfo], frames_out: torch.Tensor, order: str, channels: int, *,
                   guard: int = 0, upload_offset: int = 0):
    """Gather, CRC check, inflate and unfilter of one clip into frames_out [n,H,W,channels] (resident, contiguous);
    nothing is downloaded.  `guard` bytes of 0xA5 go on either side of the filtered-stream buffer, and the uploaded
    bytes start `upload_offset` bytes past a dword (the tests' knobs).  Returns the _Pending and the filtered buffer
    with its guards."""
    dev = frames_out.device
    n = len(files)
    h, w = int(frames_out.shape[1]), int(frames_out.shape[2])
    if guard % 4:
        raise ValueError("guard must be a multiple of 4")
    sizes = [len(memoryview(f)) for f in files]
    file_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if int(file_off[-1]) + upload_offset >= 1 << 31:
        raise ValueError(f"decode_png_device: {int(file_off[-1])} bytes of files are 2^31 or more; decode the clip in parts")
    host = np.empty(int(file_off[-1]) + upload_offset, dtype=np.uint8)
    for f, data in enumerate(files):
        host[upload_offset + int(file_off[f]):upload_offset + int(file_off[f + 1])] = np.frombuffer(data, dtype=np.uint8)
    rows, chunk_frame, stream_end, in_spans = [], [], [], []
    stream_at = 0
    for f, info in enumerate(infos):
        start = stream_at
        for off, length, idat in info.chunks:
            rows.append((int(file_off[f]) + off, length, stream_at if idat else -1))
            if idat:
                stream_at += length
            chunk_frame.append(f)
            stream_end.append(stream_at - start)
        in_spans.append((start, stream_at - start))
    stride = (h * (w * max(i.bpp for i in infos) + 1) + 3) // 4 * 4
    caps = [h * (w * i.bpp + 1) for i in infos]
    nchunks = len(rows)
    with torch.cuda.device(dev):
        files_d = torch.from_numpy(host).to(dev)[upload_offset:]
        tables = np.concatenate([np.asarray(rows, dtype=np.int64).reshape(-1), np.asarray(in_spans, dtype=np.int64).reshape(-1),
                                 np.asarray([(f * stride, caps[f]) for f in range(n)], dtype=np.int64).reshape(-1)])
        tables_d = torch.from_numpy(tables).to(dev)
        chunks_d, in_d, out_d = tables_d[:3 * nchunks], tables_d[3 * nchunks:3 * nchunks + 2 * n], tables_d[3 * nchunks + 2 * n:]
        streams_d = torch.empty(max(stream_at, 1), dtype=torch.uint8, device=dev)
        filt_buf = torch.empty(n * stride + 2 * guard, dtype=torch.uint8, device=dev)
        if guard:
            filt_buf[:guard] = 0xA5
            filt_buf[guard + n * stride:] = 0xA5
        filt_d = filt_buf[guard:guard + n * stride]
        status_d = torch.zeros(6 * n + nchunks, dtype=torch.int32, device=dev)
        s = _s(frames_out)
        check(lib().elvis_png_gather(ptr(files_d), int(file_off[-1]), ptr(chunks_d), nchunks, ptr(streams_d), stream_at,
                                     ptr(status_d) + 24 * n, s), dev)
        check(lib().elvis_png_inflate(ptr(streams_d), stream_at, ptr(in_d), ptr(filt_d), n * stride, ptr(out_d), ptr(status_d), n, s), dev)
        frame_bytes = h * w * channels
        at = 0
        while at < n:                      # a run of files of one colour type is one launch
            end = at + 1
            while end < n and infos[end].bpp == infos[at].bpp:
                end += 1
            check(lib().elvis_png_unfilter(ptr(filt_d) + at * stride, stride, ptr(frames_out) + at * frame_bytes,
                                           ptr(status_d) + 16 * n + 8 * at, end - at, h, w, infos[at].bpp, channels, int(order == "bgr"), s), dev)
            at = end
    # the work buffers are not kept: every launch above is on the current stream, and the allocator hands a freed block only
    # to later work on that stream, so an upload chunk's work space is reused by the next chunk
    pending = _Pending(status_d, n, caps, [w * i.bpp + 1 for i in infos], np.asarray(chunk_frame), np.asarray(stream_end))
    return pending, filt_buf


def _frame_codes(pending: _Pending, status: np.ndarray) -> List[int]:
    """One status code per frame from the downloaded words; the first defect in stream order wins: a chunk whose CRC is
    wrong and whose payload begins at or before the byte the inflater stopped at, then a filter type above 4 in a row
    that was produced, then the inflater's own code."""
    n = pending.n
    inf = status[:4 * n].reshape(n, 4)
    unf = status[4 * n:6 * n].reshape(n, 2)
    crc = status[6 * n:]
    codes = []
    for f in range(n):
        code, produced, consumed = int(inf[f, 0]), int(inf[f, 1]), int(inf[f, 2])
        mine = np.flatnonzero((pending.chunk_frame == f) & (crc != 0))
        if unf[f, 0] != 0 and int(unf[f, 1]) * pending.rowlens[f] < produced:
            code = E_FILTER
        if mine.size:
            first = int(mine[0])
            begins = int(pending.chunk_stream_end[first - 1]) if first > 0 and pending.chunk_frame[first - 1] == f else 0
            if int(inf[f, 0]) in (0, 9, 10) or begins <= consumed:
                code = E_CRC
        codes.append(code)
    return codes


def _decode_clip(files: Sequence, device, order: str, channels: int, names: Optional[Sequence] = None, *, guard: int = 0,
                 upload_offset: int = 0, who: str = "decode_png_device"):
    """decode_png_device without the raise: (frames [n,H,W,channels] as a view into a buffer with `guard` bytes of 0xA5 on
    either side, that buffer, the filtered-stream buffer with its guards, one status code per frame)."""
    _check_read_args(order, channels, who)
    files = list(files)
    names = [f"<file {i}>" for i in range(len(files))] if names is None else list(names)
    if len(names) != len(files):
        raise ValueError(f"{who}: {len(names)} name(s) for {len(files)} file(s)")
    if not files:
        raise ValueError(f"{who}: no files")
    infos = [parse_png(data, name) for data, name in zip(files, names)]
    h, w = _check_infos(infos, names, channels, who)
    dev = L.resolve_device(device)
    L.require_gpu(dev)
    n = len(files)
    with torch.cuda.device(dev):
        buf = torch.empty(n * h * w * channels + 2 * guard, dtype=torch.uint8, device=dev)
        if guard:
            buf[:guard] = 0xA5
            buf[guard + n * h * w * channels:] = 0xA5
        frames = buf[guard:guard + n * h * w * channels].view(n, h, w, channels)
        pending, filt_buf = _launch_decode(files, infos, frames, order, channels, guard=guard, upload_offset=upload_offset)
        # the one synchronisation of a clip: the status words
        codes = _frame_codes(pending, pending.status_d.cpu().numpy().view(np.uint32))
    return frames, buf, filt_buf, codes


def decode_png_device(files: Sequence, device="cuda:0", order: str = "bgr", channels: int = 3, names: Optional[Sequence] = None) -> torch.Tensor:
    """PNG files in memory (bytes-like, one per frame) decoded on the device into a resident contiguous uint8
    [n,H,W,channels] tensor.  `channels=3` (the default): gray is replicated and alpha dropped, as `frameio.load_frame`
    does; `order` "bgr" (what `load_frame` gives) or "rgb".  `channels=1` is for gray files only.  All files have one
    size.  ValueError before any launch for a bad argument or an unsupported file; IOError("Failed to load frame:
    <name>") for a corrupt one (`names` default to "<file i>")."""
    names = [f"<file {i}>" for i in range(len(files))] if names is None else list(names)
    frames, _, _, codes = _decode_clip(files, device, order, channels, names)
    for name, code in zip(names, codes):
        if code:
            raise _corrupt(name)
    return frames


def load_frames_device(paths: Sequence, device="cuda:0", order: str = "bgr", channels: int = 3, chunk_frames: Optional[int] = None) -> torch.Tensor:
    """The PNG files `paths` decoded on the device into one resident contiguous uint8 [n,H,W,channels] tensor: what
    `frameio.load_frame` per file and `recompose.frames_to_device` give, without a host pass over the pixels.  The files
    are read and uploaded `chunk_frames` at a time (by default as many as make 512 MB of device work space, 41 at
    1080p); every chunk's kernels are launched before the one download of all status words.  The result does not depend
    on the chunk size.  Errors as `decode_png_device`, naming the path."""
    _check_read_args(order, channels, "load_frames_device")
    paths = list(paths)
    if not paths:
        raise ValueError("load_frames_device: no paths")
    if chunk_frames is not None and (isinstance(chunk_frames, bool) or int(chunk_frames) < 1):
        raise ValueError("chunk_frames must be at least 1")
    dev = L.resolve_device(device)
    L.require_gpu(dev)
    out, size, pendings, at = None, None, [], 0
    with torch.cuda.device(dev):
        while at < len(paths):
            files, infos = [], []
            while at + len(files) < len(paths):
                path = paths[at + len(files)]
                try:
                    with open(path, "rb") as fh:
                        data = fh.read()
                except OSError as exc:
                    raise _corrupt(path) from exc
                info = parse_png(data, path)
                size = _check_infos([info], [path], channels, "load_frames_device", size)
                files.append(data)
                infos.append(info)
                step = int(chunk_frames) if chunk_frames is not None else max(1, READ_CHUNK_BYTES // (2 * size[0] * (size[1] * 4 + 1)))
                if len(files) >= step:
                    break
            _check_infos(infos, paths[at:at + len(files)], channels, "load_frames_device", size)
            if out is None:
                if len(paths) * size[0] * size[1] * channels >= 1 << 40:
                    raise ValueError("load_frames_device: the clip is too large")
                out = torch.empty((len(paths), size[0], size[1], channels), dtype=torch.uint8, device=dev)
            pending, _ = _launch_decode(files, infos, out[at:at + len(files)], order, channels)
            pendings.append((at, pending))
            at += len(files)
        # the one synchronisation: every chunk's status words in one copy
        status = torch.cat([p.status_d for _, p in pendings]).cpu().numpy().view(np.uint32)
    pos = 0
    for start, p in pendings:
        words = p.status_d.numel()
        for f, code in enumerate(_frame_codes(p, status[pos:pos + words])):
            if code:
                raise _corrupt(paths[start + f])
        pos += words
    return out


def _inflate_clip(streams: Sequence, sizes: Sequence[int], device, *, guard: int = 0, upload_offset: int = 0):
    """The inflater alone: (the output buffer on the device with `guard` bytes of 0xA5 on either side, the offset of every
    stream's output in it, status u32 [n, 4] = code, bytes produced, bytes consumed, Adler-32)."""
    streams = list(streams)
    sizes = [int(v) for v in sizes]
    if len(streams) != len(sizes):
        raise ValueError(f"inflate_device: {len(sizes)} size(s) for {len(streams)} stream(s)")
    if any(v < 0 for v in sizes):
        raise ValueError("inflate_device: sizes must not be negative")
    if guard % 4:
        raise ValueError("guard must be a multiple of 4")
    dev = L.resolve_device(device)
    L.require_gpu(dev)
    n = len(streams)
    lens = [len(memoryview(v)) for v in streams]
    in_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum([(v + 3) // 4 * 4 for v in sizes])]).astype(np.int64)
    if int(in_off[-1]) + upload_offset >= 1 << 31 or int(out_off[-1]) >= 1 << 31:
        raise ValueError("inflate_device: 2^31 bytes or more; inflate the streams in parts")
    if n == 0:
        return None, out_off, np.zeros((0, 4), dtype=np.uint32)
    host = np.empty(int(in_off[-1]) + upload_offset, dtype=np.uint8)
    for i, v in enumerate(streams):
        host[upload_offset + int(in_off[i]):upload_offset + int(in_off[i + 1])] = np.frombuffer(v, dtype=np.uint8)
    spans = np.concatenate([np.stack([in_off[:-1], np.asarray(lens, dtype=np.int64)], axis=1).reshape(-1),
                            np.stack([out_off[:-1], np.asarray(sizes, dtype=np.int64)], axis=1).reshape(-1)])
    total = int(out_off[-1])
    with torch.cuda.device(dev):
        in_d = torch.from_numpy(host).to(dev)[upload_offset:]
        spans_d = torch.from_numpy(spans).to(dev)
        buf = torch.empty(max(total, 4) + 2 * guard, dtype=torch.uint8, device=dev)
        if guard:
            buf[:guard] = 0xA5
            buf[guard + max(total, 4):] = 0xA5
        status_d = torch.zeros(4 * n, dtype=torch.int32, device=dev)
        check(lib().elvis_png_inflate(ptr(in_d), int(in_off[-1]), ptr(spans_d), ptr(buf) + guard, total, ptr(spans_d) + 16 * n,
                                      ptr(status_d), n, _s(buf)), dev)
        status = status_d.cpu().numpy().view(np.uint32).reshape(n, 4)
    return buf, out_off, status


def inflate_device(streams: Sequence, sizes: Sequence[int], device="cuda:0") -> List[bytes]:
    """zlib streams (RFC 1950: stored, fixed and dynamic blocks in any mix) inflated on the device, one wave per stream;
    sizes[i] is the exact length of stream i's output.  IOError naming the stream and the defect otherwise."""
    buf, out_off, status = _inflate_clip(streams, sizes, device)
    if buf is None:
        return []
    for i, row in enumerate(status):
        if row[0]:
            raise IOError(f"inflate_device: stream {i}: {STATUS_NAMES[int(row[0])] if int(row[0]) < len(STATUS_NAMES) else int(row[0])}")
    host = buf.cpu().numpy()
    return [host[int(out_off[i]):int(out_off[i]) + int(sizes[i])].tobytes() for i in range(len(sizes))]
