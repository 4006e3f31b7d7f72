"""PNG frames written by the device: row filters, filter choice, symbol statistics, Huffman bit packing, Adler-32 and
CRC-32 run as HIP kernels (csrc/png.hip); the host plans the layout between the two phases and writes 45 bytes of
headers per file.  Stands where the reference's client side ends, `cv2.imwrite(...png)` (elvis.py:131-135, 4566-4579).

  encode_png_device(frames_d)            resident clip -> one complete PNG file (bytes) per frame
  save_frames_device(frames_d, paths)    the same, one download, written to `paths`
  save_frames(frames, paths, device)     host arrays, uploaded in chunks of 32 MB

The files are decodable by any PNG reader; their bytes are this build's own, NOT cv2's or PIL's (DESIGN.md 7 has the
stream: literal-only dynamic-Huffman deflate, one block and one IDAT chunk per `segment_rows` rows, one length-limited
literal code per frame).  Opt-in: `frameio.save_frame` / `save_mask` stay PIL and every directory driver writes through
PIL unless it is called with `png_writer="device"`.  Reading stays PIL (`frameio.load_frame`).

Synchronisation: one per clip, as for the inpainter.  Phase 1 (`elvis_png_stats`) leaves every segment's histogram and
Adler partial on the device; they are downloaded with one blocking copy on the current stream (1040 bytes a segment),
the codes, bit lengths, chunk offsets and Adler trailers are worked out here, and phase 2 (`elvis_png_pack`) writes the
chunks into one exactly sized buffer.  The host never passes over pixel or stream bytes.  tests/_png_ref.py states the
stream in numpy and Python ints; the device files equal it bit for bit.
"""
from __future__ import annotations

import os
import struct
import zlib
from dataclasses import dataclass
from typing import List, Sequence, Tuple, Union

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


# ----------------------------------------------------------------------------- the literal code (host)
def limited_code_lengths(hist, max_len: int = MAX_CODE_LEN) -> np.ndarray:
    """Code lengths (uint8 [257], 0 = unused) of a complete prefix code for the 257-bin histogram `hist` (256 literals
    and EOB), none longer than `max_len`: package-merge, so the lengths are optimal under the limit and their Kraft sum
    is exactly 1.  Deterministic: equal counts are ordered by symbol value, a leaf before a package of the same weight.
    EOB is always coded; a histogram with a single used symbol gets a second one (EOB, or literal 0 when the one symbol
    is EOB itself) so that the code stays complete."""
    h = np.array(hist, dtype=np.int64).reshape(-1)
    if h.size != 257 or (h < 0).any():
        raise ValueError("limited_code_lengths: the histogram has 257 non-negative bins")
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
    lens = np.zeros(257, dtype=np.uint8)
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
    lengths: np.ndarray       # uint8 [n, 257]
    frame_tab: np.ndarray     # uint32 [n, FRAME_TAB]
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
    sa, sb, sl = (st[:, :, 256 + k].astype(np.int64) for k in range(3))
    for s in range(nseg):
        b = (b + sl[:, s] % ADLER_MOD * a + sb[:, s]) % ADLER_MOD
        a = (a + sa[:, s]) % ADLER_MOD
    adler = ((b << 16) | a).astype(np.uint32)
    frame_tab[:, TAB_ADLER] = adler
    return PngPlan(lengths, frame_tab, np.ascontiguousarray(chunks), file_offsets, adler)


# ----------------------------------------------------------------------------- the device forms
def _filter_code(filter) -> int:
    if isinstance(filter, str):
        if filter == "adaptive":
            return -1
    elif isinstance(filter, (int, np.integer)) and not isinstance(filter, bool) and 0 <= int(filter) <= 4:
        return int(filter)
    raise ValueError(f"png: filter must be 'adaptive' or 0..4, got {filter!r}")


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


def _encode_clip(frames_d: torch.Tensor, order, filter, segment_rows, who: str, guard: int = 0):
    """Both phases.  Returns (the output buffer on the device with `guard` bytes of 0xA5 on either side, the plan, the
    filter types u8 [n, H] on the device); (None, None, None) for an empty clip."""
    n, h, w, c, ocode, fcode, rows = _check_clip(frames_d, order, filter, segment_rows, who)
    if n == 0:
        return None, None, None
    if guard % 4:
        raise ValueError("guard must be a multiple of 4")
    dev = frames_d.device
    nseg = (h + rows - 1) // rows
    with torch.cuda.device(dev):
        types = torch.empty(n * h, dtype=torch.uint8, device=dev)
        stats_d = torch.empty(n * nseg * STATS_STRIDE, dtype=torch.int32, device=dev)
        check(lib().elvis_png_stats(ptr(frames_d), ptr(types), ptr(stats_d), n, h, w, c, ocode, fcode, rows, _s(frames_d)), dev)
        # the one synchronisation of a clip: every segment's histogram and Adler partial
        stats = stats_d.cpu().numpy().view(np.uint32).reshape(n, nseg, STATS_STRIDE)
        plan = plan_layout(stats)
        total = int(plan.file_offsets[-1])
        chunks_d = torch.from_numpy(plan.chunks).to(dev)
        tab_d = torch.from_numpy(plan.frame_tab.view(np.int32)).to(dev)
        out = torch.empty(total + 2 * guard, dtype=torch.uint8, device=dev)
        if guard:
            out[:guard] = 0xA5
            out[guard + total:] = 0xA5
        check(lib().elvis_png_pack(ptr(frames_d), ptr(types), ptr(chunks_d), ptr(tab_d), ptr(out) + guard, total, n, h, w, c, ocode,
                                   rows, _s(frames_d)), dev)
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


def _encode_to_host(frames_d, order, filter, segment_rows, who: str) -> List[np.ndarray]:
    out, plan, _ = _encode_clip(frames_d, order, filter, segment_rows, who)
    if out is None:
        return []
    c = int(frames_d.shape[3]) if frames_d.dim() == 4 else 1
    return _finish_files(out.cpu().numpy(), plan, int(frames_d.shape[1]), int(frames_d.shape[2]), c)


def encode_png_device(frames_d: torch.Tensor, order: str = "bgr", filter: Union[str, int] = "adaptive",
                      segment_rows: int = 16) -> List[bytes]:
    """One complete PNG file per frame of a resident contiguous uint8 clip [n,H,W,3], [n,H,W,1] or [n,H,W].  `order` is
    the channel order of a 3-channel clip ("bgr", what `save_frame` takes, or "rgb"); `filter` is "adaptive" (per row
    the type with the least sum of min(v, 256 - v), ties to the lower type) or one type 0..4 for every row; a frame is
    cut into deflate blocks and IDAT chunks of `segment_rows` rows.  A frame's bytes do not depend on the frames it is
    encoded with.  ValueError before any launch for a bad argument; an empty clip gives []."""
    return [v.tobytes() for v in _encode_to_host(frames_d, order, filter, segment_rows, "encode_png_device")]


def save_frames_device(frames_d: torch.Tensor, paths: Sequence, order: str = "bgr", filter: Union[str, int] = "adaptive",
                       segment_rows: int = 16) -> None:
    """`encode_png_device`, one download, and frame i written to paths[i]; directories are created as `save_frame`
    does."""
    paths = list(paths)
    if not isinstance(frames_d, torch.Tensor) or frames_d.dim() < 1 or len(paths) != frames_d.shape[0]:
        raise ValueError(f"save_frames_device: {len(paths)} path(s) for the clip {tuple(getattr(frames_d, 'shape', ()))}")
    for path, view in zip(paths, _encode_to_host(frames_d, order, filter, segment_rows, "save_frames_device")):
        os.makedirs(os.path.dirname(os.fspath(path)) or ".", exist_ok=True)
        with open(path, "wb") as f:
            f.write(memoryview(view))


def save_frames(frames, paths: Sequence, device="cuda:0", *, chunk_frames=None, order: str = "bgr",
                filter: Union[str, int] = "adaptive", segment_rows: int = 16) -> None:
    """Host frames - uint8 (H,W,3), (H,W,1) or (H,W) arrays, a list or one [n,...] array - written as PNGs to `paths`
    through the device.  Uploaded and encoded `chunk_frames` frames at a time, by default as many as make 32 MB (5 at
    1080p); a run of equal shapes is one clip.  The files do not depend on the chunk size."""
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
            save_frames_device(clip, paths[at:end], order, filter, segment_rows)
            at = end


def _check_args_only(order, filter, segment_rows) -> None:
    if order not in ("bgr", "rgb"):
        raise ValueError(f"save_frames: order must be 'bgr' or 'rgb', got {order!r}")
    _filter_code(filter)
    if isinstance(segment_rows, bool) or not isinstance(segment_rows, (int, np.integer)) or int(segment_rows) < 1:
        raise ValueError(f"save_frames: segment_rows must be an integer >= 1, got {segment_rows!r}")
