"""JPEG frames read by the device (csrc/jpeg_read.hip, csrc/jpeg_decode.h): every frame loader of the reference takes
`.jpg` / `.jpeg` beside `.png` (elvis.py:147, 193, 238, 549, 1495, 1724, 3033, 4785, 4811), and so does
`frameio.load_frame` through PIL.  This is the device path for them, the reader half of png.py once more:

  parse_jpeg(data)                          host: the markers only -> JpegInfo
  decode_jpeg_device(files, device)         JPEG files in memory -> resident u8 [n,H,W,channels]
  load_jpeg_frames_device(paths, device)    the same from disk, uploaded in chunks
  load_images_device(paths, device)         PNG and JPEG files by their first bytes, one resident clip

Baseline (SOF0, or SOF1 with 8-bit samples), Huffman coded, one interleaved scan, gray or YCbCr 4:4:4 / 4:2:2 / 4:2:0.
The host walks the markers and uploads the file bytes as they are with a table of the entropy-coded segments (a file
is cut at its RSTn markers), the (counts, values) of the Huffman tables and the quantisation tables.  The code tables,
the entropy decode (a lane per segment, all frames of a clip in one launch), the IDCT, the chroma upsampling and the
colour conversion run on the device, and one download of the per-segment status words ends a clip:
IOError("Failed to load frame: <path>") for a corrupt file, as `frameio.load_frame`.  Unsupported files raise
ValueError before any launch.  The pixels are those of a libjpeg-turbo PIL with default settings - the slow integer
IDCT, fancy upsampling - bit for bit; tests/_jpeg_ref.py states them.  What PIL makes of corrupt data (warnings, partial
pictures) is not reproduced.  Opt-in: `frameio.load_frame` stays PIL, and the directory drivers read through PIL unless
called with `png_reader="device"`.  The writer is jpeg_write.py.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import png
from ._lib import check, lib, ptr
from .ops import _s

STATUS_NAMES = ("ok", "no Huffman code of up to 16 bits matches", "coefficient index past 63",
                "the bits run out before the segment's MCUs are done", "dequantised coefficient outside [-32768, 32767]",
                "bad descriptor")
FD_WORDS = 32               # the frame descriptor, i32: see include/elvis_amd.h
SEG_WORDS = 5               # offset, length, first MCU, MCU count, frame
HUFF_BYTES = 272            # 16 counts and 256 values
TABLE_BYTES = 1312          # sizeof(JpegTable) of csrc/jpeg_decode.h
MAX_FRAMES = 4096           # frames of one launch
READ_CHUNK_BYTES = 512 << 20
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_SOF_REFUSED = {0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential (hierarchical)", 0xC6: "differential progressive",
                0xC7: "lossless (differential)", 0xC9: "arithmetic coding", 0xCA: "arithmetic coding (progressive)",
                0xCB: "lossless with arithmetic coding", 0xCD: "arithmetic coding (differential)",
                0xCE: "arithmetic coding (differential progressive)", 0xCF: "lossless with arithmetic coding (differential)"}


@dataclass
class JpegComponent:
    id: int
    h: int
    v: int
    tq: int                 # quantisation table
    td: int = 0             # DC and AC Huffman tables of the scan
    ta: int = 0


@dataclass
class JpegInfo:
    width: int
    height: int
    components: List[JpegComponent]
    qtables: np.ndarray                                        # uint16 [4, 64], natural order; zeros where not defined
    huffman: Dict[Tuple[int, int], Tuple[bytes, bytes]]        # (class 0 DC | 1 AC, table) -> (16 counts, values)
    restart_interval: int
    segments: List[Tuple[int, int, int, int]]                  # (byte offset, byte length, first MCU, MCU count)


def _corrupt(name) -> IOError:
    return IOError(f"Failed to load frame: {name}")


def _check_huffman(counts: bytes, values: bytes, cls: int) -> bool:
    space = 1
    for c in counts:
        space = 2 * space - c
        if space < 0:
            return False
    return sum(counts) <= 256 and (cls == 1 or all(v <= 15 for v in values))


def parse_jpeg(data, name="<bytes>") -> JpegInfo:
    """Host only: the markers of one JPEG file; no entropy-coded byte is decoded (they are searched for FF).  ValueError
    (naming `name` and the feature) for a file that is no JPEG or a valid one of a kind that is not built; IOError("Failed
    to load frame: <name>") for one that is broken at marker level.  EXIF orientation is ignored, as PIL's
    `Image.open(...).convert("RGB")` ignores it."""
    data = bytes(data)
    size = len(data)
    if data[:2] != b"\xff\xd8":
        raise _corrupt(name)
    at = 2
    qt = np.zeros((4, 64), np.uint16)
    qt_defined = [False] * 4
    huff: Dict[Tuple[int, int], Tuple[bytes, bytes]] = {}
    comps: Optional[List[JpegComponent]] = None
    width = height = ri = 0
    jfif, adobe = False, None
    while True:
        if at + 4 > size or data[at] != 0xFF:
            raise _corrupt(name)
        while data[at + 1] == 0xFF:
            at += 1
            if at + 4 > size:
                raise _corrupt(name)
        m = data[at + 1]
        if m in (0x00, 0x01, 0xD8, 0xD9) or 0xD0 <= m <= 0xD7:
            raise _corrupt(name)                               # no SOS before EOI, or a marker that has no place here
        (ln,) = struct.unpack(">H", data[at + 2:at + 4])
        if ln < 2 or at + 2 + ln > size:
            raise _corrupt(name)
        body = data[at + 4:at + 2 + ln]
        at += 2 + ln
        if m in _SOF_REFUSED:
            raise ValueError(f"{name}: {_SOF_REFUSED[m]} JPEG (SOF{m - 0xC0}) is not supported")
        if m in (0xC0, 0xC1):
            if comps is not None or len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise _corrupt(name)
            if body[0] != 8:
                raise ValueError(f"{name}: {body[0]}-bit precision is not supported (8-bit only)")
            height, width = struct.unpack(">HH", body[1:5])
            n = body[5]
            if n in (2, 4):
                raise ValueError(f"{name}: {n} components are not supported (1 or 3)")
            if n not in (1, 3) or width == 0:
                raise _corrupt(name)
            if height == 0:
                raise ValueError(f"{name}: height 0 (a DNL marker gives the height) is not supported")
            comps = [JpegComponent(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(n)]
            if any(c.tq > 3 or not 1 <= c.h <= 4 or not 1 <= c.v <= 4 for c in comps) or len({c.id for c in comps}) != n:
                raise _corrupt(name)
        elif m == 0xDB:
            p = 0
            while p < len(body):
                prec, t = body[p] >> 4, body[p] & 15
                nbytes = 128 if prec == 1 else 64
                if prec > 1 or t > 3 or p + 1 + nbytes > len(body):
                    raise _corrupt(name)
                vals = np.frombuffer(body, dtype=">u2" if prec else np.uint8, count=64, offset=p + 1)
                qt[t, list(ZIGZAG)] = vals
                qt_defined[t] = True
                p += 1 + nbytes
        elif m == 0xC4:
            p = 0
            while p < len(body):
                if p + 17 > len(body):
                    raise _corrupt(name)
                cls, t = body[p] >> 4, body[p] & 15
                counts = body[p + 1:p + 17]
                total = sum(counts)
                values = body[p + 17:p + 17 + total]
                if cls > 1 or t > 3 or len(values) != total or not _check_huffman(counts, values, cls):
                    raise _corrupt(name)
                huff[(cls, t)] = (counts, values)
                p += 17 + total
        elif m == 0xDD:
            if len(body) != 2:
                raise _corrupt(name)
            (ri,) = struct.unpack(">H", body)
        elif m == 0xDC:
            raise ValueError(f"{name}: a DNL marker is not supported")
        elif m == 0xE0 and body[:5] == b"JFIF\x00":
            jfif = True
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif m == 0xDA:
            if comps is None or len(body) < 1:
                raise _corrupt(name)
            ns = body[0]
            if len(body) != 4 + 2 * ns or ns < 1 or ns > len(comps):
                raise _corrupt(name)
            if ns < len(comps):
                raise ValueError(f"{name}: more than one scan (a scan of {ns} of {len(comps)} components) is not supported")
            for c, comp in enumerate(comps):
                if body[1 + 2 * c] != comp.id:
                    raise _corrupt(name)
                comp.td, comp.ta = body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15
                if comp.td > 3 or comp.ta > 3 or (0, comp.td) not in huff or (1, comp.ta) not in huff or not qt_defined[comp.tq]:
                    raise _corrupt(name)
            if tuple(body[1 + 2 * ns:]) != (0, 63, 0):
                raise ValueError(f"{name}: a scan with Ss, Se, Ah/Al = {tuple(body[1 + 2 * ns:])} is not supported (sequential 0, 63, 0 only)")
            break
    if len(comps) == 3:
        samp = [(c.h, c.v) for c in comps]
        if samp[0] not in ((1, 1), (2, 1), (2, 2)) or samp[1] != (1, 1) or samp[2] != (1, 1):
            raise ValueError(f"{name}: sampling {'/'.join(f'{h}x{v}' for h, v in samp)} is not supported (luma 1x1, 2x1 or 2x2, chroma 1x1)")
        if adobe is not None and adobe != 1:
            raise ValueError(f"{name}: an Adobe APP14 segment with transform {adobe} (not YCbCr) is not supported")
        if not jfif and adobe is None and [c.id for c in comps] == [82, 71, 66]:
            raise ValueError(f"{name}: component ids R, G, B without JFIF (an RGB file) are not supported")
        hmax, vmax = samp[0]
    else:
        hmax = vmax = 1
    total = -(-width // (8 * hmax)) * -(-height // (8 * vmax))
    per = ri if ri else total
    segments, start, p = [], at, at
    while True:
        p = data.find(b"\xff", p)
        if p < 0:
            raise _corrupt(name)                               # no EOI
        q = p
        while q + 1 < size and data[q + 1] == 0xFF:
            q += 1
        if q + 1 >= size:
            raise _corrupt(name)
        b = data[q + 1]
        if b == 0:
            if q != p:
                raise _corrupt(name)                           # fill bytes in front of a stuffed zero
            p += 2
            continue
        first = len(segments) * per
        if first >= total:
            raise _corrupt(name)                               # more segments than ceil(MCUs / Ri)
        segments.append((start, p - start, first, min(per, total - first)))
        if 0xD0 <= b <= 0xD7:
            if b - 0xD0 != (len(segments) - 1) % 8 or ri == 0:
                raise _corrupt(name)
            start = p = q + 2
            continue
        if b == 0xD9:
            break
        if b == 0xDC:
            raise ValueError(f"{name}: a DNL marker is not supported")
        if b in (0xDA, 0xC4, 0xDB, 0xDD):
            raise ValueError(f"{name}: more than one scan is not supported")
        raise _corrupt(name)
    if len(segments) != -(-total // per):
        raise _corrupt(name)
    return JpegInfo(int(width), int(height), comps, qt, huff, int(ri), segments)


# ----------------------------------------------------------------------------- the layout
@dataclass
class JpegPlan:
    """What the entry points are handed for the files of one launch."""
    fd: np.ndarray            # int32 [n, 32]
    qt: np.ndarray            # uint16 [n, 4, 64]
    huff: np.ndarray          # uint8 [n, 8, 272]: DC tables 0..3, AC tables 0..3
    segs: np.ndarray          # int32 [nseg, 5]
    seg_frame: np.ndarray     # [nseg]
    file_off: np.ndarray      # int64 [n + 1]
    stride_blocks: int        # coefficient blocks between two frames; a frame's planes are 64 bytes a block


def frame_blocks(info: JpegInfo) -> int:
    if len(info.components) == 1:
        return -(-info.width // 8) * -(-info.height // 8)
    hmax, vmax = info.components[0].h, info.components[0].v
    return -(-info.width // (8 * hmax)) * -(-info.height // (8 * vmax)) * (hmax * vmax + 2)


def plan_clip(infos: Sequence[JpegInfo], sizes: Sequence[int]) -> JpegPlan:
    n = len(infos)
    fd = np.zeros((n, FD_WORDS), np.int32)
    qt = np.zeros((n, 4, 64), np.uint16)
    huff = np.zeros((n, 8, HUFF_BYTES), np.uint8)
    file_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    segs, seg_frame = [], []
    for f, info in enumerate(infos):
        gray = len(info.components) == 1
        samp = [(1, 1)] if gray else [(c.h, c.v) for c in info.components]
        hmax, vmax = samp[0]
        mcux, mcuy = -(-info.width // (8 * hmax)), -(-info.height // (8 * vmax))
        fd[f, :5] = (len(samp), hmax, vmax, mcux, mcuy)
        base = 0
        for c, (comp, (h, v)) in enumerate(zip(info.components, samp)):
            fd[f, 8 + 8 * c:16 + 8 * c] = (h, v, base, base * 64, mcux * h * 8, comp.td, comp.ta, comp.tq)
            base += mcux * h * mcuy * v
        fd[f, 5] = base
        qt[f] = info.qtables
        for (cls, t), (counts, values) in info.huffman.items():
            huff[f, 4 * cls + t, :16] = np.frombuffer(counts, np.uint8)
            huff[f, 4 * cls + t, 16:16 + len(values)] = np.frombuffer(values, np.uint8)
        for off, length, first, count in info.segments:
            segs.append((int(file_off[f]) + off, length, first, count, f))
            seg_frame.append(f)
    return JpegPlan(fd, qt, huff, np.asarray(segs, np.int32).reshape(-1, SEG_WORDS), np.asarray(seg_frame, np.int64), file_off,
                    max(frame_blocks(i) for i in infos))


def _check_read_args(order, channels, who: str) -> None:
    if order not in ("bgr", "rgb"):
        raise ValueError(f"{who}: order must be 'bgr' or 'rgb', got {order!r}")
    if isinstance(channels, bool) or channels not in (1, 3):
        raise ValueError(f"{who}: channels must be 1 or 3, got {channels!r}")


def _check_infos(infos: Sequence[JpegInfo], names: Sequence, channels: int, who: str, size=None) -> Tuple[int, int]:
    """One size for all files, gray files only for channels=1: (H, W)."""
    for info, name in zip(infos, names):
        if size is None:
            size = (info.height, info.width)
        if (info.height, info.width) != size:
            raise ValueError(f"{who}: {name} is {info.height}x{info.width}, the files before it {size[0]}x{size[1]}")
        if channels == 1 and len(info.components) != 1:
            raise ValueError(f"{who}: {name} is a colour file; channels=1 is for gray files only")
    return size


@dataclass
class _Pending:
    """A launched clip whose status words are still on the device."""
    status_d: torch.Tensor        # i32 [nseg, 2]: code, MCUs done
    seg_frame: np.ndarray
    n: int
    tables_d: Optional[torch.Tensor] = None   # u8 [n, 8, TABLE_BYTES], the derived code tables: kept for `_decode_clip` only


def _guarded(nbytes: int, guard: int, dev, zero: bool = False):
    """(a uint8 buffer of nbytes with `guard` bytes of 0xA5 on either side, the payload's view)"""
    buf = (torch.zeros if zero else torch.empty)(nbytes + 2 * guard, dtype=torch.uint8, device=dev)
    if guard:
        buf[:guard] = 0xA5
        buf[guard + nbytes:] = 0xA5
    return buf, buf[guard:guard + nbytes]


def _launch_decode(files: Sequence, infos: Sequence[JpegInfo], frames_out: torch.Tensor, order: str, channels: int, *,
                   guard: int = 0, upload_offset: int = 0, keep_tables: bool = False):
    """Code tables, entropy decode, IDCT, upsampling and colour of one clip into frames_out [n,H,W,channels] (resident,
    contiguous); nothing is downloaded.  `guard` bytes of 0xA5 go on either side of the coefficient and plane buffers, and
    the uploaded bytes start `upload_offset` bytes past a dword; `keep_tables` leaves the derived code tables in the
    _Pending (the tests' knobs).  Returns the _Pending, the coefficient buffer and the plane buffer with their guards,
    and the plan."""
    dev = frames_out.device
    n = len(files)
    h, w = int(frames_out.shape[1]), int(frames_out.shape[2])
    if guard % 16:
        raise ValueError("guard must be a multiple of 16")
    if n > MAX_FRAMES:
        raise ValueError(f"decode_jpeg_device: {n} files in one launch (at most {MAX_FRAMES}); decode the clip in parts")
    plan = plan_clip(infos, [len(memoryview(f)) for f in files])
    total = int(plan.file_off[-1])
    if total + upload_offset >= 1 << 31 or n * plan.stride_blocks * 128 >= 1 << 40:
        raise ValueError(f"decode_jpeg_device: {total} bytes of files are 2^31 or more; decode the clip in parts")
    host = np.empty(total + upload_offset, dtype=np.uint8)
    for f, data in enumerate(files):
        host[upload_offset + int(plan.file_off[f]):upload_offset + int(plan.file_off[f + 1])] = np.frombuffer(data, dtype=np.uint8)
    nseg = plan.segs.shape[0]
    with torch.cuda.device(dev):
        files_d = torch.from_numpy(host).to(dev)[upload_offset:]
        fd_d = torch.from_numpy(plan.fd).to(dev)
        qt_d = torch.from_numpy(plan.qt.view(np.int16)).to(dev)
        huff_d = torch.from_numpy(plan.huff).to(dev)
        segs_d = torch.from_numpy(plan.segs).to(dev)
        tables_d = torch.empty(n * 8 * TABLE_BYTES, dtype=torch.uint8, device=dev)
        coef_buf, coef_d = _guarded(n * plan.stride_blocks * 128, guard, dev, zero=True)
        plane_buf, plane_d = _guarded(n * plan.stride_blocks * 64, guard, dev)
        status_d = torch.zeros(2 * nseg, dtype=torch.int32, device=dev)
        s = _s(frames_out)
        check(lib().elvis_jpeg_entropy(ptr(files_d), total, ptr(segs_d), nseg, ptr(fd_d), n, ptr(huff_d), ptr(qt_d), ptr(tables_d),
                                       ptr(coef_d), plan.stride_blocks, ptr(status_d), s), dev)
        check(lib().elvis_jpeg_idct(ptr(coef_d), plan.stride_blocks, ptr(fd_d), n, ptr(plane_d), s), dev)
        check(lib().elvis_jpeg_colour(ptr(plane_d), plan.stride_blocks, ptr(fd_d), ptr(frames_out), n, h, w, channels, int(order == "bgr"), s), dev)
    # the work buffers are not kept: every launch above is on the current stream, and the allocator hands a freed block
    # only to later work on that stream
    return _Pending(status_d, plan.seg_frame, n, tables_d if keep_tables else None), coef_buf, plane_buf, plan


def _frame_codes(pending: _Pending, status: np.ndarray) -> List[int]:
    """One status code per frame: that of its first defective segment."""
    codes = [0] * pending.n
    st = status.reshape(-1, 2)
    for s in np.flatnonzero(st[:, 0])[::-1]:
        codes[int(pending.seg_frame[s])] = int(st[s, 0])
    return codes


def _decode_clip(files: Sequence, device, order: str, channels: int, names: Optional[Sequence] = None, *, guard: int = 0,
                 upload_offset: int = 0, who: str = "decode_jpeg_device"):
    """decode_jpeg_device without the raise: a dict of the frames [n,H,W,channels] (a view into `frames_buf`, which has
    `guard` bytes of 0xA5 on either side), the coefficient and plane buffers with their guards, the plan, the status
    words u32 [nseg, 2] and one status code per frame."""
    _check_read_args(order, channels, who)
    files = list(files)
    names = [f"<file {i}>" for i in range(len(files))] if names is None else list(names)
    if len(names) != len(files):
        raise ValueError(f"{who}: {len(names)} name(s) for {len(files)} file(s)")
    if not files:
        raise ValueError(f"{who}: no files")
    infos = [parse_jpeg(data, name) for data, name in zip(files, names)]
    h, w = _check_infos(infos, names, channels, who)
    dev = L.resolve_device(device)
    n = len(files)
    with torch.cuda.device(dev):
        frames_buf, payload = _guarded(n * h * w * channels, guard, dev)
        frames = payload.view(n, h, w, channels)
        pending, coef_buf, plane_buf, plan = _launch_decode(files, infos, frames, order, channels, guard=guard, upload_offset=upload_offset,
                                                            keep_tables=True)
        # the one synchronisation of a clip: the status words
        status = pending.status_d.cpu().numpy().view(np.uint32).reshape(-1, 2)
    return {"frames": frames, "frames_buf": frames_buf, "coef_buf": coef_buf, "plane_buf": plane_buf, "plan": plan,
            "status": status, "codes": _frame_codes(pending, status), "tables": pending.tables_d}


def decode_jpeg_device(files: Sequence, device="cuda:0", order: str = "bgr", channels: int = 3, names: Optional[Sequence] = None) -> torch.Tensor:
    """JPEG files in memory (bytes-like, one per frame) decoded on the device into a resident contiguous uint8
    [n,H,W,channels] tensor.  `channels=3` (the default): gray is replicated; `order` "bgr" (what `frameio.load_frame`
    gives) or "rgb".  `channels=1` is for gray files only.  All files have one size.  ValueError before any launch for a
    bad argument or an unsupported file; IOError("Failed to load frame: <name>") for a corrupt one (`names` default to
    "<file i>")."""
    names = [f"<file {i}>" for i in range(len(files))] if names is None else list(names)
    got = _decode_clip(files, device, order, channels, names)
    for name, code in zip(names, got["codes"]):
        if code:
            raise _corrupt(name)
    return got["frames"]


def _read(path) -> bytes:
    try:
        with open(path, "rb") as fh:
            return fh.read()
    except OSError as exc:
        raise _corrupt(path) from exc


def load_jpeg_frames_device(paths: Sequence, device="cuda:0", order: str = "bgr", channels: int = 3,
                            chunk_frames: Optional[int] = None) -> torch.Tensor:
    """The JPEG files `paths` decoded on the device into one resident contiguous uint8 [n,H,W,channels] tensor: what
    `frameio.load_frame` per file and `recompose.frames_to_device` give, without a host pass over the pixels.  The files
    are read and uploaded `chunk_frames` at a time (by default as many as make 512 MB of device work space); every
    chunk's kernels are launched before the one download of all status words.  The result does not depend on the chunk
    size.  Errors as `decode_jpeg_device`, naming the path."""
    who = "load_jpeg_frames_device"
    _check_read_args(order, channels, who)
    paths = list(paths)
    if not paths:
        raise ValueError(f"{who}: no paths")
    if chunk_frames is not None and (isinstance(chunk_frames, bool) or int(chunk_frames) < 1):
        raise ValueError("chunk_frames must be at least 1")
    dev = L.resolve_device(device)
    out, size, pendings, at = None, None, [], 0
    with torch.cuda.device(dev):
        while at < len(paths):
            files, infos = [], []
            while at + len(files) < len(paths):
                path = paths[at + len(files)]
                data = _read(path)
                info = parse_jpeg(data, path)
                size = _check_infos([info], [path], channels, who, size)
                files.append(data)
                infos.append(info)
                # per frame: coefficients and planes, 128 + 64 bytes a block, and the file; every launch lasts as long as
                # its longest segment, so chunks are as large as the work space allows
                step = int(chunk_frames) if chunk_frames is not None else max(1, READ_CHUNK_BYTES // (192 * frame_blocks(infos[0]) + 2 * len(files[0])))
                if len(files) >= min(step, MAX_FRAMES):
                    break
            if out is None:
                if len(paths) * size[0] * size[1] * channels >= 1 << 40:
                    raise ValueError(f"{who}: the clip is too large")
                out = torch.empty((len(paths), size[0], size[1], channels), dtype=torch.uint8, device=dev)
            pending, _, _, _ = _launch_decode(files, infos, out[at:at + len(files)], order, channels)
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


def _kind(path) -> str:
    try:
        with open(path, "rb") as fh:
            head = fh.read(8)
    except OSError as exc:
        raise _corrupt(path) from exc
    if head == png.PNG_SIGNATURE:
        return "png"
    if head[:2] == b"\xff\xd8":
        return "jpeg"
    raise ValueError(f"load_images_device: {path} is neither a PNG nor a JPEG file (by its first bytes)")


def load_images_device(paths: Sequence, device="cuda:0", order: str = "bgr", channels: int = 3,
                       chunk_frames: Optional[int] = None) -> torch.Tensor:
    """PNG and JPEG files, told apart by their first bytes (the PNG signature or FF D8) and not by their suffix, decoded
    on the device into one resident contiguous uint8 [n,H,W,channels] clip.  A list that is all PNG is exactly one call
    of `png.load_frames_device`, one that is all JPEG one of `load_jpeg_frames_device`; in a mixed list each kind is
    decoded into its rows of the clip.  All files have one size (ValueError otherwise)."""
    _check_read_args(order, channels, "load_images_device")
    paths = list(paths)
    if not paths:
        raise ValueError("load_images_device: no paths")
    kinds = [_kind(p) for p in paths]
    loaders = {"png": lambda sel: png.load_frames_device(sel, device, order, channels, chunk_frames),
               "jpeg": lambda sel: load_jpeg_frames_device(sel, device, order, channels, chunk_frames)}
    if len(set(kinds)) == 1:
        return loaders[kinds[0]](paths)
    out = None
    for kind in ("png", "jpeg"):
        rows = [i for i, k in enumerate(kinds) if k == kind]
        clip = loaders[kind]([paths[i] for i in rows])
        if out is None:
            out = torch.empty((len(paths),) + tuple(clip.shape[1:]), dtype=torch.uint8, device=clip.device)
        if tuple(clip.shape[1:]) != tuple(out.shape[1:]):
            raise ValueError(f"load_images_device: the JPEG files are {clip.shape[1]}x{clip.shape[2]}, the PNG files "
                             f"{out.shape[1]}x{out.shape[2]}")
        out[torch.as_tensor(rows, device=clip.device)] = clip
    return out
