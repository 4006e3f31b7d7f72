"""The hand-off to the encoders: RGB frames to I420 on the device, the Y4M container, the importance rule and the ROI maps.

What the reference does between its degraders and Kvazaar / SVT-AV1 / VMAF.  The pixel pass runs on the device:
`rgb_to_i420_device` is `cv2.cvtColor(frame, COLOR_RGB2YUV_I420)` over a resident `[n,H,W,3]` uint8 clip
(`elvis_rgb_to_i420_u8`, csrc/handoff.hip), and `convert_frames_to_yuv420p` (presley.py:217-223) and `write_y4m`
(utils.py:453-462, presley.py:590-599) keep the reference's names and argument order over it, so a clip leaves the
device as 1.5 bytes per pixel instead of 3.  The block-grid rules - `calculate_importance_scores` (utils.py:665-688,
presley.py:129-152), `create_kvazaar_roi_file` (utils.py:1026-1053), `create_svtav1_roi_file` (utils.py:1056-1092) -
touch By x Bx values per frame and RUN ON THE HOST in numpy.

The way back is the hand-off FROM a decoder: `i420_to_rgb_device` is `cv2.cvtColor(planes, COLOR_YUV2RGB_I420)` over a
resident `[n, H*3//2, W]` clip (`elvis_i420_to_rgb_u8`, csrc/i420_in.hip); `parse_y4m` walks a YUV4MPEG2 file on the host
without reading a payload byte, `load_y4m_device` / `load_yuv420p_device` read the payloads into pinned memory, upload
1.5 bytes per pixel and give the resident `[n,H,W,3]` clip every restorer takes, and `read_y4m` is the host-to-host
form next to `write_y4m`.

PARITY UNPINNED vs cv2: OpenCV is absent from the build and GPU environments.  The colour conversion restates OpenCV
4.x's RGB8toYUV420pInvoker (20-bit fixed point, chroma taken from the even row / even column pixel of each 2x2 quad,
not averaged), its inverse restates YUV420p2RGB8Invoker (the same fixed point, luma clamped at 16, chroma replicated
over its quad, not interpolated; bit-exact with tests/_i420_in_ref.py, not checked against cv2 itself) and the one resize of the SVT-AV1 map restates its float INTER_AREA (`ResizeAreaFast` at a whole ratio in
both axes, `ResizeArea` over `computeResizeAreaTab` otherwise); the device is bit-exact with tests/_handoff_ref.py, not
checked against cv2 itself.  The importance rule, both ROI file formats and the Y4M framing ARE pinned against the
reference's own code (tests/golden/handoff.npz).
DEPARTURES: an odd frame height or width raises ValueError (cv2 raises its own error); an importance grid that is not
larger than the 64 x 64 superblock grid in both axes raises ValueError (cv2.resize leaves the area rule there).
"""
from __future__ import annotations

import io
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib, ptr
from .degrade import area_table
from .ops import _s
from .recompose import frames_to_device

I420_CHUNK_BYTES = 32 << 20
KVAZAAR_DELTA_LIMIT = 14           # Kvazaar's own bound on a delta QP
HEVC_QP = (0, 51)
AV1_QP = (0, 63)
AV1_SUPERBLOCK = 64
AV1_SEGMENTS = 8


# ----------------------------------------------------------------------------- the device form
def rgb_to_i420_device(frames_d: torch.Tensor, order: str = "rgb", out=None) -> torch.Tensor:
    """cv2.cvtColor(frame, COLOR_RGB2YUV_I420) (order="bgr": COLOR_BGR2YUV_I420) of every frame of a resident clip.
    frames [n,H,W,3] u8 on the device -> [n, H*3//2, W] u8: per frame the Y plane, then U and V at half size, the
    bytes the reference writes.  `out`, when given, must be exactly that: shape, uint8, device, contiguous.  An odd H
    or W, a channel count other than 3, a non-uint8 input or another `order` raise ValueError.
    PARITY UNPINNED vs cv2 (module docstring)."""
    if order not in ("rgb", "bgr"):
        raise ValueError('rgb_to_i420: order must be "rgb" or "bgr"')
    if not isinstance(frames_d, torch.Tensor) or frames_d.dtype != torch.uint8 or not frames_d.is_cuda or not frames_d.is_contiguous():
        raise ValueError("rgb_to_i420: frames must be a contiguous CUDA uint8 tensor")
    if frames_d.dim() != 4 or frames_d.shape[3] != 3:
        raise ValueError("rgb_to_i420: frames must be [n, H, W, 3]")
    n, h, w, _ = frames_d.shape
    if h % 2 or w % 2:
        raise ValueError(f"rgb_to_i420: I420 needs an even height and width, got {h} x {w}")
    shape = (n, h * 3 // 2, w)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=frames_d.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != frames_d.device \
            or tuple(out.shape) != shape:
        raise ValueError(f"rgb_to_i420: out must be a contiguous uint8 tensor of shape {shape} on the frames' device")
    if n and h and w:
        check(lib().elvis_rgb_to_i420_u8(ptr(frames_d), ptr(out), n, h, w, int(order == "bgr"), _s(frames_d)), frames_d.device)
    return out


# ----------------------------------------------------------------------------- the reference's call surface
def _chunk_frames(frame_shape, chunk_frames) -> int:
    if chunk_frames is not None:
        if int(chunk_frames) < 1:
            raise ValueError("chunk_frames must be at least 1")
        return int(chunk_frames)
    h, w = frame_shape[:2]
    return max(1, I420_CHUNK_BYTES // max(1, h * 3 // 2 * w))


def _i420_chunks(frames: Sequence[np.ndarray], device, chunk_frames):
    """Upload, convert and download `frames` a chunk at a time; yields host arrays [k, H*3//2, W]."""
    dev = L.resolve_device(device)
    step = _chunk_frames(frames[0].shape, chunk_frames)
    with torch.cuda.device(dev):
        for at in range(0, len(frames), step):
            yield rgb_to_i420_device(frames_to_device(list(frames[at:at + step]), dev)).cpu().numpy()


def convert_frames_to_yuv420p(frames: List[np.ndarray], device="cuda:0", *, chunk_frames=None) -> bytes:
    """presley.py:217-223 on the device: the I420 bytes of every RGB frame, one after the other.  The clip is uploaded,
    converted and downloaded in chunks of `chunk_frames` frames - by default as many as make 32 MB of I420 (10 frames at
    1080p) - so neither the RGB nor the I420 clip is ever whole in HBM; the bytes do not depend on the chunk size.
    PARITY UNPINNED vs cv2 (module docstring)."""
    if len(frames) == 0:
        return b""
    yuv_bytes = io.BytesIO()
    for planes in _i420_chunks(frames, device, chunk_frames):
        yuv_bytes.write(planes.tobytes())
    return yuv_bytes.getvalue()


def y4m_header(width: int, height: int, framerate: float) -> bytes:
    """The stream header `write_y4m` starts with: the frame rate as a whole number of thousandths.  Host."""
    return f"YUV4MPEG2 W{width} H{height} F{int(round(framerate * 1000))}:1000 Ip A1:1 C420\n".encode()


def write_y4m(frames: List[np.ndarray], y4m_path: str, framerate: float, device="cuda:0", *, chunk_frames=None) -> None:
    """utils.py:453-462 (= presley.py:590-599) on the device: `y4m_header`, then per frame `FRAME\\n` and its I420
    planes.  Converted in chunks of `chunk_frames` frames - by default as many as make 32 MB of I420 (10 frames at
    1080p) - and written as they arrive; the file does not depend on the chunk size.
    PARITY UNPINNED vs cv2 (module docstring)."""
    height, width = frames[0].shape[:2]
    if height % 2 or width % 2:
        raise ValueError(f"write_y4m: I420 needs an even height and width, got {height} x {width}")
    L.resolve_device(device)
    with open(y4m_path, "wb") as f:
        f.write(y4m_header(width, height, framerate))
        for planes in _i420_chunks(frames, device, chunk_frames):
            for frame_planes in planes:
                f.write(b"FRAME\n")
                f.write(frame_planes.tobytes())


# ----------------------------------------------------------------------------- the way back: decoder output to a clip
def i420_to_rgb_device(planes_d: torch.Tensor, order: str = "rgb", out=None) -> torch.Tensor:
    """cv2.cvtColor(planes, COLOR_YUV2RGB_I420) (order="bgr": COLOR_YUV2BGR_I420) of every frame of a resident clip of
    decoder output.  planes [n, H*3//2, W] u8 on the device, contiguous - per frame the Y plane, then U and V at half
    size, what `rgb_to_i420_device` writes - -> [n,H,W,3] u8.  `out`, when given, must be exactly that: shape, uint8,
    device, contiguous.  A second-axis length that is no multiple of 3 or that makes H odd, an odd W, a non-uint8
    input or another `order` raise ValueError.
    PARITY UNPINNED vs cv2 (module docstring)."""
    if order not in ("rgb", "bgr"):
        raise ValueError('i420_to_rgb: order must be "rgb" or "bgr"')
    if not isinstance(planes_d, torch.Tensor) or planes_d.dtype != torch.uint8 or not planes_d.is_cuda or not planes_d.is_contiguous():
        raise ValueError("i420_to_rgb: planes must be a contiguous CUDA uint8 tensor")
    if planes_d.dim() != 3:
        raise ValueError("i420_to_rgb: planes must be [n, H*3//2, W]")
    n, rows, w = planes_d.shape
    if rows % 3:                                         # H*3//2 of an odd H is 1 mod 3
        raise ValueError(f"i420_to_rgb: {rows} rows are not the H*3//2 of an even height")
    h = rows // 3 * 2
    if w % 2:
        raise ValueError(f"i420_to_rgb: I420 needs an even height and width, got {h} x {w}")
    shape = (n, h, w, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=planes_d.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != planes_d.device \
            or tuple(out.shape) != shape:
        raise ValueError(f"i420_to_rgb: out must be a contiguous uint8 tensor of shape {shape} on the planes' device")
    if n and h and w:
        check(lib().elvis_i420_to_rgb_u8(ptr(planes_d), ptr(out), n, h, w, int(order == "bgr"), _s(planes_d)), planes_d.device)
    return out


Y4M_MAGIC = b"YUV4MPEG2"
Y4M_COLOURSPACES = ("420", "420jpeg", "420mpeg2", "420paldv")   # one layout; the chroma siting is ignored, as cv2 ignores it
_Y4M_LINE_LIMIT = 4096


@dataclass(frozen=True)
class Y4MInfo:
    """What `parse_y4m` found: the stream header's fields and where every frame's planes start in the file."""
    width: int
    height: int
    fps_num: int                      # 0:0 where the header has no F token
    fps_den: int
    interlace: str                    # "p" or "?" ("?" also where the header has no I token)
    aspect: str                       # "1:1"; "0:0" (unknown) where the header has no A token
    colourspace: str                  # one of Y4M_COLOURSPACES; "420" where the header has no C token
    frame_count: int
    frame_offsets: Tuple[int, ...]    # byte offset of each frame's payload

    @property
    def frame_bytes(self) -> int:
        return self.width * self.height * 3 // 2

    @property
    def framerate(self) -> Optional[float]:
        return self.fps_num / self.fps_den if self.fps_num > 0 and self.fps_den > 0 else None


def _read_line(f, limit: int = _Y4M_LINE_LIMIT) -> bytes:
    """The bytes up to and including the next newline, one at a time from an unbuffered file: nothing past it is read."""
    line = bytearray()
    while len(line) < limit:
        c = f.read(1)
        if not c:
            break
        line += c
        if c == b"\n":
            break
    return bytes(line)


def parse_y4m(path: str) -> Y4MInfo:
    """The header of a YUV4MPEG2 file and the walk over its frames.  HOST.  The stream header and every `FRAME...\\n`
    line are read at their computed positions; no payload byte is.  Header tokens come in any order and unknown ones
    (`X...`) are ignored; `FRAME` lines may carry parameters; C420, C420jpeg, C420mpeg2, C420paldv or no C token are
    one layout (the siting is ignored); Ip, I? or no I token.  ValueError naming the file and the property: a wrong
    magic, a missing, non-positive or odd W or H, another colourspace, an interlaced stream.  IOError naming the file
    and the frame index: a FRAME marker that is not where the frame size puts it, a last frame cut short."""
    path = os.fspath(path)
    with open(path, "rb", buffering=0) as f:
        size = os.fstat(f.fileno()).st_size
        head = _read_line(f)
        if not head.startswith(Y4M_MAGIC) or not head.endswith(b"\n") or head[len(Y4M_MAGIC):len(Y4M_MAGIC) + 1] not in (b" ", b"\n"):
            raise ValueError(f"{path}: not a YUV4MPEG2 file (magic {head[:len(Y4M_MAGIC)]!r})")
        fields = {}
        for token in head[len(Y4M_MAGIC):].decode("ascii", "replace").split():
            fields.setdefault(token[0], token[1:])
        dims = {}
        for key, name in (("W", "width"), ("H", "height")):
            try:
                dims[key] = int(fields[key])
            except (KeyError, ValueError):
                raise ValueError(f"{path}: the Y4M header has no usable {name} ({key} token: {fields.get(key)!r})") from None
            if dims[key] <= 0:
                raise ValueError(f"{path}: Y4M {name} {dims[key]} is not positive")
            if dims[key] % 2:
                raise ValueError(f"{path}: I420 needs an even {name}, the Y4M header says {dims[key]}")
        colourspace = fields.get("C", "420")
        if colourspace not in Y4M_COLOURSPACES:
            raise ValueError(f"{path}: Y4M colourspace C{colourspace} is not 8-bit 4:2:0 (one of {', '.join('C' + c for c in Y4M_COLOURSPACES)})")
        interlace = fields.get("I", "?")
        if interlace not in ("p", "?"):
            raise ValueError(f"{path}: Y4M interlace I{interlace} is not progressive")
        fps_num = fps_den = 0
        if "F" in fields:
            try:
                num, den = fields["F"].split(":")
                fps_num, fps_den = int(num), int(den)
            except ValueError:
                raise ValueError(f"{path}: malformed Y4M frame rate F{fields['F']}") from None
        frame_bytes = dims["W"] * dims["H"] * 3 // 2
        offsets, pos = [], len(head)
        while pos < size:
            f.seek(pos)
            marker = f.read(6)
            if marker[:5] != b"FRAME" or marker[5:6] not in (b"\n", b" "):
                raise IOError(f"{path}: frame {len(offsets)}: no FRAME marker at byte {pos} (found {marker!r})")
            if marker[5:6] == b" ":
                marker += _read_line(f)
                if not marker.endswith(b"\n"):
                    raise IOError(f"{path}: frame {len(offsets)}: the FRAME line at byte {pos} does not end")
            start = pos + len(marker)
            if start + frame_bytes > size:
                raise IOError(f"{path}: frame {len(offsets)} is cut short: {size - start} of {frame_bytes} bytes")
            offsets.append(start)
            pos = start + frame_bytes
    return Y4MInfo(dims["W"], dims["H"], fps_num, fps_den, interlace, fields.get("A", "0:0"), colourspace, len(offsets), tuple(offsets))


def _window(total: int, start: int, count, what: str):
    start = int(start)
    count = total - start if count is None else int(count)
    if start < 0 or count < 0 or start + count > total:
        raise ValueError(f"{what}: frames [{start}, {start + count}) are not within the {total} it holds")
    return start, count


def _planes_to_clip(fill, count: int, height: int, width: int, dev, order: str, chunk_frames) -> torch.Tensor:
    """`count` I420 frames to one resident [count,H,W,3] clip, a chunk at a time: `fill(rows, at, k)` puts frames
    [at, at + k) into the pinned `rows` [k, H*3//2, W]; the chunk goes up on a copy stream and is converted on the
    current one, so the read and the upload of chunk i + 1 overlap the conversion of chunk i (two staging slots, the
    copy-stream pattern of restore._HostClipPipeline).  The clip does not depend on the chunk size."""
    rows = height * 3 // 2
    step = min(_chunk_frames((height, width), chunk_frames), max(1, count))
    with torch.cuda.device(dev):
        out = torch.empty((count, height, width, 3), dtype=torch.uint8, device=dev)
        if count == 0:
            return out
        compute = torch.cuda.current_stream(dev)
        h2d = torch.cuda.Stream(dev)
        h2d.wait_stream(compute)                          # `planes` may be a block that work queued on `compute` still reads
        slots = 1 if step >= count else 2
        host = [torch.empty((step, rows, width), dtype=torch.uint8).pin_memory() for _ in range(slots)]
        planes = [torch.empty((step, rows, width), dtype=torch.uint8, device=dev) for _ in range(slots)]
        uploaded, converted = [None] * slots, [None] * slots
        for i, at in enumerate(range(0, count, step)):
            slot, k = i % slots, min(step, count - at)
            if uploaded[slot] is not None:
                uploaded[slot].synchronize()              # the upload before last read this pinned buffer
            fill(host[slot].numpy()[:k], at, k)
            with torch.cuda.stream(h2d):
                if converted[slot] is not None:
                    h2d.wait_event(converted[slot])       # the conversion before last read this device buffer
                planes[slot][:k].copy_(host[slot][:k], non_blocking=True)
                uploaded[slot] = torch.cuda.Event()
                uploaded[slot].record(h2d)
            compute.wait_event(uploaded[slot])
            i420_to_rgb_device(planes[slot][:k], order, out=out[at:at + k])
            converted[slot] = torch.cuda.Event()
            converted[slot].record(compute)
        for ev in uploaded:
            if ev is not None:
                ev.synchronize()                          # the pinned buffers are free before they are let go
    return out


def _fill_from_file(f, path: str, offsets, frame_bytes: int):
    def fill(rows: np.ndarray, at: int, k: int) -> None:
        for j in range(k):
            f.seek(offsets(at + j))
            got = f.readinto(memoryview(rows[j]).cast("B"))
            if got != frame_bytes:
                raise IOError(f"{path}: frame {at + j} is cut short: {got} of {frame_bytes} bytes")
    return fill


def load_y4m_device(path: str, device, order: str = "bgr", *, start: int = 0, count: Optional[int] = None,
                    chunk_frames: Optional[int] = None) -> torch.Tensor:
    """Frames [start, start + count) of a YUV4MPEG2 file (`count=None`: to the end) as one resident [count,H,W,3] u8
    clip, `order` "bgr" (what the restorers take, as decoded frames are in the reference) or "rgb".  `parse_y4m` finds
    the payloads; they are read with `readinto` straight into a pinned [k, H*3//2, W] staging buffer, uploaded and
    converted by `i420_to_rgb_device` in chunks of `chunk_frames` frames - by default as many as make 32 MB of I420 (10
    frames at 1080p) - with the read and upload of one chunk overlapping the conversion of the one before.  The clip
    does not depend on the chunk size.  PARITY UNPINNED vs cv2 (module docstring)."""
    if order not in ("rgb", "bgr"):
        raise ValueError('load_y4m_device: order must be "rgb" or "bgr"')
    info = parse_y4m(path)
    start, count = _window(info.frame_count, start, count, os.fspath(path))
    dev = L.resolve_device(device)
    with open(path, "rb", buffering=0) as f:
        fill = _fill_from_file(f, os.fspath(path), lambda i: info.frame_offsets[start + i], info.frame_bytes)
        return _planes_to_clip(fill, count, info.height, info.width, dev, order, chunk_frames)


def yuv420p_frame_count(size: int, width: int, height: int, what: str = "yuv420p") -> int:
    """How many I420 frames of `width` x `height` make `size` bytes; ValueError where the size is odd or not positive,
    or the bytes are no whole number of frames (the usual cause: a wrong width or height).  Host."""
    width, height = int(width), int(height)
    if width <= 0 or height <= 0 or width % 2 or height % 2:
        raise ValueError(f"{what}: I420 needs an even, positive width and height, got {width} x {height}")
    frame_bytes = width * height * 3 // 2
    if size % frame_bytes:
        raise ValueError(f"{what}: {size} bytes are not a whole number of {width} x {height} I420 frames of {frame_bytes} bytes "
                         "(a wrong width or height?)")
    return size // frame_bytes


def load_yuv420p_device(source: Union[str, bytes, bytearray, memoryview], width: int, height: int, device, order: str = "bgr", *,
                        start: int = 0, count: Optional[int] = None, chunk_frames: Optional[int] = None) -> torch.Tensor:
    """The inverse of `convert_frames_to_yuv420p`: raw I420 frames, one after the other - a `.yuv` path, or the bytes -
    as one resident [count,H,W,3] u8 clip; windows, chunks and `order` as in `load_y4m_device`.  A size that is not a
    whole number of frames raises ValueError.  PARITY UNPINNED vs cv2 (module docstring)."""
    if order not in ("rgb", "bgr"):
        raise ValueError('load_yuv420p_device: order must be "rgb" or "bgr"')
    in_memory = isinstance(source, (bytes, bytearray, memoryview))
    what = f"{len(source)} bytes of yuv420p" if in_memory else os.fspath(source)
    size = len(source) if in_memory else os.path.getsize(source)
    total = yuv420p_frame_count(size, width, height, what)
    start, count = _window(total, start, count, what)
    frame_bytes = int(width) * int(height) * 3 // 2
    dev = L.resolve_device(device)
    if in_memory:
        flat = np.frombuffer(source, np.uint8)

        def fill(rows: np.ndarray, at: int, k: int) -> None:
            rows.reshape(-1)[:] = flat[(start + at) * frame_bytes:(start + at + k) * frame_bytes]

        return _planes_to_clip(fill, count, int(height), int(width), dev, order, chunk_frames)
    with open(source, "rb", buffering=0) as f:
        fill = _fill_from_file(f, what, lambda i: (start + i) * frame_bytes, frame_bytes)
        return _planes_to_clip(fill, count, int(height), int(width), dev, order, chunk_frames)


def read_y4m(y4m_path: str, device="cuda:0", order: str = "rgb"):
    """The host-to-host convenience next to `write_y4m`: (frames, framerate) - the [H,W,3] u8 frames of the file,
    converted on the device, and its frame rate (None where the header has none).
    PARITY UNPINNED vs cv2 (module docstring)."""
    info = parse_y4m(y4m_path)
    arr = load_y4m_device(y4m_path, device, order).cpu().numpy()
    return [arr[i] for i in range(arr.shape[0])], info.framerate


# ----------------------------------------------------------------------------- host numpy: importance and ROI maps
def calculate_importance_scores(frames, block_size, alpha, beta, complexities, foreground_masks) -> List[np.ndarray]:
    """utils.py:665-688 (= presley.py:129-152).  HOST numpy.  `complexities` carries `.SC` and `.TC`, `[F,By,Bx]` each;
    `foreground_masks` is `[F,By,Bx]`; `frames` and `block_size` are not read (as in the reference).  In the arrays' own
    dtype and the reference's order: frame f mixes alpha SC[f] + (1 - alpha) TC[f + 1] (the last frame is SC alone),
    is smoothed as beta c[f] + (1 - beta) c[f - 1] (the first frame is itself), multiplied by the mask with every
    value under 0.5 replaced by -1, and normalised per frame by (x - min) / (max - min + 1e-8).  The masks are copied,
    never written."""
    sc, tc = complexities.SC, complexities.TC
    mixed = np.zeros_like(sc)
    mixed[:-1] = alpha * sc[:-1] + (1 - alpha) * tc[1:]
    mixed[-1] = sc[-1]
    smooth = np.zeros_like(mixed)
    smooth[0] = mixed[0]
    smooth[1:] = beta * mixed[1:] + (1 - beta) * mixed[:-1]
    sign = np.array(foreground_masks, copy=True)
    sign[sign < 0.5] = -1.0
    smooth *= sign
    low = smooth.min(axis=(1, 2), keepdims=True)
    high = smooth.max(axis=(1, 2), keepdims=True)
    scores = (smooth - low) / (high - low + 1e-8)
    return [scores[f] for f in range(len(scores))]


def kvazaar_delta_qp(importance: np.ndarray, base_qp: int, qp_range: int = 15) -> np.ndarray:
    """One frame of `create_kvazaar_roi_file`: (1 - importance) * 2 * qp_range - qp_range in the array's dtype (1 ->
    -qp_range, 0 -> +qp_range), clipped to +-14 (Kvazaar's limit), then to [0 - base_qp, 51 - base_qp] so the final QP
    is a HEVC one, then cut to int8 toward zero.  HOST numpy; int8 [By,Bx]."""
    delta = (1.0 - np.asarray(importance)) * 2 * qp_range - qp_range
    delta = np.clip(delta, -KVAZAAR_DELTA_LIMIT, KVAZAAR_DELTA_LIMIT)
    delta = np.clip(delta, HEVC_QP[0] - base_qp, HEVC_QP[1] - base_qp)
    return delta.astype(np.int8)


def create_kvazaar_roi_file(importance_scores: List[np.ndarray], roi_path: str, base_qp: int, qp_range: int = 15) -> None:
    """utils.py:1026-1053.  HOST numpy.  Binary; per frame an int32 pair (grid width, grid height), then the int8
    `kvazaar_delta_qp` map in row order."""
    with open(roi_path, "wb") as f:
        for importance in importance_scores:
            rows, cols = importance.shape
            f.write(np.array([cols, rows], dtype=np.int32).tobytes())
            f.write(kvazaar_delta_qp(importance, base_qp, qp_range).tobytes())


def _area_axis(values: np.ndarray, dst: int) -> np.ndarray:
    """ResizeArea along axis 0 of a float32 array: out[d] = sum of weight * values[s] over the computeResizeAreaTab
    entries of (len -> dst), float32, in table order (the first product starts the sum)."""
    out = np.zeros((dst,) + values.shape[1:], np.float32)
    started = [False] * dst
    for d, s, weight in area_table(values.shape[0], dst):
        term = values[s] * weight
        out[d] = out[d] + term if started[d] else term
        started[d] = True
    return out


def resize_area_f32(grid: np.ndarray, cols: int, rows: int) -> np.ndarray:
    """cv2.resize(float32 grid, (cols, rows), interpolation=INTER_AREA) onto a strictly smaller grid, restated from
    OpenCV 4.x.  A whole ratio in both axes is `ResizeAreaFast`: the cell's values summed in float32, row by row, then
    times `1.f / area`.  Otherwise `ResizeArea`: every source row reduced along x over the `computeResizeAreaTab`
    table (`degrade.area_table`), the rows then combined over the y table, float32 in table order.  HOST numpy.
    PARITY UNPINNED vs cv2 (module docstring)."""
    grid = np.ascontiguousarray(grid, np.float32)
    src_rows, src_cols = grid.shape
    if src_rows <= rows or src_cols <= cols:
        raise ValueError(f"resize_area: a {src_rows} x {src_cols} grid is not larger than {rows} x {cols} in both axes")
    if src_rows % rows == 0 and src_cols % cols == 0:
        fy, fx = src_rows // rows, src_cols // cols
        cells = grid.reshape(rows, fy, cols, fx)
        total = np.zeros((rows, cols), np.float32)
        for j in range(fy):
            for i in range(fx):
                total = total + cells[:, j, :, i]
        return total * np.float32(1.0 / (fy * fx))
    along_x = _area_axis(np.ascontiguousarray(grid.T), cols).T          # [src_rows, cols]
    return _area_axis(np.ascontiguousarray(along_x), rows)


def svtav1_delta_qp(importance: np.ndarray, base_crf: int, qp_range: int, width: int, height: int) -> np.ndarray:
    """One frame of `create_svtav1_roi_file`: the importance as float32, area-resized (`resize_area_f32`) onto the
    ceil(height / 64) x ceil(width / 64) superblock grid, cut to the 8 segment levels clip(int32(v * 8), 0, 7), mapped
    to qp_range - level * 2 * qp_range // 7 and clipped to [0 - base_crf, 63 - base_crf].  HOST numpy; int [rows,
    cols].  An importance grid that is not larger than the superblock grid in both axes raises ValueError."""
    cols = (width + AV1_SUPERBLOCK - 1) // AV1_SUPERBLOCK
    rows = (height + AV1_SUPERBLOCK - 1) // AV1_SUPERBLOCK
    resized = resize_area_f32(np.asarray(importance).astype(np.float32), cols, rows)
    levels = np.clip((resized * AV1_SEGMENTS).astype(np.int32), 0, AV1_SEGMENTS - 1)
    delta = qp_range - (levels * 2 * qp_range // (AV1_SEGMENTS - 1))
    return np.clip(delta, AV1_QP[0] - base_crf, AV1_QP[1] - base_crf).astype(int)


def create_svtav1_roi_file(importance_scores: List[np.ndarray], roi_path: str, base_crf: int, qp_range: int, width: int,
                           height: int) -> None:
    """utils.py:1056-1092.  HOST numpy.  Text; per frame one line: the frame index, then the `svtav1_delta_qp` offsets
    of its 64 x 64 superblocks in row order, separated by blanks."""
    with open(roi_path, "w") as f:
        for index, importance in enumerate(importance_scores):
            offsets = svtav1_delta_qp(importance, base_crf, qp_range, width, height).flatten()
            f.write(f"{index} " + " ".join(map(str, offsets)) + "\n")


# ----------------------------------------------------------------------------- the ROI approach with the project's own codec
def roi_levels_from_importance(importance_scores, qp_range: int = 15, base_qp: int = 25) -> np.ndarray:
    """Importance scores ([By,Bx] per frame, 0..1, as `calculate_importance_scores` gives them) to the levels the device
    JPEG writer's `roi_levels=` takes: uint8 [n,By,Bx].  HOST numpy.  Per frame `kvazaar_delta_qp(importance, base_qp,
    qp_range)` - the offsets `create_kvazaar_roi_file` would write - less the fixed floor max(-min(qp_range, 14),
    -base_qp), the offset of importance 1: importance 1 is level 0, the file's own quality, and every QP above it is a
    level.  The floor is fixed, not the clip's minimum, so a frame's levels do not depend on what else is in the clip.
    With the reference's Kvazaar default, base_qp = 48, the offsets are clipped at 51 - 48 = +3 and the levels end at 3
    plus the floor's 14; the default here, 25, leaves the whole +-14.  elvis.py's removability maps (high: removable)
    go in as 1 - removability."""
    floor = max(-min(int(qp_range), KVAZAAR_DELTA_LIMIT), -int(base_qp))
    from .jpeg_write import jpeg_roi_levels
    frames = [jpeg_roi_levels(kvazaar_delta_qp(importance, base_qp, qp_range), floor) for importance in importance_scores]
    if not frames:
        return np.zeros((0, 1, 1), np.uint8)
    return np.stack(frames, axis=0)


def encode_with_roi_device(frames_d: torch.Tensor, importance_scores, block_size: int, *, quality: int = 95, target_bytes: Optional[int] = None,
                           qp_range: int = 15, base_qp: int = 25, subsampling: str = "420", order: str = "bgr", restart_rows: int = 1,
                           optimize: bool = False):
    """The reference's ROI approach end to end on a resident clip, with the project's intra codec in the encoder's place
    (`encode_with_roi`, elvis.py:2013-2118; `create_kvazaar_roi_file` + `encode_kvazaar`, utils.py:1026-1053): the
    importance scores become levels (`roi_levels_from_importance`), with `target_bytes` (the clip's budget, bitrate * n /
    fps / 8) `jpeg_write.jpeg_quality_for_bytes` finds the quality inside 1..`quality` whose files fit it, and
    `jpeg_write.jpeg_roundtrip_device` encodes and decodes at that quality with the map.  `block_size`: the luma pixels
    of a cell of the importance grid, a multiple of 8.  Returns (the decoded resident clip, the bytes of every frame's
    file, int64 [n]; the quality used; the levels, uint8 [n,By,Bx]).  The files are baseline JPEG with a dead zone per
    block: nothing is claimed about what x265, Kvazaar or SVT-AV1 would make of the same maps.  `optimize=True` codes
    every frame with its own optimal Huffman tables (`jpeg_write.encode_jpeg_device`), in the search and in the round
    trip: a dead zone moves the symbol statistics towards long runs and EOBs, where the Annex K tables fit worst."""
    from . import jpeg_write
    levels = roi_levels_from_importance(importance_scores, qp_range, base_qp)
    kw = dict(restart_rows=restart_rows, roi_levels=levels, roi_block_size=block_size)
    if jpeg_write._check_optimize(optimize, "encode_with_roi_device"):
        kw["optimize"] = True
    if target_bytes is not None:
        quality = jpeg_write.jpeg_quality_for_bytes(frames_d, target_bytes, quality, subsampling, order, **kw)[0]
    decoded, nbytes = jpeg_write.jpeg_roundtrip_device(frames_d, quality, subsampling, order, **kw)
    return decoded, nbytes, quality, levels
