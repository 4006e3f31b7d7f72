"""The hand-off to the encoders: RGB frames to I420 on the device, the Y4M container, the importance rule and the ROI maps.

What the reference does between its degraders and Kvazaar / SVT-AV1 / VMAF.  The pixel pass runs on the device:
`rgb_to_i420_device` is `cv2.cvtColor(frame, COLOR_RGB2YUV_I420)` over a resident `[n,H,W,3]` uint8 clip
(`elvis_rgb_to_i420_u8`, csrc/handoff.hip), and `convert_frames_to_yuv420p` (presley.py:217-223) and `write_y4m`
(utils.py:453-462, presley.py:590-599) keep the reference's names and argument order over it, so a clip leaves the
device as 1.5 bytes per pixel instead of 3.  The block-grid rules - `calculate_importance_scores` (utils.py:665-688,
presley.py:129-152), `create_kvazaar_roi_file` (utils.py:1026-1053), `create_svtav1_roi_file` (utils.py:1056-1092) -
touch By x Bx values per frame and RUN ON THE HOST in numpy.

PARITY UNPINNED vs cv2: OpenCV is absent from the build and GPU environments.  The colour conversion restates OpenCV
4.x's RGB8toYUV420pInvoker (20-bit fixed point, chroma taken from the even row / even column pixel of each 2x2 quad,
not averaged) and the one resize of the SVT-AV1 map restates its float INTER_AREA (`ResizeAreaFast` at a whole ratio in
both axes, `ResizeArea` over `computeResizeAreaTab` otherwise); the device is bit-exact with tests/_handoff_ref.py, not
checked against cv2 itself.  The importance rule, both ROI file formats and the Y4M framing ARE pinned against the
reference's own code (tests/golden/handoff.npz).
DEPARTURES: an odd frame height or width raises ValueError (cv2 raises its own error); an importance grid that is not
larger than the 64 x 64 superblock grid in both axes raises ValueError (cv2.resize leaves the area rule there).
"""
from __future__ import annotations

import io
from typing import List, Sequence

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
