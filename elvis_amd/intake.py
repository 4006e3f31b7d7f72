"""Clip intake on the device: the first thing the reference does to its source video (presley.py:177-198) - every
decoded frame through `cv2.resize(frame, (width, height), interpolation=cv2.INTER_AREA)`, then `frame_stride`, then
`max_frames` - and the `cv2.resize(mask, ..., interpolation=cv2.INTER_NEAREST)` it applies to masks (presley.py:427, 846,
867, 884; elvis.py:206, 564, 4578).  Kernels: csrc/resize.hip.

    resize_area_device / resize_area              INTER_AREA of a resident clip / of one host image
    resize_nearest_device / resize_masks_nearest_device   INTER_NEAREST, resident / host to host
    intake_device                                 stride, cap, resize of a resident clip
    load_clip_device                              a .y4m or raw .yuv file to the working-size resident clip

INTER_AREA (`resize_area_device`): with both ratios whole, the integer box sum - a copy at 1x1, (sum + 2) >> 2 at 2x2,
otherwise rint(float32(sum) * float32(1.0 / (fx * fy))), half to even; with a fractional ratio on either axis,
`ResizeArea_<uchar, float>` on both, each axis with its own `degrade.area_table`, every product and every sum rounded to
float32 on its own, in table order.  Any ratio >= 1 on each axis.

PARITY UNPINNED vs cv2: OpenCV is absent from the build and GPU environments, so its rules are restated from OpenCV
4.x; the device output is bit-exact with the numpy statement in tests/_resize_ref.py, not checked against cv2 itself.
DEPARTURE: a destination larger than the source on either axis raises ValueError naming the axis; cv2 switches to its
area-mode bilinear there, which is not built.
"""
from __future__ import annotations

import functools
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .degrade import area_table

CHANNELS = (1, 3, 4)
TILE_VALUES = 1024                      # destination values (pixel x channel) of a workgroup's tile, at most
TILE_WIDTH = 64                         # destination columns of a tile, before a steep x ratio narrows it
LDS_LIMIT = 64 * 1024                   # bytes of LDS a workgroup may ask for
LDS_TARGET = 16 * 1024                  # ... and what a chunk of source rows is sized to: several workgroups per CU
INTAKE_CHUNK_BYTES = 256 << 20          # source RGB a `load_clip_device` window holds by default
_DEVICE_TABLES: Dict[tuple, tuple] = {}


# ----------------------------------------------------------------------------- tables and the tile plan (host)
@functools.lru_cache(maxsize=256)
def axis_tables(src: int, dst: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """`degrade.area_table(src, dst)` in the kernel's three arrays: start int32 [dst + 1] (the entries of destination d
    are start[d] .. start[d + 1]), first int32 [dst] (the source index of d's first entry; a destination's entries are
    consecutive source indices) and the float32 weights.  Cached; the arrays are read-only."""
    tab = area_table(int(src), int(dst))
    owner = np.array([t[0] for t in tab], np.int64)
    source = np.array([t[1] for t in tab], np.int64)
    start = np.searchsorted(owner, np.arange(dst + 1)).astype(np.int32)
    if (np.diff(start) < 1).any() or (np.diff(owner) < 0).any():
        raise AssertionError(f"area_table({src}, {dst}) leaves a destination index without entries")
    first = source[start[:-1]].astype(np.int32)
    if not np.array_equal(source, first[owner] + (np.arange(len(tab)) - start[owner])):
        raise AssertionError(f"area_table({src}, {dst}): a destination's entries are not consecutive source indices")
    out = (start, first, np.array([t[2] for t in tab], np.float32))
    for a in out:
        a.setflags(write=False)
    return out


def _reach(start: np.ndarray, first: np.ndarray, span: int) -> int:
    """The most source indices a tile of `span` destination indices reads."""
    d0 = np.arange(0, len(first), span)
    d1 = np.minimum(d0 + span, len(first)) - 1
    return int((first[d1] + (start[d1 + 1] - start[d1]) - first[d0]).max())


@functools.lru_cache(maxsize=256)
def _plan(hs: int, ws: int, hd: int, wd: int, c: int) -> Tuple[int, int, int, int]:
    """(th, tw, rows_per_chunk, row_stride) of `elvis_resize_area_u8`; row_stride 0: the source is read in place."""
    xstart, xfirst, _ = axis_tables(ws, wd)
    ystart, yfirst, _ = axis_tables(hs, hd)
    tw = min(wd, TILE_WIDTH)
    while True:
        row_stride = (_reach(xstart, xfirst, tw) * c + 3 + 3) & ~3      # the segment at any alignment, in whole dwords
        if row_stride <= LDS_LIMIT or tw == 1:
            break
        tw = (tw + 1) // 2
    th = min(hd, max(1, TILE_VALUES // (tw * c)))
    if row_stride > LDS_LIMIT:
        return th, tw, 1, 0
    rows = max(1, min(_reach(ystart, yfirst, th), LDS_TARGET // row_stride))
    return th, tw, rows, row_stride


def resize_area_plan(hs: int, ws: int, hd: int, wd: int, c: int) -> Tuple[int, int, int]:
    """(th, tw, LDS bytes) of the area resize's workgroup for `hs x ws -> hd x wd` with `c` channels: the tile of
    destination rows and columns it owns - at most `TILE_VALUES` values, `TILE_WIDTH` columns unless the x ratio is so
    steep that one source row's share does not fit the LDS - and the bytes of the chunk of source rows it streams
    through LDS (0: one destination column's share of a source row exceeds `LDS_LIMIT`, the kernel reads the source in
    place).  Host."""
    hs, ws, hd, wd, c = int(hs), int(ws), int(hd), int(wd), int(c)
    _check_sizes("resize_area_plan", hs, ws, hd, wd)
    if c not in CHANNELS:
        raise ValueError(f"resize_area_plan: {c} channels (C in {CHANNELS})")
    th, tw, rows, row_stride = _plan(hs, ws, hd, wd, c)
    return th, tw, rows * row_stride


def _check_sizes(who: str, hs: int, ws: int, hd: int, wd: int) -> None:
    if hd < 1 or wd < 1:
        raise ValueError(f"{who}: the output size must be positive, got {hd}x{wd}")
    if hd > hs:
        raise ValueError(f"{who}: the output height {hd} is larger than the source height {hs}; INTER_AREA upscaling "
                         "(cv2's area-mode bilinear) is not built")
    if wd > ws:
        raise ValueError(f"{who}: the output width {wd} is larger than the source width {ws}; INTER_AREA upscaling "
                         "(cv2's area-mode bilinear) is not built")


def _device_tables(hs: int, ws: int, hd: int, wd: int, device) -> tuple:
    key = (hs, ws, hd, wd, str(device))
    hit = _DEVICE_TABLES.get(key)
    if hit is None:
        if len(_DEVICE_TABLES) > 64:
            _DEVICE_TABLES.clear()
        hit = _DEVICE_TABLES[key] = tuple(torch.from_numpy(np.array(a)).to(device)
                                          for a in axis_tables(ws, wd) + axis_tables(hs, hd))
    return hit


# ----------------------------------------------------------------------------- the device forms
def _chk_in(x_d, who: str, ranks: Sequence[int]) -> None:
    if (not isinstance(x_d, torch.Tensor) or x_d.dtype != torch.uint8 or x_d.dim() not in ranks or not x_d.is_cuda
            or not x_d.is_contiguous() or (x_d.dim() == 4 and x_d.shape[3] not in CHANNELS) or 0 in x_d.shape):
        shapes = "[n,H,W,C]" if tuple(ranks) == (4,) else "[n,H,W,C] or [n,H,W]"
        raise ValueError(f"{who} takes a contiguous uint8 {shapes} tensor on the device, C in {CHANNELS}")


def _out(x_d: torch.Tensor, shape: tuple, out, who: str) -> torch.Tensor:
    """`out` goes to the kernel as a bare pointer: it must be exactly the result - shape, uint8, device, contiguous."""
    if out is None:
        return torch.zeros(shape, dtype=torch.uint8, device=x_d.device)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != x_d.device \
            or tuple(out.shape) != tuple(shape):
        raise ValueError(f"{who}: out must be a contiguous uint8 tensor of shape {tuple(shape)} on the input's device")
    return out


def resize_area_device(frames_d: torch.Tensor, out_h: int, out_w: int, out=None) -> torch.Tensor:
    """cv2.resize(frame, (out_w, out_h), interpolation=cv2.INTER_AREA) of every frame of a resident uint8 [n,H,W,C]
    clip, C in {1, 3, 4}, out_h <= H and out_w <= W at any ratio, in one launch (`elvis_resize_area_u8`; the rule is in
    the module docstring).  `out`, when given, must be exactly the result: [n,out_h,out_w,C], uint8, contiguous, on the
    frames' device.  ValueError: another dtype, rank, channel count or device, a non-positive size, an output larger than
    the source on either axis (the message names it), a wrong `out`.
    PARITY UNPINNED vs cv2 (module docstring)."""
    who = "resize_area_device"
    _chk_in(frames_d, who, (4,))
    n, hs, ws, c = frames_d.shape
    hd, wd = int(out_h), int(out_w)
    _check_sizes(who, hs, ws, hd, wd)
    out = _out(frames_d, (n, hd, wd, c), out, who)
    th, tw, rows, row_stride = _plan(hs, ws, hd, wd, c)
    xstart, xfirst, _ = axis_tables(ws, wd)
    ystart, yfirst, _ = axis_tables(hs, hd)
    with torch.cuda.device(frames_d.device):
        xs_d, xf_d, xw_d, ys_d, yf_d, yw_d = _device_tables(hs, ws, hd, wd, frames_d.device)
        L.check(L.lib().elvis_resize_area_u8(L.ptr(frames_d), L.ptr(out), n, hs, ws, hd, wd, c, xstart.ctypes.data,
                                             xfirst.ctypes.data, ystart.ctypes.data, yfirst.ctypes.data, L.ptr(xs_d), L.ptr(xf_d),
                                             L.ptr(xw_d), L.ptr(ys_d), L.ptr(yf_d), L.ptr(yw_d), th, tw, rows, row_stride,
                                             L.stream_handle(frames_d.device)), frames_d.device)
    return out


def resize_nearest_device(x_d: torch.Tensor, out_h: int, out_w: int, out=None) -> torch.Tensor:
    """cv2.resize(x, (out_w, out_h), interpolation=cv2.INTER_NEAREST) of every image of a resident uint8 [n,H,W,C]
    (C in {1, 3, 4}) or [n,H,W] tensor, up or down: destination index d reads source index floor(d * src / dst) in
    integers on each axis, the rule of `tiler._nearest_rows` (`elvis_resize_nearest_u8`).  `out` as in
    `resize_area_device`.  ValueError: another dtype, rank, channel count or device, a non-positive size, a wrong `out`."""
    who = "resize_nearest_device"
    _chk_in(x_d, who, (3, 4))
    n, hs, ws = x_d.shape[:3]
    c = x_d.shape[3] if x_d.dim() == 4 else 1
    hd, wd = int(out_h), int(out_w)
    if hd < 1 or wd < 1:
        raise ValueError(f"{who}: the output size must be positive, got {hd}x{wd}")
    out = _out(x_d, (n, hd, wd) + tuple(x_d.shape[3:]), out, who)
    with torch.cuda.device(x_d.device):
        L.check(L.lib().elvis_resize_nearest_u8(L.ptr(x_d), L.ptr(out), n, hs, ws, hd, wd, c, L.stream_handle(x_d.device)),
                x_d.device)
    return out


def intake_device(frames_d: torch.Tensor, width: int, height: int, frame_stride: int = 1, max_frames: Optional[int] = None) -> torch.Tensor:
    """presley.py:186-198 on a resident clip [n,H,W,C]: every frame INTER_AREA-resized to (width, height), then
    `[::frame_stride]`, then `[:max_frames]`.  The resize is per frame, so the frames are picked first and only what is
    left is resized: the same clip.  Returns [k,height,width,C] u8."""
    _chk_in(frames_d, "intake_device", (4,))
    picked = _pick(frames_d.shape[0], frame_stride, max_frames, "intake_device")
    kept = frames_d[picked.start:picked.stop:picked.step]
    return resize_area_device(kept if picked.step == 1 else kept.contiguous(), height, width)


def _pick(total: int, frame_stride, max_frames, who: str) -> range:
    """The source indices Presley keeps of `total` frames: [::frame_stride][:max_frames]."""
    if int(frame_stride) != frame_stride or int(frame_stride) < 1:
        raise ValueError(f"{who}: frame_stride must be an integer of at least 1, got {frame_stride!r}")
    if max_frames is not None and (int(max_frames) != max_frames or int(max_frames) < 0):
        raise ValueError(f"{who}: max_frames must be None or a non-negative integer, got {max_frames!r}")
    picked = range(0, total, int(frame_stride))
    return picked if max_frames is None else picked[:int(max_frames)]


# ----------------------------------------------------------------------------- host to host
def resize_area(image: np.ndarray, dsize: Tuple[int, int], device="cuda:0") -> np.ndarray:
    """cv2.resize(image, dsize, interpolation=cv2.INTER_AREA) of one uint8 image in host memory, (H,W,C) with C in
    {1, 3, 4} or (H,W); `dsize` is (width, height), cv2's order.  The result has the image's rank.
    PARITY UNPINNED vs cv2 (module docstring)."""
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim not in (2, 3):
        raise ValueError(f"resize_area takes one uint8 (H,W,C) or (H,W) image, got {image.shape} {image.dtype}")
    width, height = dsize
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        img = np.ascontiguousarray(image if image.ndim == 3 else image[..., None])
        out = resize_area_device(torch.from_numpy(img[None]).to(dev), height, width)[0].cpu().numpy()
    return out if image.ndim == 3 else out[..., 0]


def resize_masks_nearest_device(masks: Sequence[Optional[np.ndarray]], h: int, w: int, device="cuda:0") -> List[Optional[np.ndarray]]:
    """`complexity.resize_masks_nearest(masks, h, w)` with the gather on the device: uint8 2-D masks of any size, an
    entry that is None stays None; masks of one shape go up and through the kernel together.  Host to host."""
    out: List[Optional[np.ndarray]] = [None] * len(masks)
    groups: Dict[tuple, List[int]] = {}
    for i, mask in enumerate(masks):
        if mask is None:
            continue
        m = np.asarray(mask)
        if m.dtype != np.uint8 or m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
            raise ValueError(f"resize_masks_nearest_device: a mask must be a non-empty 2-D uint8 array, got {m.shape} {m.dtype}")
        groups.setdefault(m.shape, []).append(i)
    if groups:
        dev = L.resolve_device(device)
        with torch.cuda.device(dev):
            for idx in groups.values():
                stack = np.stack([np.asarray(masks[i]) for i in idx])
                small = resize_nearest_device(torch.from_numpy(stack).to(dev), h, w).cpu().numpy()
                for j, i in enumerate(idx):
                    out[i] = small[j]
    return out


# ----------------------------------------------------------------------------- file to working-size clip
def load_clip_device(path: str, width: int, height: int, device, *, src_width: Optional[int] = None,
                     src_height: Optional[int] = None, frame_stride: int = 1, max_frames: Optional[int] = None,
                     order: str = "rgb", chunk_frames: Optional[int] = None) -> Tuple[torch.Tensor, Optional[float]]:
    """presley.py:177-198 from a file: the frames `[::frame_stride][:max_frames]` of a `.y4m` file (its size from the
    header) or of a raw I420 `.yuv` file (`src_width`, `src_height`), decoded by `handoff.load_y4m_device` /
    `load_yuv420p_device` and INTER_AREA-resized to (width, height).  Returns ([k,height,width,3] u8 on the device,
    frame rate); the frame rate is None for raw files and for headers without one.  The file is read in windows of
    `chunk_frames` kept frames (by default as many as keep a window's source frames within 256 MB); a window starts at a
    kept frame and ends at one, the frames between kept ones are dropped before the resize, and nothing past the last
    kept frame is read.  The clip does not depend on `chunk_frames`.
    PARITY UNPINNED vs cv2 (module docstring)."""
    from . import handoff
    who = "load_clip_device"
    path = os.fspath(path)
    if order not in ("rgb", "bgr"):
        raise ValueError(f'{who}: order must be "rgb" or "bgr"')
    if chunk_frames is not None and (int(chunk_frames) != chunk_frames or int(chunk_frames) < 1):
        raise ValueError(f"{who}: chunk_frames must be an integer of at least 1")
    if path.lower().endswith(".y4m"):
        info = handoff.parse_y4m(path)
        hs, ws, total, rate = info.height, info.width, info.frame_count, info.framerate

        def load(start, count):
            return handoff.load_y4m_device(path, device, order, start=start, count=count, chunk_frames=chunk_frames)
    else:
        if src_width is None or src_height is None:
            raise ValueError(f"{who}: a raw .yuv input needs src_width= and src_height=")
        hs, ws, rate = int(src_height), int(src_width), None
        total = handoff.yuv420p_frame_count(os.path.getsize(path), ws, hs, path)

        def load(start, count):
            return handoff.load_yuv420p_device(path, ws, hs, device, order, start=start, count=count, chunk_frames=chunk_frames)
    width, height = int(width), int(height)
    _check_sizes(who, hs, ws, height, width)
    picked = _pick(total, frame_stride, max_frames, who)
    stride = picked.step
    dev = L.resolve_device(device)
    step = int(chunk_frames) if chunk_frames is not None else max(1, INTAKE_CHUNK_BYTES // (hs * ws * 3 * stride))
    with torch.cuda.device(dev):
        out = torch.zeros((len(picked), height, width, 3), dtype=torch.uint8, device=dev)
        for at in range(0, len(picked), step):
            k = min(step, len(picked) - at)
            window = load(picked[at], (k - 1) * stride + 1)[::stride]
            resize_area_device(window if stride == 1 else window.contiguous(), height, width, out=out[at:at + k])
    return out, rate
