"""Foreground masks on the device, in the slot where the reference runs UFO.

The slot in the reference:

  ufo_masks = segment_frames(np.array(reference_frames), device=device)      presley.py:203  -> segment_frames
  the mask files UFO writes and elvis.py:1187, 178-219, 536-575 read                          -> save_foreground_masks
  calculate_removability_scores (EVCA, then UFO, then the combination)       elvis.py:968-1224
                                                              -> drivers.calculate_removability_scores_device

and the clip form on a resident tensor, `foreground_masks_device`.

UFO is a trained video salient-object network; neither its architecture nor its weights are in the reference tree.  This
is a BUILD-DEFINED, training-free segmenter behind that call surface and IT IS NOT UFO: it claims no parity
with UFO's masks.  On the 1/4-resolution grid it compensates the global (camera) shift against the previous frame,
takes what still differs as motion, adds the colour distance to the frame's border, thresholds the sum by Otsu's
method, cleans the mask with a close and an open, and lets three consecutive frames vote.  A frame in which nothing or
nearly everything comes out as foreground is returned as all ones - the reference's meaning of "no mask"
(elvis.py:212-214): nothing is boosted.  Everything is integer arithmetic except the float64 threshold search;
tests/_segment_ref.py states it in numpy and the kernels (csrc/segment.hip) equal that bit for bit.

ITS DEFAULTS ARE UNTUNED AND UNMEASURED ON REAL VIDEO.  Sub-pixel camera motion and textured backgrounds are where it
is weakest: the shift is a whole number of reduced pixels (4 pixels), and a background as varied as the object has no
border colour to stand apart from.  The background a moving object uncovers counts as motion, so a mask trails behind
its object by the object's own step.

One call is ten launches and a memset on the current stream, nothing is read back, and the intermediates stay in a
workspace at documented offsets (include/elvis_amd.h) - `details=True` returns them as tensors.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, Optional, Union

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib, ptr
from .ops import _s

Q = 4                                  # the reduction (a constant of the kernels)
SHARE_DEN = 10000                      # max_share is compared in integers, to four decimals
MAX_RADIUS, MAX_DILATION, MAX_WEIGHT = 16, 4, 1024
MAX_SIDE, MAX_FRAMES = 16384, 4096
SEGMENT_CHUNK_BYTES = 64 << 20


@dataclass
class SegmentConfig:
    """The settings of the segmenter.  Untuned and unmeasured on real video (module docstring).
    radius: the global shift is searched in [-radius, radius]^2 reduced pixels (4 pixels each), 0..16.
    motion_weight, spatial_weight: the weights of the two terms, 1..1024.
    motion_floor, spatial_floor: a term is scaled by max(its maximum over the frame, its floor), so that noise alone
        is not stretched to full scale.  864 = 16 * 9 * 6 is six grey levels a pixel over the nine reduced pixels of the
        motion sum, 384 = 16 * 24 a colour distance of 24 a pixel.
    min_peak: a frame whose fused map stays below it has no foreground, 0..255.
    dilation: dilations after the close and the open, 0..4.
    max_share: a frame with a larger foreground share (to four decimals) is returned as all ones, (0, 1].
    temporal_vote: 2 of 3 over the frames t - 1, t, t + 1."""
    radius: int = 8
    motion_weight: int = 2
    spatial_weight: int = 1
    motion_floor: int = 864
    spatial_floor: int = 384
    min_peak: int = 48
    dilation: int = 1
    max_share: float = 0.7
    temporal_vote: bool = True


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_config(cfg: Optional[SegmentConfig], who: str) -> SegmentConfig:
    """`cfg` (None: the defaults) with every field inside its limits; ValueError otherwise."""
    cfg = SegmentConfig() if cfg is None else cfg
    if not isinstance(cfg, SegmentConfig):
        raise ValueError(f"{who}: cfg must be a SegmentConfig, got {type(cfg).__name__}")
    if not _is_int(cfg.radius) or not 0 <= cfg.radius <= MAX_RADIUS:
        raise ValueError(f"{who}: radius must be an integer in 0..{MAX_RADIUS}, got {cfg.radius!r}")
    if not _is_int(cfg.dilation) or not 0 <= cfg.dilation <= MAX_DILATION:
        raise ValueError(f"{who}: dilation must be an integer in 0..{MAX_DILATION}, got {cfg.dilation!r}")
    for name in ("motion_weight", "spatial_weight"):
        v = getattr(cfg, name)
        if not _is_int(v) or not 1 <= v <= MAX_WEIGHT:
            raise ValueError(f"{who}: {name} must be an integer in 1..{MAX_WEIGHT}, got {v!r}")
    for name in ("motion_floor", "spatial_floor"):
        v = getattr(cfg, name)
        if not _is_int(v) or not 1 <= v < 2 ** 31:
            raise ValueError(f"{who}: {name} must be a positive integer, got {v!r}")
    if not _is_int(cfg.min_peak) or not 0 <= cfg.min_peak <= 255:
        raise ValueError(f"{who}: min_peak must be an integer in 0..255, got {cfg.min_peak!r}")
    if isinstance(cfg.max_share, bool) or not isinstance(cfg.max_share, (int, float, np.integer, np.floating)) \
            or not 0 < cfg.max_share <= 1 or share_num(cfg.max_share) < 1:
        raise ValueError(f"{who}: max_share must be a number in (0, 1] (four decimals are kept), got {cfg.max_share!r}")
    if not isinstance(cfg.temporal_vote, (bool, np.bool_)):
        raise ValueError(f"{who}: temporal_vote must be a bool, got {cfg.temporal_vote!r}")
    return cfg


def share_num(max_share) -> int:
    """max_share as the kernels compare it: count * 10000 > share_num * pixels."""
    return int(round(float(max_share) * SHARE_DEN))


def _check_shape(h: int, w: int, m: int, cfg: SegmentConfig, who: str) -> None:
    if not Q <= h <= MAX_SIDE or not Q <= w <= MAX_SIDE:
        raise ValueError(f"{who}: a {h} x {w} frame is outside {Q}..{MAX_SIDE} on a side")
    need = 2 * cfg.radius + 1
    if h // Q < need or w // Q < need:
        raise ValueError(f"{who}: a {h} x {w} frame is {h // Q} x {w // Q} at 1/{Q} resolution, smaller than the "
                         f"2 * radius + 1 = {need} that radius = {cfg.radius} needs")
    if m > MAX_FRAMES:
        raise ValueError(f"{who}: {m} frames in one call (at most {MAX_FRAMES}, the halo frames included)")


def _align(v: int) -> int:
    return (v + 255) // 256 * 256


def workspace_layout(m: int, h: int, w: int, radius: int) -> Dict[str, int]:
    """The byte offsets of the workspace's sections (include/elvis_amd.h) and their `total`."""
    p, d2 = (h // Q) * (w // Q), (2 * radius + 1) ** 2
    sizes = (("red", m * 3 * p * 2), ("sad", m * d2 * 8), ("maxima", m * 8), ("hist", m * 1024), ("count", m * 4),
             ("shift", m * 8), ("means", m * 48), ("M", m * p * 2), ("S", m * p * 2), ("Mn", m * p), ("Sn", m * p),
             ("F", m * p), ("thr", m * 4), ("pre", m * p), ("voted", m * p))
    out, at = {}, 0
    for name, size in sizes:
        out[name] = at
        at = _align(at + size)
    out["total"] = at
    return out


def _details(ws: torch.Tensor, m: int, n: int, h: int, w: int, radius: int) -> Dict[str, torch.Tensor]:
    ry, rx, d = h // Q, w // Q, 2 * radius + 1
    p = ry * rx
    lay = workspace_layout(m, h, w, radius)

    def view(name, dtype, count, shape):
        size = count * torch.empty((), dtype=dtype).element_size()
        return ws[lay[name]:lay[name] + size].view(dtype).view(shape).clone()
    return {
        "red": view("red", torch.int16, m * 3 * p, (m, 3, ry, rx)).permute(0, 2, 3, 1).contiguous(),
        "sad": view("sad", torch.int64, m * d * d, (m, d, d)),
        "shift": view("shift", torch.int32, m * 2, (m, 2)),
        "means": view("means", torch.int32, m * 12, (m, 4, 3)),
        "M": view("M", torch.int16, m * p, (m, ry, rx)).to(torch.int32) & 0xFFFF,
        "S": view("S", torch.int16, m * p, (m, ry, rx)).to(torch.int32) & 0xFFFF,
        "Mn": view("Mn", torch.uint8, m * p, (m, ry, rx)),
        "Sn": view("Sn", torch.uint8, m * p, (m, ry, rx)),
        "F": view("F", torch.uint8, m * p, (m, ry, rx)),
        "thr": view("thr", torch.int32, m, (m,)),
        "pre": view("pre", torch.uint8, m * p, (m, ry, rx)),
        "voted": view("voted", torch.uint8, n * p, (n, ry, rx)),
        "count": view("count", torch.int32, n, (n,)),
    }


def _check_halo(t, name: str, most: int, like: torch.Tensor, who: str) -> int:
    if t is None:
        return 0
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.device != like.device or not t.is_contiguous() \
            or t.dim() != 4 or tuple(t.shape[1:]) != tuple(like.shape[1:]) or t.shape[0] > most:
        raise ValueError(f"{who}: {name} must be a contiguous uint8 tensor of at most {most} frame(s) of shape "
                         f"{tuple(like.shape[1:])} on the frames' device")
    return int(t.shape[0])


def foreground_masks_device(frames_d: torch.Tensor, order: str = "rgb", cfg: Optional[SegmentConfig] = None, *,
                            before: Optional[torch.Tensor] = None, after: Optional[torch.Tensor] = None, details: bool = False):
    """The foreground masks of a resident clip: frames [n,H,W,C] u8, C in {1, 3} (`order` "rgb" or "bgr" for C == 3)
    -> u8 [n,H,W] of 0 / 1, 1 = foreground; a frame without a usable mask is all ones.

    `before`: up to two frames preceding frames[0], `after`: up to one following the last, each [k,H,W,C] on the
    frames' device.  With the two frames before and the one after wherever the clip has them, the result does not
    depend on how a clip is cut into calls (one frame before means: that frame is the clip's first).
    `details=True` returns `(masks, intermediates)`: red [m,Ry,Rx,3] i16, sad [m,D,D] i64, shift [m,2], means, M, S,
    Mn, Sn, F, pre [m,Ry,Rx], thr [m] over the m = before + n + after frames, voted [n,Ry,Rx] and count [n].

    ValueError before any launch: a non-CUDA, non-contiguous or non-uint8 tensor, another `order`, a frame smaller at
    1/4 resolution than 2 * radius + 1 on a side, and every `cfg` field outside its limits (`check_config`).
    BUILD-DEFINED, not UFO; untuned and unmeasured on real video (module docstring)."""
    who = "foreground_masks_device"
    cfg = check_config(cfg, who)
    if order not in ("rgb", "bgr"):
        raise ValueError(f'{who}: order must be "rgb" or "bgr"')
    if not isinstance(frames_d, torch.Tensor) or frames_d.dtype != torch.uint8:
        raise ValueError(f"{who}: frames must be a contiguous CUDA uint8 tensor")
    if frames_d.dim() != 4 or frames_d.shape[3] not in (1, 3) or frames_d.shape[0] < 1:
        raise ValueError(f"{who}: frames must be [n, H, W, C] with n >= 1 and 1 or 3 channels")
    n, h, w, c = frames_d.shape
    _check_shape(h, w, n, cfg, who)                     # the shape first: a host tensor shows it as well
    if not frames_d.is_cuda or not frames_d.is_contiguous():
        raise ValueError(f"{who}: frames must be a contiguous CUDA uint8 tensor")
    nb = _check_halo(before, "before", 2, frames_d, who)
    na = _check_halo(after, "after", 1, frames_d, who)
    m = nb + n + na
    _check_shape(h, w, m, cfg, who)
    dev = frames_d.device
    with torch.cuda.device(dev):
        total = lib().elvis_segment_workspace_bytes(m, h, w, cfg.radius)
        if total == 0 or total != workspace_layout(m, h, w, cfg.radius)["total"]:
            raise RuntimeError(f"{who}: the library's workspace layout ({total} bytes) is not this module's")
        ws = torch.empty(total, dtype=torch.uint8, device=dev)
        masks = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
        check(lib().elvis_segment_foreground_u8(ptr(frames_d), ptr(before) if nb else 0, nb, ptr(after) if na else 0, na,
                                                ptr(masks), ptr(ws), total, n, h, w, c, int(order == "bgr"), cfg.radius,
                                                cfg.motion_weight, cfg.spatial_weight, cfg.motion_floor, cfg.spatial_floor,
                                                cfg.min_peak, cfg.dilation, share_num(cfg.max_share), int(cfg.temporal_vote),
                                                _s(frames_d)), dev)
        if details:
            return masks, _details(ws, m, n, h, w, cfg.radius)
    return masks


def _host_clip(frames, who: str) -> np.ndarray:
    clip = frames if isinstance(frames, np.ndarray) else np.asarray(frames)
    if clip.ndim == 3:
        clip = clip[..., None]
    if clip.ndim != 4 or clip.dtype != np.uint8 or clip.shape[3] not in (1, 3):
        raise ValueError(f"{who}: frames must be uint8 [F, H, W, C] with 1 or 3 channels (or [F, H, W]), an array or a list of frames")
    return clip


def segment_frames(frames, device="cuda:0", *, order: str = "rgb", cfg: Optional[SegmentConfig] = None,
                   chunk_frames: Optional[int] = None) -> np.ndarray:
    """presley.py:203's `segment_frames(np.array(reference_frames), device=device)`: an array or a list of RGB frames
    [F,H,W,3] uint8 (`order="bgr"` for frames as OpenCV decodes them; [F,H,W] or one channel is taken as luma) -> numpy
    uint8 [F,H,W] of 0 / 1, what presley.py:204 resizes to the block grid and `calculate_importance_scores` takes.

    The clip is uploaded in chunks of `chunk_frames` frames - by default as many as make 64 MB - each with the two
    frames before it and the one after it, so the result is the same for every chunk size.
    BUILD-DEFINED, NOT UFO: no parity with UFO's masks is claimed; the defaults are untuned and unmeasured on real
    video (module docstring)."""
    who = "segment_frames"
    cfg = check_config(cfg, who)
    if order not in ("rgb", "bgr"):
        raise ValueError(f'{who}: order must be "rgb" or "bgr"')
    clip = _host_clip(frames, who)
    count, h, w, c = clip.shape
    if chunk_frames is None:
        step = max(1, SEGMENT_CHUNK_BYTES // max(1, h * w * c))
    elif not _is_int(chunk_frames) or chunk_frames < 1:
        raise ValueError(f"{who}: chunk_frames must be an integer of at least 1")
    else:
        step = int(chunk_frames)
    step = min(step, MAX_FRAMES - 3)
    out = np.zeros((count, h, w), np.uint8)
    if count == 0:
        return out
    _check_shape(h, w, 1, cfg, who)
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        held, held_lo = None, 0                       # the resident frames [held_lo, held_lo + len(held))
        for a in range(0, count, step):
            b = min(count, a + step)
            lo, hi = max(0, a - 2), min(count, b + 1)
            have = held_lo + held.shape[0] if held is not None else lo
            parts = [held[lo - held_lo:]] if held is not None else []
            if hi > have:
                parts.append(torch.from_numpy(np.array(clip[have:hi], order="C")).to(dev))    # a copy: the caller's may be read-only
            held, held_lo = (parts[0] if len(parts) == 1 else torch.cat(parts)), lo
            masks = foreground_masks_device(held[a - lo:b - lo], order, cfg, before=held[:a - lo] if a > lo else None,
                                            after=held[b - lo:] if hi > b else None)
            out[a:b] = masks.cpu().numpy()
    return out


def save_foreground_masks(masks, directory: Union[str, os.PathLike]) -> None:
    """The masks as the files UFO leaves and elvis.py:1187, 178-219, 536-575 read: `{i+1:05d}.png` in `directory`, one
    gray channel, 0 / 255 (any non-zero value of `masks` [F,H,W] is foreground).  Written through `frameio.save_mask`."""
    from .frameio import save_mask
    arr = np.asarray(masks)
    if arr.ndim != 3 or arr.dtype.kind not in "biu":
        raise ValueError(f"save_foreground_masks: masks must be an integer or bool [F, H, W] array, got {arr.dtype} {arr.shape}")
    os.makedirs(os.fspath(directory), exist_ok=True)
    for i in range(arr.shape[0]):
        save_mask(np.where(arr[i] != 0, 255, 0).astype(np.uint8), os.path.join(os.fspath(directory), f"{i + 1:05d}.png"))


__all__ = ["SegmentConfig", "check_config", "foreground_masks_device", "save_foreground_masks", "segment_frames", "share_num",
           "workspace_layout"]
