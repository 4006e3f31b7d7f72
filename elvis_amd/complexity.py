"""Block complexity: the spatial (SC) and temporal (TC) complexity maps every server-side stage starts from, and the
removability scores the reference derives from them.

The reference takes the maps from EVCA: `calculate_removability_scores` (elvis.py:968-1224) runs it as a subprocess and
reads `evca_SC_blocks.csv` / `evca_TC_blocks.csv`; Presley calls `analyze_frames(np.array(frames),
EVCAConfig(block_size=...))` and reads `.SC` and `.TC` (presley.py:26,202).  EVCA is available neither to the reference
tree nor to this build, so its pixels can be neither generated nor pinned.

BUILD-DEFINED: `block_complexity_device` / `analyze_frames` are a DCT-energy block complexity in the published VCA form
behind the reference's call surface, on the device (`elvis_block_complexity_f64`, csrc/complexity.hip).  The contract is
the one of include/elvis_amd.h and DESIGN.md 7; tests/_complexity_ref.py states it in numpy float64 and the device agrees
with it to 1e-9 * max(1, |value|).  It does NOT claim parity with EVCA.
PINNED against the reference's own code (tests/golden/removability.npz): `removability_from_complexity`, the tail of
`calculate_removability_scores` (elvis.py:1172-1218), with `resize_masks_nearest` in the place of its one cv2 call - the
INTER_NEAREST index rule `tiler._nearest_rows` states.  Both run ON THE HOST in numpy: By x Bx values per frame.
"""
from __future__ import annotations

import threading
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib, ptr
from .ops import _s
from .tiler import _nearest_rows

BLOCK_SIZES = (8, 16, 32)
COMPLEXITY_CHUNK_BYTES = 64 << 20

_tables_lock = threading.Lock()
_tables = {}


# ----------------------------------------------------------------------------- the tables
def complexity_tables(block_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """The two float64 [B, B] tables the kernel is handed, built on the host so that no device cos / exp takes part:
    dct[k][m] = s_k cos(pi (2m + 1) k / 2B) with s_0 = sqrt(1 / B), s_k = sqrt(2 / B) (the orthonormal DCT-II), and
    weight[i][j] = exp(|(i j / B^2)^2 - 1|) with weight[0][0] = 0 (the DC term is excluded)."""
    if block_size not in BLOCK_SIZES:
        raise ValueError(f"block_complexity: block_size must be one of {BLOCK_SIZES}, got {block_size!r}")
    b = int(block_size)
    k = np.arange(b, dtype=np.float64)
    dct = np.cos(np.pi * (2.0 * k[None, :] + 1.0) * k[:, None] / (2.0 * b)) * np.sqrt(2.0 / b)
    dct[0] = np.sqrt(1.0 / b)
    weight = np.exp(np.abs((k[:, None] * k[None, :] / (b * b)) ** 2 - 1.0))
    weight[0, 0] = 0.0
    return np.ascontiguousarray(dct), np.ascontiguousarray(weight)


def _device_tables(block_size: int, device: torch.device):
    key = (int(block_size), str(device))
    with _tables_lock:
        if key not in _tables:
            _tables[key] = tuple(torch.from_numpy(t).to(device) for t in complexity_tables(block_size))
        return _tables[key]


# ----------------------------------------------------------------------------- the device form
def block_complexity_device(frames_d: torch.Tensor, block_size: int = 16, order: str = "rgb", prev: Optional[torch.Tensor] = None,
                            out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """SC and TC of every whole `block_size` block of a resident clip: frames [n,H,W,C] u8 on the device, C in {1, 3}
    -> two float64 [n, H // B, W // B] tensors.  C == 3 is reduced to the luma the encoder is handed (the Y of
    `rgb_to_i420_device`; `order` "rgb" or "bgr"), C == 1 is taken as it is.  `prev` [H,W,C] is the frame before
    frames[0]; without it TC[0] is 0.  `out`, when given, is the pair (sc, tc): float64, contiguous, of that shape, on
    the frames' device.  One launch; the bytes do not depend on how a clip is cut into calls.  A block size other than
    8, 16, 32, a frame smaller than one block, C other than 1, 3, another `order`, and non-uint8, non-contiguous or
    non-CUDA input raise ValueError before any launch.
    BUILD-DEFINED, not EVCA's pixels (module docstring)."""
    if block_size not in BLOCK_SIZES:
        raise ValueError(f"block_complexity: block_size must be one of {BLOCK_SIZES}, got {block_size!r}")
    if order not in ("rgb", "bgr"):
        raise ValueError('block_complexity: order must be "rgb" or "bgr"')
    if not isinstance(frames_d, torch.Tensor) or frames_d.dtype != torch.uint8 or not frames_d.is_cuda or not frames_d.is_contiguous():
        raise ValueError("block_complexity: frames must be a contiguous CUDA uint8 tensor")
    if frames_d.dim() != 4 or frames_d.shape[3] not in (1, 3):
        raise ValueError("block_complexity: frames must be [n, H, W, C] with 1 or 3 channels")
    n, h, w, c = frames_d.shape
    if h < block_size or w < block_size:
        raise ValueError(f"block_complexity: a {h} x {w} frame is smaller than one block of {block_size}")
    if prev is not None and (not isinstance(prev, torch.Tensor) or prev.dtype != torch.uint8 or not prev.is_contiguous()
                             or prev.device != frames_d.device or tuple(prev.shape) != (h, w, c)):
        raise ValueError(f"block_complexity: prev must be a contiguous uint8 tensor of shape {(h, w, c)} on the frames' device")
    shape = (n, h // block_size, w // block_size)
    if out is None:
        sc = torch.empty(shape, dtype=torch.float64, device=frames_d.device)
        tc = torch.empty(shape, dtype=torch.float64, device=frames_d.device)
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 2 or any(
                not isinstance(o, torch.Tensor) or o.dtype != torch.float64 or not o.is_contiguous() or o.device != frames_d.device
                or tuple(o.shape) != shape for o in out):
            raise ValueError(f"block_complexity: out must be two contiguous float64 tensors of shape {shape} on the frames' device")
        sc, tc = out
    if n:
        dct_d, weight_d = _device_tables(block_size, frames_d.device)
        check(lib().elvis_block_complexity_f64(ptr(frames_d), ptr(prev), ptr(dct_d), ptr(weight_d), ptr(sc), ptr(tc), n, h, w, c,
                                               int(order == "bgr"), int(block_size), _s(frames_d)), frames_d.device)
    return sc, tc


# ----------------------------------------------------------------------------- Presley's call surface
@dataclass
class EVCAConfig:
    """The one setting of EVCA's config that the reference passes (presley.py:202)."""
    block_size: int = 16


@dataclass
class BlockComplexity:
    """What `analyze_frames` returns: `.SC` and `.TC`, numpy float64 [F, By, Bx]."""
    SC: np.ndarray
    TC: np.ndarray


def analyze_frames(frames, config: Optional[EVCAConfig] = None, device="cuda:0", *, order: str = "rgb",
                   chunk_frames: Optional[int] = None) -> BlockComplexity:
    """presley.py:202's `analyze_frames(np.array(frames), EVCAConfig(block_size=...))` on the device: `.SC` and `.TC`
    of a host clip [F,H,W,C] (or [F,H,W], or a list of frames), uint8.  The clip is uploaded and analysed in chunks of
    `chunk_frames` frames - by default as many as make 64 MB - and the last frame of a chunk is carried, on the
    device, as `prev` of the next: the result does not depend on the chunk size.
    BUILD-DEFINED, not EVCA's pixels (module docstring)."""
    config = EVCAConfig() if config is None else config
    block = config.block_size
    if block not in BLOCK_SIZES:
        raise ValueError(f"analyze_frames: block_size must be one of {BLOCK_SIZES}, got {block!r}")
    clip = np.asarray(frames) if not isinstance(frames, np.ndarray) else frames
    if clip.ndim == 3:
        clip = clip[..., None]
    if clip.ndim != 4 or clip.dtype != np.uint8 or clip.shape[3] not in (1, 3):
        raise ValueError("analyze_frames: frames must be uint8 [F, H, W, C] with 1 or 3 channels (or [F, H, W])")
    count, h, w, c = clip.shape
    if h < block or w < block:
        raise ValueError(f"analyze_frames: a {h} x {w} frame is smaller than one block of {block}")
    if order not in ("rgb", "bgr"):
        raise ValueError('analyze_frames: order must be "rgb" or "bgr"')
    if chunk_frames is None:
        step = max(1, COMPLEXITY_CHUNK_BYTES // (h * w * c))
    elif int(chunk_frames) < 1:
        raise ValueError("chunk_frames must be at least 1")
    else:
        step = int(chunk_frames)
    sc = np.zeros((count, h // block, w // block), np.float64)
    tc = np.zeros_like(sc)
    if count == 0:
        return BlockComplexity(sc, tc)
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        last = None
        for at in range(0, count, step):
            chunk_d = torch.from_numpy(np.ascontiguousarray(clip[at:at + step])).to(dev)
            sc_d, tc_d = block_complexity_device(chunk_d, block, order, prev=last)
            sc[at:at + step] = sc_d.cpu().numpy()
            tc[at:at + step] = tc_d.cpu().numpy()
            last = chunk_d[-1]
    return BlockComplexity(sc, tc)


# ----------------------------------------------------------------------------- host numpy: masks and removability
def resize_masks_nearest(masks: Sequence[Optional[np.ndarray]], by: int, bx: int) -> List[Optional[np.ndarray]]:
    """`cv2.resize(mask, (bx, by), interpolation=cv2.INTER_NEAREST)` of every mask (elvis.py:1191, presley.py:204):
    destination index d reads source index floor(d * src_n / dst_n) in each axis (`tiler._nearest_rows`).  HOST numpy;
    every mask keeps its dtype, an entry that is None stays None."""
    out: List[Optional[np.ndarray]] = []
    for mask in masks:
        if mask is None:
            out.append(None)
            continue
        m = np.asarray(mask)
        if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
            raise ValueError(f"resize_masks_nearest: a mask must be a non-empty 2-D array, got shape {m.shape}")
        out.append(m[_nearest_rows(m.shape[0], by)][:, _nearest_rows(m.shape[1], bx)])
    return out


def normalize_array(arr: np.ndarray) -> np.ndarray:
    """elvis.py:864-867: (arr - min) / (max - min) over the whole array; an array without a spread comes back as it is."""
    min_val, max_val = arr.min(), arr.max()
    return (arr - min_val) / (max_val - min_val) if max_val > min_val else arr


def removability_from_complexity(spatial: np.ndarray, temporal: np.ndarray, masks: Optional[Sequence[Optional[np.ndarray]]] = None,
                                 alpha: float = 0.5, smoothing_beta: float = 1) -> np.ndarray:
    """The tail of `calculate_removability_scores` (elvis.py:1172-1218) from the two [F,By,Bx] maps on.  HOST numpy, in
    the arrays' own dtype and the reference's order of operations: each map is `normalize_array`-ed over the whole
    clip; frame f is alpha S[f] + (1 - alpha) T[f + 1], the last frame S[-1]; a frame's score is multiplied by 10 where
    its mask, nearest-resized to the block grid (`resize_masks_nearest`), is 0 - `masks` is None, or one 2-D array (any
    size) or None per frame, and a frame without a mask is left alone; with smoothing_beta < 1 and two frames or more,
    frame f >= 1 becomes beta s[f] + (1 - beta) s[f - 1] from the UNSMOOTHED scores; a last `normalize_array`.  The
    inputs are not written.  Returns [F,By,Bx] in [0, 1] (a clip without a spread comes back as it is)."""
    spatial, temporal = np.asarray(spatial), np.asarray(temporal)
    if spatial.ndim != 3 or spatial.shape != temporal.shape or spatial.shape[0] < 1:
        raise ValueError(f"removability: spatial and temporal must be [F, By, Bx] of one shape, got {spatial.shape} and {temporal.shape}")
    count, by, bx = spatial.shape
    temporal_3d = normalize_array(temporal)
    spatial_3d = normalize_array(spatial)
    scores = np.zeros_like(spatial_3d)
    scores[:-1] = alpha * spatial_3d[:-1] + (1 - alpha) * temporal_3d[1:]
    scores[-1] = spatial_3d[-1]
    if masks is not None:
        given = list(masks)[:count]
        for i, resized in enumerate(resize_masks_nearest(given, by, bx)):
            if resized is not None:
                scores[i][resized == 0] *= 10.0
    if smoothing_beta < 1 and count >= 2:
        smoothed = np.zeros_like(scores)
        smoothed[0] = scores[0]
        smoothed[1:] = smoothing_beta * scores[1:] + (1 - smoothing_beta) * scores[:-1]
        scores = smoothed
    return normalize_array(scores)
