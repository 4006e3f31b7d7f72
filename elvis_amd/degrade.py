"""Server-side per-block degrade filters on the device - what produces the hot path's
inputs, so benchmark and test clips are built on the GPU instead of by a python loop over 32 400 blocks.

`filter_frame_downsample` / `filter_frame_gaussian` keep the reference's names, arguments and return values
(elvis.py:2141-2196: BGR or RGB uint8 HWC image + per-block scores in [0,1] -> (filtered image, int32 map));
`filter_frame_dct` is the build's definition of the ELVIS v2 DCT degrade (the reference has none).
The `*_device` forms work on resident `[n,H,W,C]` uint8 tensors and `[n,By,Bx]` int32 maps.

Presley's adaptive degraders keep their names, argument order, defaults and return values too:
`degrade_adaptive_downsample` / `degrade_adaptive_blur` (utils.py:1101-1217) and `generate_degradation_map`,
`downscale_block`, `blur_block`, `degrade_frame`, `degrade_video_adaptive` (presley.py:968-1039), over
`degrade_scale_device` / `degrade_gaussian_fx_device`: raw scale factors 0, 2, 3, 4, ... (any ratio, INTER_AREA's
fractional-overlap table included), any block size in [2, 32], frames that are no multiple of the block (the rows and
columns past the last whole block come back unchanged), and the Gaussian in cv2's own CV_8U fixed point.

PARITY UNPINNED vs cv2 (Presley's functions): OpenCV is absent from the build and GPU environments, so its 8-bit rules
are restated from OpenCV 4.x (INTER_AREA at an integer ratio and by `computeResizeAreaTab` / `ResizeArea_<uchar,
float>` otherwise, the 11-bit INTER_LINEAR, the bit-exact 8.8 / 16.16 GaussianBlur); the device output is bit-exact
with the numpy restatement in tests/_presley_degrade_ref.py, not checked against cv2 itself.  The map rules and the
per-block control flow ARE pinned against the reference's own code (tests/golden/presley_degrade.npz).
DEPARTURE: an importance array (or a map) whose shape is not the block grid raises ValueError; the reference
bilinearly resizes the importance with cv2.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib, ptr
from .classical import gaussian_taps_u8
from .ops import _block_maps, _block_out, _check_image_grid, _chk_u8, _one_image, _s
from .recompose import frames_to_device, frames_to_host

DCT_LEVELS = 4
MAX_BLOCK = 32            # Presley's degraders: 2 <= block_size <= 32
MAX_ROUNDS = 64           # ELVIS_DEGRADE_MAX_ROUNDS
_TABLES: Dict[str, tuple] = {}
_AREA_TABLES: Dict[tuple, tuple] = {}


def gaussian_taps() -> Tuple[float, float, float]:
    """getGaussianKernel(5, 1.0): normalised in float64, rounded to float32; (k0, k1, k2) of (k0 k1 k2 k1 k0)."""
    k = np.exp(-np.arange(-2, 3, dtype=np.float64) ** 2 / 2.0)
    k = (k / k.sum()).astype(np.float32)
    return float(k[0]), float(k[1]), float(k[2])


def _dct_tables(device) -> tuple:
    key = str(device)
    if key not in _TABLES:
        u = np.arange(8, dtype=np.float64)[:, None]
        x = np.arange(8, dtype=np.float64)[None, :]
        basis = np.cos((2 * x + 1) * u * np.pi / 16.0) * np.sqrt(2.0 / 8.0)
        basis[0] *= np.sqrt(0.5)
        uv = (np.arange(8)[:, None] + np.arange(8)[None, :]).astype(np.float64)
        gain = np.stack([np.exp2(-lv * uv / 14.0) for lv in range(DCT_LEVELS)])
        _TABLES[key] = (torch.from_numpy(basis.astype(np.float32)).to(device), torch.from_numpy(gain.astype(np.float32)).to(device))
    return _TABLES[key]


def degrade_downsample_device(frames_d: torch.Tensor, levels_d: torch.Tensor, block_size: int, out=None) -> torch.Tensor:
    _chk_u8(frames_d)
    n, h, w, c = frames_d.shape
    m = _block_maps(levels_d, n, "degrade")
    out = _block_out(frames_d, block_size, out, "degrade")
    check(lib().elvis_degrade_downsample_u8(ptr(frames_d), ptr(m), ptr(out), n, h, w, c, block_size, m.shape[1], m.shape[2],
                                            _s(frames_d)), frames_d.device)
    return out


def degrade_gaussian_device(frames_d: torch.Tensor, rounds_d: torch.Tensor, block_size: int, out=None) -> torch.Tensor:
    _chk_u8(frames_d)
    n, h, w, c = frames_d.shape
    m = _block_maps(rounds_d, n, "degrade")
    out = _block_out(frames_d, block_size, out, "degrade")
    k0, k1, k2 = gaussian_taps()
    check(lib().elvis_degrade_gaussian_u8(ptr(frames_d), ptr(m), ptr(out), n, h, w, c, block_size, m.shape[1], m.shape[2],
                                          k0, k1, k2, _s(frames_d)), frames_d.device)
    return out


def degrade_dct_device(frames_d: torch.Tensor, levels_d: torch.Tensor, out=None) -> torch.Tensor:
    _chk_u8(frames_d)
    n, h, w, c = frames_d.shape
    m = _block_maps(levels_d, n, "degrade")
    basis, gain = _dct_tables(frames_d.device)
    out = _block_out(frames_d, 8, out, "degrade")
    check(lib().elvis_degrade_dct_u8(ptr(frames_d), ptr(m), ptr(out), ptr(basis), ptr(gain), DCT_LEVELS, n, h, w, c,
                                     m.shape[1], m.shape[2], _s(frames_d)), frames_d.device)
    return out


def _check_grid(image: np.ndarray, scores: np.ndarray, block_size: int):
    _check_image_grid(image, scores, block_size, "degrade filters", "scores {} do")


def filter_frame_downsample(image: np.ndarray, frame_scores: np.ndarray, block_size: int, device="cuda:0"):
    """elvis.py:2141-2169 on the device: levels = round(score * log2(block_size)); every block of level L is
    INTER_AREA-downscaled by 2**L and INTER_LINEAR-upscaled back.  Returns (image, int32 level map)."""
    _check_grid(image, frame_scores, block_size)
    levels = np.round(frame_scores * int(np.log2(block_size))).astype(np.int32)
    return _one_image(image, levels, device, degrade_downsample_device, block_size), levels


def filter_frame_gaussian(image: np.ndarray, frame_scores: np.ndarray, block_size: int, device="cuda:0", *,
                          arithmetic: str = "float32"):
    """elvis.py:2171-2196 on the device: rounds = round(score * 10) passes of GaussianBlur(5x5, sigma 1) per
    block (BORDER_REFLECT_101 at the block edges).  Returns (image, int32 rounds map).

    PARITY UNPINNED vs cv2.  arithmetic="float32" (the default): each pass is two float32 separable passes with the
    `getGaussianKernel(5, 1)` taps and ONE round-half-even uint8 cast (bit-exact with oracle/degrade_ref.py); a pixel
    can differ from OpenCV's by +-1 LSB per pass, and the passes compound (up to 10).  arithmetic="opencv": each pass
    is cv2.GaussianBlur's own CV_8U rule, restated - the 8.8 fixed-point taps 14 62 104 62 14, 16.16 accumulation, one
    rounding (`degrade_gaussian_fx_device`, bit-exact with tests/_presley_degrade_ref.py; block sizes 2..32).  cv2 is
    absent here and the reference holds no pixel fixture, so neither form is checked against cv2 itself; same control
    flow, block grid and border rule as the reference in both."""
    if arithmetic not in ("float32", "opencv"):
        raise ValueError('filter_frame_gaussian: arithmetic must be "float32" or "opencv"')
    _check_grid(image, frame_scores, block_size)
    rounds = np.round(frame_scores * 10).astype(np.int32)
    fn = degrade_gaussian_device if arithmetic == "float32" else degrade_gaussian_fx_device
    return _one_image(image, rounds, device, fn, block_size), rounds


def filter_frame_dct(image: np.ndarray, frame_scores: np.ndarray, block_size: int = 8, device="cuda:0"):
    """ELVIS v2 DCT degrade (build-defined): levels = round(score * 3); per 8x8 block the
    DCT coefficient (u,v) is scaled by 2^(-level*(u+v)/14).  Returns (image, int32 level map)."""
    if block_size != 8:
        raise ValueError("the DCT degrade works on 8x8 blocks")
    _check_grid(image, frame_scores, block_size)
    levels = np.round(frame_scores * (DCT_LEVELS - 1)).astype(np.int32)
    return _one_image(image, levels, device, degrade_dct_device), levels


# ----------------------------------------------------------------------------- Presley's adaptive degraders
def area_table(src: int, dst: int) -> List[Tuple[int, int, np.float32]]:
    """cv::computeResizeAreaTab for one axis of cv2.resize(INTER_AREA) from `src` to `dst` samples: the entries
    (destination index, source index, float32 weight) in OpenCV's order, scale = 1 / (dst / src) in float64."""
    scale = 1.0 / (dst / src)
    tab = []
    for dx in range(dst):
        f1 = dx * scale
        f2 = f1 + scale
        cell = min(scale, src - f1)
        s1, s2 = math.ceil(f1), min(math.floor(f2), src - 1)
        s1 = min(s1, s2)
        if s1 - f1 > 1e-3:
            tab.append((dx, s1 - 1, np.float32((s1 - f1) / cell)))
        for sx in range(s1, s2):
            tab.append((dx, sx, np.float32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            tab.append((dx, s2, np.float32(min(min(f2 - s2, 1.0), cell) / cell)))
    return tab


def area_tables(block_size: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The device tables of `elvis_degrade_scale_u8` for one block size, indexed by the target size d in
    [1, block_size // 2] (every d = max(1, block_size // scale) a scale >= 2 can give): starts int32
    [block_size // 2 + 1][block_size // 2 + 2] (the entries of destination i of target d are
    starts[d, i] .. starts[d, i + 1]), source indices int32 and weights float32."""
    hb = block_size // 2
    starts = np.zeros((hb + 1, hb + 2), np.int32)
    src, wgt = [], []
    for d in range(1, hb + 1):
        tab = area_table(block_size, d)
        if len(tab) > 2 * block_size:
            raise AssertionError("area table longer than the kernel's staging buffer")
        first = len(src)
        owners = [t[0] for t in tab]
        for i in range(d + 1):
            starts[d, i] = first + sum(1 for o in owners if o < i)
        src += [t[1] for t in tab]
        wgt += [t[2] for t in tab]
    return starts, np.asarray(src, np.int32), np.asarray(wgt, np.float32)


def _area_tables(device, block_size: int) -> tuple:
    key = (str(device), int(block_size))
    if key not in _AREA_TABLES:
        _AREA_TABLES[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in area_tables(block_size))
    return _AREA_TABLES[key]


def _presley_args(frames_d: torch.Tensor, map_d: torch.Tensor, block_size: int, out):
    """Checks shared by the two device forms; returns (map, out, whether the grid holds a block).  Rows and columns
    past the last whole block are not written by the kernels: without `out` the result starts as a copy of the frames
    when there are any; a given `out` keeps there what the caller put."""
    _chk_u8(frames_d)
    if frames_d.dim() != 4:
        raise ValueError("degrade: frames must be [n, H, W, C]")
    if not 2 <= int(block_size) <= MAX_BLOCK:
        raise ValueError(f"degrade: block_size must be in [2, {MAX_BLOCK}]")
    n, h, w, c = frames_d.shape
    if not 1 <= c <= 4:
        raise ValueError("degrade: 1..4 channels are supported")
    m = _block_maps(map_d, n, "degrade")
    if tuple(m.shape[1:]) != (h // block_size, w // block_size):
        raise ValueError(f"degrade: map {tuple(m.shape[1:])} does not match the block grid {(h // block_size, w // block_size)}")
    return m, _block_out(frames_d, block_size, out, "degrade"), m.shape[1] > 0 and m.shape[2] > 0


def degrade_scale_device(frames_d: torch.Tensor, scales_d: torch.Tensor, block_size: int, out=None) -> torch.Tensor:
    """Per block of scale >= 2: INTER_AREA to max(1, block_size // scale), INTER_LINEAR back (`downscale_block`,
    presley.py:978-983); a scale <= 1 copies the block.  frames [n,H,W,C] u8, scales [n,H//b,W//b] int32, any
    block_size in [2, 32]; pixels past the last whole block are not degraded (see `_presley_args` for `out`).
    PARITY UNPINNED vs cv2 (module docstring)."""
    m, out, any_block = _presley_args(frames_d, scales_d, block_size, out)
    if any_block:
        n, h, w, c = frames_d.shape
        starts, src, wgt = _area_tables(frames_d.device, block_size)
        check(lib().elvis_degrade_scale_u8(ptr(frames_d), ptr(m), ptr(out), n, h, w, c, int(block_size), m.shape[1], m.shape[2],
                                           ptr(starts), ptr(src), ptr(wgt), src.numel(), _s(frames_d)), frames_d.device)
    return out


def degrade_gaussian_fx_device(frames_d: torch.Tensor, rounds_d: torch.Tensor, block_size: int, out=None) -> torch.Tensor:
    """Per block, `rounds` passes of cv2.GaussianBlur(block, (5, 5), sigmaX=1.0) in its CV_8U fixed point (`blur_block`,
    presley.py:986-990); rounds <= 0 copies the block, more than 64 raises ValueError.  frames [n,H,W,C] u8, rounds
    [n,H//b,W//b] int32, any block_size in [2, 32]; pixels past the last whole block are not blurred.
    PARITY UNPINNED vs cv2 (module docstring)."""
    m, out, any_block = _presley_args(frames_d, rounds_d, block_size, out)
    if any_block:
        if int(m.max()) > MAX_ROUNDS:
            raise ValueError(f"degrade: more than {MAX_ROUNDS} blur rounds are not supported")
        n, h, w, c = frames_d.shape
        t = gaussian_taps_u8(1.0, 5)
        check(lib().elvis_degrade_gaussian_fx_u8(ptr(frames_d), ptr(m), ptr(out), n, h, w, c, int(block_size), m.shape[1],
                                                 m.shape[2], int(t[0]), int(t[1]), int(t[2]), _s(frames_d)), frames_d.device)
    return out


def generate_degradation_map(importance: np.ndarray, max_value: int) -> np.ndarray:
    """presley.py:968-975: clip(round((1 - importance) * max_value), 0, max_value) as int32.  np.round is half-to-even
    and the arithmetic stays in the array's own dtype (a float32 importance is not up-cast: that would move bin
    edges).  Host numpy."""
    inv_importance = 1 - np.asarray(importance)
    degradation_map = np.round(inv_importance * max_value).astype(np.int32)
    return np.clip(degradation_map, 0, max_value)


def _scale_map(importance: np.ndarray, max_scale: int) -> np.ndarray:
    """utils.py:1134-1149: bin = clip(floor((1 - importance) * max_scale), 0, max_scale - 1); bin 0 -> 0, bin k -> k + 1."""
    inv_importance = 1 - np.asarray(importance)
    bin_indices = np.clip(np.floor(inv_importance * max_scale).astype(np.int32), 0, max_scale - 1)
    return np.where(bin_indices == 0, 0, bin_indices + 1).astype(np.int32)


def _check_frame(frame: np.ndarray, grid_array: np.ndarray, block_size: int, what: str):
    if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or frame.ndim != 3:
        raise ValueError("degrade filters take uint8 (H,W,C) images")
    if not 2 <= int(block_size) <= MAX_BLOCK:
        raise ValueError(f"degrade: block_size must be in [2, {MAX_BLOCK}]")
    grid = (frame.shape[0] // block_size, frame.shape[1] // block_size)
    if np.shape(grid_array) != grid:
        raise ValueError(f"{what} {np.shape(grid_array)} does not match the block grid {grid} (it is not resized here)")


def _check_rounds(rounds: np.ndarray):
    if np.size(rounds) and int(np.max(rounds)) > MAX_ROUNDS:
        raise ValueError(f"degrade: more than {MAX_ROUNDS} blur rounds are not supported")


def degrade_adaptive_downsample(frame: np.ndarray, importance: np.ndarray, block_size: int, max_scale: int = 4,
                                device="cuda:0") -> Tuple[np.ndarray, np.ndarray]:
    """utils.py:1101-1168 on the device: scale = 0, 2, 3, ..., max_scale from the importance bins (`_scale_map`); every
    block of scale > 0 is INTER_AREA-resized to max(1, block_size // scale) and INTER_LINEAR-resized back; rows and
    columns past the last whole block are returned unchanged.  Returns (frame, int32 scale map).
    PARITY UNPINNED vs cv2; an importance that is not the block grid raises ValueError (module docstring)."""
    _check_frame(frame, importance, block_size, "importance")
    degradation_map = _scale_map(importance, max_scale)
    return _one_image(frame, degradation_map, device, degrade_scale_device, block_size), degradation_map


def degrade_adaptive_blur(frame: np.ndarray, importance: np.ndarray, block_size: int, max_rounds: int = 10,
                          device="cuda:0") -> Tuple[np.ndarray, np.ndarray]:
    """utils.py:1171-1217 on the device: rounds = clip(round((1 - importance) * max_rounds), 0, max_rounds) passes of
    GaussianBlur(5x5, sigma 1) per block, in cv2's CV_8U fixed point; rows and columns past the last whole block are
    returned unchanged.  Returns (frame, int32 rounds map).  max_rounds above 64 raises ValueError.
    PARITY UNPINNED vs cv2; an importance that is not the block grid raises ValueError (module docstring)."""
    _check_frame(frame, importance, block_size, "importance")
    degradation_map = generate_degradation_map(importance, max_rounds)
    _check_rounds(degradation_map)
    return _one_image(frame, degradation_map, device, degrade_gaussian_fx_device, block_size), degradation_map


def _one_block(block: np.ndarray, value: int, device, fn) -> np.ndarray:
    if not isinstance(block, np.ndarray) or block.dtype != np.uint8 or block.ndim != 3 or block.shape[0] != block.shape[1]:
        raise ValueError("degrade: a block is a square uint8 (b,b,C) array")
    return _one_image(block, np.full((1, 1), int(value), np.int32), device, fn, block.shape[0])


def downscale_block(block: np.ndarray, scale: int, device="cuda:0") -> np.ndarray:
    """presley.py:978-983 for one (b,b,C) block, on the device: INTER_AREA to max(1, b // scale), INTER_LINEAR back.
    A scale below 1 raises ValueError (the reference divides by zero).  PARITY UNPINNED vs cv2 (module docstring)."""
    if int(scale) < 1:
        raise ValueError("downscale_block: scale must be >= 1")
    return _one_block(block, scale, device, degrade_scale_device)


def blur_block(block: np.ndarray, rounds: int, device="cuda:0") -> np.ndarray:
    """presley.py:986-990 for one (b,b,C) block, on the device: `rounds` passes of GaussianBlur(5x5, sigma 1) in cv2's
    CV_8U fixed point; with rounds <= 0 the block itself is returned, as in the reference.  More than 64 rounds
    raise ValueError.  PARITY UNPINNED vs cv2 (module docstring)."""
    if int(rounds) <= 0:
        return block
    _check_rounds(np.asarray(rounds))
    return _one_block(block, rounds, device, degrade_gaussian_fx_device)


def _kernel_of(method: Callable):
    """`method` selects the kernel; there is no CPU fallback that could run a foreign callable per block."""
    if method is downscale_block:
        return degrade_scale_device
    if method is blur_block:
        return degrade_gaussian_fx_device
    raise ValueError("degrade: method must be elvis_amd's downscale_block or blur_block")


def degrade_frame(frame: np.ndarray, degradation_map: np.ndarray, block_size: int, method: Callable,
                  device="cuda:0") -> np.ndarray:
    """presley.py:993-1013 on the device: every block whose map value is > 0 becomes method(block, value), with
    `method` one of this module's `downscale_block` / `blur_block` (any other callable raises ValueError); rows and
    columns past the last whole block are returned unchanged.  A map that is not the block grid raises ValueError.
    PARITY UNPINNED vs cv2 (module docstring)."""
    fn = _kernel_of(method)
    _check_frame(frame, degradation_map, block_size, "degradation_map")
    levels = np.asarray(degradation_map).astype(np.int32)
    if fn is degrade_gaussian_fx_device:
        _check_rounds(levels)
    return _one_image(frame, levels, device, fn, block_size)


def degrade_video_adaptive(frames: Sequence[np.ndarray], importance_scores: Sequence[np.ndarray], block_size: int,
                           max_value: int, method: Callable, device="cuda:0") -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """presley.py:1016-1039 on the device: per frame, map = generate_degradation_map(importance, max_value) and
    degrade_frame(frame, map, block_size, method); the clip is uploaded once and degraded by one launch.  Frames
    and importances are paired as zip pairs them.  Returns (degraded frames, int32 maps).  Same `method` rule,
    departures and PARITY UNPINNED status as `degrade_frame`."""
    fn = _kernel_of(method)
    count = min(len(frames), len(importance_scores))
    if count == 0:
        return [], []
    frames = list(frames[:count])
    for frame, importance in zip(frames, importance_scores):
        _check_frame(frame, importance, block_size, "importance")
    maps = [generate_degradation_map(importance, max_value) for importance in importance_scores[:count]]
    levels = np.stack(maps).astype(np.int32)
    if fn is degrade_gaussian_fx_device:
        _check_rounds(levels)
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        out = fn(frames_to_device(frames, dev), torch.from_numpy(np.ascontiguousarray(levels)).to(dev), block_size)
        return frames_to_host(out), maps
