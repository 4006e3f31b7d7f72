"""Classical per-block restorers on the device: the OpenCV baselines ELVIS and Presley compare every neural slot to.

`restore_downsample_opencv_lanczos` / `restore_blur_opencv_unsharp_mask` keep the names, arguments and return
values of elvis.py:2773-2866 (one BGR or RGB uint8 HWC image + per-block map); `restore_with_opencv_lanczos` /
`restore_with_opencv_unsharp` keep those of utils.py:1253-1392 (a list of frames, `halo`, `temporal_blend`) and
plug in as a `restore_fn`.  The `*_device` forms work on resident `[n,H,W,C]` uint8 tensors and `[n,By,Bx]` int32
maps, a whole clip per launch.  Every tap table is built here on the host and read by the kernels
(csrc/classical.hip), so the device work is pure integer arithmetic.

PARITY UNPINNED vs cv2: OpenCV is absent from the build and GPU environments, so its 8-bit rules are restated
(INTER_AREA at an integer scale, the 11-bit INTER_LANCZOS4 taps with 22-bit rounding, the bit-exact 8.8 / 16.16
fixed-point GaussianBlur, addWeighted in float32); the device output is bit-exact with the numpy restatement in
tests/_classical_ref.py, not checked against cv2 itself.
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib, ptr
from .ops import _block_maps, _block_out, _check_image_grid, _chk_u8, _one_image, _s
from .recompose import frames_to_device, frames_to_host
from .tiler import _nearest_rows

MAX_LEVEL = 16            # ELVIS_CLASSICAL_MAX_LEVEL: sigma of the unsharp mask; log2 of the Lanczos factor
MAX_HALO = 32
MAX_BLOCK = 32
LANCZOS_PHASES = 32       # destination indices per factor in the device table (= the largest block)
LANCZOS_FACTORS = (2, 4, 8, 16, 32)
_TABLES: Dict[str, tuple] = {}


# ----------------------------------------------------------------------------- tap tables (host)
def lanczos4_coeffs(x) -> np.ndarray:
    """cv::interpolateLanczos4(x): 8 float32 coefficients of source offsets -3..4 for the fraction x."""
    x = np.float32(x)
    if x < np.finfo(np.float32).eps:
        return np.array([0, 0, 0, 1, 0, 0, 0, 0], np.float32)
    s45 = 0.70710678118654752440084436210485
    cs = ((1, 0), (-s45, -s45), (0, 1), (s45, -s45), (-1, 0), (s45, s45), (0, -1), (-s45, s45))
    y0 = float(-(x + np.float32(3))) * math.pi * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    coeffs = np.zeros(8, np.float32)
    total = np.float32(0)
    for i in range(8):
        y = float(-(x + np.float32(3) - np.float32(i))) * math.pi * 0.25
        coeffs[i] = np.float32((cs[i][0] * s0 + cs[i][1] * c0) / (y * y))
        total = np.float32(total + coeffs[i])
    return (coeffs * (np.float32(1) / total)).astype(np.float32)


def lanczos_taps(factor: int, n_dst: int) -> Tuple[np.ndarray, np.ndarray]:
    """The 8-bit INTER_LANCZOS4 upscale by `factor` (cv::resize fixed-point path): for every destination index d,
    the first source index sx - 3 (before BORDER_REPLICATE clamping) and the int16 taps rint(coef * 2048)."""
    inv = 1.0 / float(factor)
    first = np.zeros(n_dst, np.int64)
    taps = np.zeros((n_dst, 8), np.int16)
    for d in range(n_dst):
        fx = np.float32((d + 0.5) * inv - 0.5)
        sx = int(np.floor(fx))
        fx = np.float32(fx - np.float32(sx))
        first[d] = sx - 3
        taps[d] = np.rint(lanczos4_coeffs(fx) * np.float32(2048)).astype(np.int16)
    return first, taps


def lanczos_tap_table() -> np.ndarray:
    """int16 [5][32][8]: the taps of destination index d for the factor 2**(i+1) (the device table)."""
    return np.stack([lanczos_taps(f, LANCZOS_PHASES)[1] for f in LANCZOS_FACTORS])


def gaussian_taps_u8(sigma: float, ksize: int = 0) -> np.ndarray:
    """cv::GaussianBlur's CV_8U taps for `sigma` and an odd `ksize` (0: cvRound(6 sigma + 1) | 1, which is 6L + 1 for
    the unsharp mask's sigma = L): getGaussianKernelBitExact, then error diffusion to 8 fractional bits; int16,
    symmetric, sum 256.  (5, sigma 1), the kernel of both degraders, gives 14 62 104 62 14."""
    n = int(ksize) if ksize else int(np.rint(6 * float(sigma) + 1)) | 1
    if n < 1 or n % 2 == 0 or not sigma > 0:
        raise ValueError("gaussian_taps_u8: ksize must be odd and sigma positive")
    scale2 = -0.125 / (float(sigma) * float(sigma))
    vals = [math.exp(float((2 * i + 1 - n) ** 2) * scale2) for i in range(n // 2)]
    mul = 1.0 / (sum(vals) * 2.0 + 1.0)
    taps = np.zeros(n, np.int16)
    err = 0.0
    for i in range(n // 2):
        adj = vals[i] * mul * 256.0 + err
        v = int(np.rint(adj))
        err = adj - v
        taps[i] = taps[n - 1 - i] = v
    taps[n // 2] = 256 - 2 * int(taps[: n // 2].sum())
    return taps


def gaussian_tap_table(max_level: int = MAX_LEVEL) -> Tuple[np.ndarray, np.ndarray]:
    """(taps int16, offsets int32[max_level + 1]): level L's 6L + 1 taps start at taps[offsets[L]]."""
    parts = [gaussian_taps_u8(lv) for lv in range(1, max_level + 1)]
    offsets = np.zeros(max_level + 1, np.int32)
    offsets[1:] = np.cumsum([0] + [len(p) for p in parts[:-1]])
    return np.concatenate(parts), offsets


def _tables(device) -> tuple:
    key = str(device)
    if key not in _TABLES:
        g_taps, g_offs = gaussian_tap_table()
        _TABLES[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device)
                             for a in (lanczos_tap_table(), g_taps, g_offs))
    return _TABLES[key]


# ----------------------------------------------------------------------------- device-resident forms
_WHO = "classical restorers"


def lanczos_restore_device(frames_d: torch.Tensor, levels_d: torch.Tensor, block_size: int, out=None) -> torch.Tensor:
    """Per block of level L > 0: INTER_AREA downscale to max(1, block_size >> L), INTER_LANCZOS4 back to
    block_size (levels clamped to [0, 16] on the device).  frames [n,H,W,C] u8, levels [n,H//b,W//b] int32."""
    _chk_u8(frames_d)
    n, h, w, c = frames_d.shape
    m = _block_maps(levels_d, n, _WHO)
    taps, _, _ = _tables(frames_d.device)
    out = _block_out(frames_d, block_size, out, _WHO)
    check(lib().elvis_classical_lanczos_u8(ptr(frames_d), ptr(m), ptr(out), n, h, w, c, block_size, m.shape[1], m.shape[2],
                                           ptr(taps), _s(frames_d)), frames_d.device)
    return out


def unsharp_restore_device(frames_d: torch.Tensor, levels_d: torch.Tensor, block_size: int, halo: int = 0,
                           out=None) -> torch.Tensor:
    """Per block of level L > 0: unsharp mask with sigma L, amount L/2 on the block grown by `halo` pixels and
    clipped at the frame (levels clamped to [0, 16] on the device).  frames [n,H,W,C] u8, levels [n,H//b,W//b]."""
    _chk_u8(frames_d)
    n, h, w, c = frames_d.shape
    m = _block_maps(levels_d, n, _WHO)
    _, g_taps, g_offs = _tables(frames_d.device)
    out = _block_out(frames_d, block_size, out, _WHO)
    check(lib().elvis_classical_unsharp_u8(ptr(frames_d), ptr(m), ptr(out), n, h, w, c, block_size, m.shape[1], m.shape[2],
                                           int(halo), ptr(g_taps), ptr(g_offs), MAX_LEVEL, _s(frames_d)), frames_d.device)
    return out


def temporal_blend_device(frames_d: torch.Tensor, temporal_blend: float, out=None) -> torch.Tensor:
    """out[0] = frames[0]; out[f] = uint8(tb * out[f-1] + (1 - tb) * frames[f]) in float64 (utils.py:1308-1312).
    `out` may be `frames_d` itself."""
    _chk_u8(frames_d)
    tb = float(temporal_blend)
    out = torch.empty_like(frames_d) if out is None else out
    _chk_u8(out)
    if out.shape != frames_d.shape:
        raise ValueError("out must have the frames' shape")
    n = frames_d.shape[0]
    if n == 0 or frames_d.numel() == 0:
        raise ValueError("temporal_blend_device: empty clip")
    check(lib().elvis_temporal_blend_u8(ptr(frames_d), ptr(out), n, frames_d.numel() // n, tb, 1 - tb, _s(frames_d)),
          frames_d.device)
    return out


# ----------------------------------------------------------------------------- the reference's call surface
def _check_image(image: np.ndarray, maps: np.ndarray, block_size: int):
    _check_image_grid(image, maps, block_size, "the classical restorers", "map {} does")


def _check_level_range(levels: np.ndarray):
    if levels.size and levels.max() > MAX_LEVEL:
        raise ValueError(f"levels above {MAX_LEVEL} are not supported")


def restore_downsample_opencv_lanczos(downsampled_image: np.ndarray, downscale_maps: np.ndarray, block_size: int,
                                      device="cuda:0") -> np.ndarray:
    """elvis.py:2773-2820 on the device: factors = 2**maps (int32); every block with factor > 1 is INTER_AREA-
    downscaled to max(1, block_size // factor) and INTER_LANCZOS4-resized back, the others are copied.  When the
    largest factor is 1 the input itself is returned, as in the reference.

    Departures: a factor that is not a power of two, or a level above 16, raises ValueError (the reference would
    resize to a non-integer scale or overflow int32), and so does a map that does not match the block grid (the
    reference leaves uncovered blocks black).  PARITY UNPINNED vs cv2 (module docstring)."""
    maps = np.asarray(downscale_maps)
    _check_level_range(maps)
    factors = np.power(2, maps).astype(np.int32)
    if int(factors.max()) == 1:
        return downsampled_image
    _check_image(downsampled_image, maps, block_size)
    scaled = factors > 1
    if (factors[scaled] & (factors[scaled] - 1)).any():
        raise ValueError("restore_downsample_opencv_lanczos: downscale factors must be powers of two")
    levels = np.zeros(factors.shape, np.int32)
    levels[scaled] = np.log2(factors[scaled]).astype(np.int32)
    return _one_image(downsampled_image, levels, device, lanczos_restore_device, block_size)


def restore_blur_opencv_unsharp_mask(blurred_image: np.ndarray, blur_maps: np.ndarray, block_size: int,
                                     device="cuda:0") -> np.ndarray:
    """elvis.py:2822-2866 on the device: level = int(map) per block (truncated, elvis.py:2849); a block of level
    L > 0 becomes addWeighted(block, 1 + L/2, GaussianBlur(block, sigma L), -L/2, 0), the others are copied.

    Departures: a level above 16, or a map that does not match the block grid, raises ValueError.  PARITY
    UNPINNED vs cv2 (module docstring)."""
    maps = np.asarray(blur_maps)
    _check_image(blurred_image, maps, block_size)
    levels = maps.astype(np.int64)
    _check_level_range(levels)
    return _one_image(blurred_image, np.maximum(levels, 0), device, unsharp_restore_device, block_size, 0)


def _clip_levels(frames: List[np.ndarray], degradation_maps, block_size: int) -> np.ndarray:
    """utils.py:1272-1279 per frame: the frame's map, zeros when it has none, INTER_NEAREST-resized to the block
    grid (then truncated to int32) when its shape differs."""
    h, w = frames[0].shape[:2]
    by, bx = h // block_size, w // block_size
    levels = np.zeros((len(frames), by, bx), np.int32)
    for i in range(len(frames)):
        if len(degradation_maps) <= i:
            continue
        m = np.asarray(degradation_maps[i])
        if m.shape != (by, bx):
            m = m.astype(np.float32)[_nearest_rows(m.shape[0], by)][:, _nearest_rows(m.shape[1], bx)].astype(np.int32)
        elif not np.array_equal(m, np.trunc(m)):
            raise ValueError("restore_with_opencv_*: map values must be whole numbers (sigma = level, amount = level / 2)")
        _check_level_range(m)
        levels[i] = np.maximum(m, 0)
    return levels


def _restore_clip(frames: List[np.ndarray], degradation_maps, block_size: int, halo: int, temporal_blend: float,
                  device) -> List[np.ndarray]:
    if not frames:
        return []
    if not 0 <= int(halo) <= MAX_HALO:
        raise ValueError(f"halo must be in [0, {MAX_HALO}]")
    if temporal_blend > 1:
        raise ValueError("temporal_blend must be <= 1")
    if not 2 <= block_size <= MAX_BLOCK or block_size & (block_size - 1):
        raise ValueError(f"block_size must be a power of two in [2, {MAX_BLOCK}]")
    levels = _clip_levels(frames, degradation_maps, block_size)
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        fd = frames_to_device(frames, dev)
        if levels.shape[1] and levels.shape[2]:
            out = unsharp_restore_device(fd, torch.from_numpy(levels).to(dev), block_size, int(halo))
        else:
            out = fd.clone()                 # no whole block: every pixel is copied
        if temporal_blend > 0 and len(frames) > 1:
            temporal_blend_device(out, temporal_blend, out=out)
        return frames_to_host(out)


def restore_with_opencv_unsharp(frames: List[np.ndarray], degradation_maps, block_size: int, halo: int = 0,
                                temporal_blend: float = 0.0, device="cuda", **kwargs) -> List[np.ndarray]:
    """utils.py:1315-1392 on the device, the whole clip per launch: every block of level L > 0 (the frame's map,
    zeros when the frame has none, NEAREST-resized to the grid when its shape differs) is unsharp-masked with
    sigma L and amount L/2 on its tile (the block grown by `halo` pixels, clipped at the frame); rows and columns
    past the last whole block are copied; with 0 < temporal_blend, out[f] = uint8(tb out[f-1] + (1-tb) out[f]).
    Usable as a `restore_fn` (extra keyword arguments are ignored).

    Departures: map values that are not whole numbers, levels above 16, halo outside [0, 32], temporal_blend
    above 1 and block sizes other than 2..32 (powers of two) raise ValueError.  PARITY UNPINNED vs cv2 (module
    docstring)."""
    return _restore_clip(frames, degradation_maps, block_size, halo, temporal_blend, device)


def restore_with_opencv_lanczos(frames: List[np.ndarray], degradation_maps, block_size: int, halo: int = 0,
                                temporal_blend: float = 0.0, device="cuda", **kwargs) -> List[np.ndarray]:
    """utils.py:1253-1312 on the device.  Despite its name the reference's function is the same per-block unsharp
    mask as `restore_with_opencv_unsharp` (sigma = level, amount = level / 2), and so is this one; same
    arguments, departures and PARITY UNPINNED status."""
    return _restore_clip(frames, degradation_maps, block_size, halo, temporal_blend, device)
