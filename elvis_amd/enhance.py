"""`RealESRGANer.enhance` as the reference runs it (elvis.py:2482-2519, utils.py:1428-1470, presley.py:1279-1314): the
network of `get_realesrgan_upsampler` inside the `realesrgan` package's `pre_process` / `tile_process` / `post_process`,
then `cv2.resize(..., interpolation=cv2.INTER_LANCZOS4)` to `outscale`.  Kernels: csrc/sr_enhance.hip.

    pre_process   F.pad(img, (0, pre_pad, 0, pre_pad), 'reflect'); for an x2 network a second reflect pad to an even
                  size, of the already padded image                     -> `reflect_index_maps`, read by the tile gather
    tile_process  ceil(W / tile) x ceil(H / tile) tiles, each run with `tile_pad` pixels of context clipped at the
                  padded image, the context cropped off the output      -> `plan_tiles`, gather / forward / paste
    post_process  crop the mod pad and the pre_pad off the output       -> the paste clips at s*H x s*W
    enhance       resize the output to (int(W * outscale), int(H * outscale)) unless outscale == scale
                                                                        -> `resize_lanczos4_device`

The tiles of one padded shape go through `model.forward` together, `model.max_batch(th, tw)` at a time, where the
reference runs them one by one; every kernel of the networks is per-sample, so the grouping changes nothing.

PARITY UNPINNED vs cv2 and vs the `realesrgan` package (neither is available to the tests).  Pinned: the resize is
bit-exact with the numpy statement of cv2's 8-bit fixed-point rule (tests/_enhance_ref.py; the rule classical.py
already states for its per-block upscale), the padding equals `torch.nn.functional.pad(..., 'reflect')`, and a tiled
run equals the composition of `model.forward` on each padded crop.
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .classical import lanczos4_coeffs
from .recompose import frames_to_device, frames_to_host

LDS_LIMIT = 64 * 1024                   # bytes of LDS per workgroup of the resize: two workgroups per CU stay resident
RESIZE_TILES = ((16, 64), (16, 32), (8, 32), (8, 16), (4, 16))   # destination tiles, largest first
INT32_LIMIT = 1 << 31

Tile = namedtuple("Tile", "y0 x0 h w crop_y crop_x out_y out_x out_h out_w")
_DEVICE_TABLES: Dict[tuple, tuple] = {}


# ----------------------------------------------------------------------------- tables (host)
@functools.lru_cache(maxsize=256)
def lanczos4_resize_taps(n_src: int, n_dst: int) -> Tuple[np.ndarray, np.ndarray]:
    """cv2's 8-bit INTER_LANCZOS4 tables of one axis resized from `n_src` to `n_dst`: for every destination index d the
    first source index sx - 3 (int32, before the BORDER_REPLICATE clamp to [0, n_src - 1]) and the eight int16 taps
    rint(coef * 2048), with fx = float32((d + 0.5) * (double(n_src) / n_dst) - 0.5), sx = floor(fx), coef =
    lanczos4_coeffs(fx - sx).  Cached per (n_src, n_dst); the arrays are read-only."""
    n_src, n_dst = int(n_src), int(n_dst)
    if n_src < 1 or n_dst < 1:
        raise ValueError(f"lanczos4_resize_taps: sizes must be positive, got {n_src} -> {n_dst}")
    scale = float(n_src) / float(n_dst)
    first = np.zeros(n_dst, np.int32)
    taps = np.zeros((n_dst, 8), np.int16)
    phases: Dict[float, np.ndarray] = {}
    for d in range(n_dst):
        fx = np.float32((d + 0.5) * scale - 0.5)
        sx = int(np.floor(fx))
        fr = np.float32(fx - np.float32(sx))
        first[d] = sx - 3
        key = float(fr)
        if key not in phases:
            phases[key] = np.rint(lanczos4_coeffs(fr) * np.float32(2048)).astype(np.int16)
        taps[d] = phases[key]
    first.setflags(write=False)
    taps.setflags(write=False)
    return first, taps


def lanczos4_sum_bound(xtaps: np.ndarray, ytaps: np.ndarray) -> int:
    """The largest magnitude a partial sum of the two-pass resize can reach on 8-bit pixels, rounding constant included:
    255 * max(Px * Py + Nx * Ny) + 2^21 over the phases of the two tables (P, N: the sums of a phase's positive and of
    its negative taps).  The kernel accumulates in int32, so this must stay below 2^31."""
    def pn(t):
        t = np.unique(np.asarray(t, np.int64).reshape(-1, 8), axis=0)
        return np.maximum(t, 0).sum(1), np.maximum(-t, 0).sum(1)
    px, nx = pn(xtaps)
    py, ny = pn(ytaps)
    worst = int((px[:, None] * py[None, :] + nx[:, None] * ny[None, :]).max())
    return 255 * worst + (1 << 21)


@functools.lru_cache(maxsize=256)
def _checked_tables(hs: int, ws: int, hd: int, wd: int):
    xf, xt = lanczos4_resize_taps(ws, wd)
    yf, yt = lanczos4_resize_taps(hs, hd)
    bound = lanczos4_sum_bound(xt, yt)
    if bound >= INT32_LIMIT:
        raise ValueError(f"resize_lanczos4: the taps of {hs}x{ws} -> {hd}x{wd} allow a sum of {bound}, "
                         f"the int32 limit is {INT32_LIMIT - 1}")
    return xf, xt, yf, yt


@functools.lru_cache(maxsize=256)
def resize_tile_plan(hs: int, ws: int, hd: int, wd: int, c: int) -> Tuple[int, int, int]:
    """(th, tw, LDS bytes) of the resize's workgroup: the largest destination tile of `RESIZE_TILES` whose source
    footprint and int32 intermediate fit `LDS_LIMIT`, by the library's own count for the tables of this resize.  A
    ratio so steep that the smallest tile does not fit is a ValueError."""
    xf, _, yf, _ = _checked_tables(hs, ws, hd, wd)
    need = 0
    for th, tw in RESIZE_TILES:
        need = L.lib().elvis_resize_lanczos4_lds_bytes(xf.ctypes.data, yf.ctypes.data, hs, ws, hd, wd, c, th, tw)
        L.check(min(need, 0))
        if need <= LDS_LIMIT:
            return th, tw, need
    th, tw = RESIZE_TILES[-1]
    raise ValueError(f"resize_lanczos4: {hs}x{ws} -> {hd}x{wd} with {c} channel(s) is too steep: the smallest destination "
                     f"tile {th}x{tw} needs {need} bytes of LDS, the limit is {LDS_LIMIT} bytes per workgroup")


def _device_tables(hs: int, ws: int, hd: int, wd: int, device) -> tuple:
    key = (hs, ws, hd, wd, str(device))
    hit = _DEVICE_TABLES.get(key)
    if hit is None:
        if len(_DEVICE_TABLES) > 64:
            _DEVICE_TABLES.clear()
        hit = _DEVICE_TABLES[key] = tuple(torch.from_numpy(np.array(a)).to(device) for a in _checked_tables(hs, ws, hd, wd))
    return hit


def _chk_frames(frames_d: torch.Tensor, who: str, channels: Sequence[int]) -> None:
    if (not isinstance(frames_d, torch.Tensor) or frames_d.dtype != torch.uint8 or frames_d.dim() != 4 or not frames_d.is_cuda
            or not frames_d.is_contiguous() or frames_d.shape[3] not in channels or 0 in frames_d.shape):
        raise ValueError(f"{who} takes a contiguous uint8 [n,H,W,C] tensor on the device, C in {tuple(channels)}")


def resize_lanczos4_device(frames_d: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
    """cv2.resize(frame, (out_w, out_h), interpolation=cv2.INTER_LANCZOS4) of every frame of a resident uint8
    [n,H,W,C] clip, C in 1..4, any ratio, in one launch (`elvis_resize_lanczos4_u8`).  Equal sizes give a copy, as cv2
    does.  ValueError: a ratio too steep for the kernel's LDS tile (`resize_tile_plan`), or taps whose sums could
    overflow int32 (`lanczos4_sum_bound`)."""
    _chk_frames(frames_d, "resize_lanczos4_device", (1, 2, 3, 4))
    n, hs, ws, c = frames_d.shape
    hd, wd = int(out_h), int(out_w)
    if hd < 1 or wd < 1:
        raise ValueError(f"resize_lanczos4_device: the output size must be positive, got {hd}x{wd}")
    if (hd, wd) == (hs, ws):
        return frames_d.clone()
    xf, _, yf, _ = _checked_tables(hs, ws, hd, wd)
    th, tw, _ = resize_tile_plan(hs, ws, hd, wd, c)
    with torch.cuda.device(frames_d.device):
        xf_d, xt_d, yf_d, yt_d = _device_tables(hs, ws, hd, wd, frames_d.device)
        out = torch.empty((n, hd, wd, c), dtype=torch.uint8, device=frames_d.device)
        L.check(L.lib().elvis_resize_lanczos4_u8(L.ptr(frames_d), L.ptr(out), n, hs, ws, hd, wd, c, xf.ctypes.data, yf.ctypes.data,
                                                 L.ptr(xf_d), L.ptr(xt_d), L.ptr(yf_d), L.ptr(yt_d), th, tw,
                                                 L.stream_handle(frames_d.device)), frames_d.device)
    return out


def _reflect_right(idx: np.ndarray, pad: int, what: str) -> np.ndarray:
    if pad >= len(idx):       # torch: "Padding size should be less than the corresponding input dimension"
        raise ValueError(f"{what}: a reflect pad of {pad} needs more than {pad} pixels, got {len(idx)}")
    return np.concatenate([idx, idx[len(idx) - 2 - np.arange(pad)]]) if pad else idx


def reflect_index_maps(H: int, W: int, pre_pad: int, mod: int) -> Tuple[np.ndarray, np.ndarray]:
    """(rows int32 [Hp], cols int32 [Wp]): the source row / column of every row / column of the image `pre_process`
    hands to the network - F.pad(img, (0, pre_pad, 0, pre_pad), 'reflect'), then, when a side of the padded image is no
    multiple of `mod` (2 for an x2 network, else 1), F.pad(..., (0, mod_pad_w, 0, mod_pad_h), 'reflect') of the padded
    image.  Reflection leaves the edge pixel out.  `pre_pad >= min(H, W)` is a ValueError, torch's own limit."""
    H, W, pre_pad, mod = int(H), int(W), int(pre_pad), int(mod)
    if H < 1 or W < 1 or pre_pad < 0 or mod < 1:
        raise ValueError(f"reflect_index_maps: bad arguments H={H} W={W} pre_pad={pre_pad} mod={mod}")
    if pre_pad >= min(H, W):
        raise ValueError(f"pre_pad={pre_pad} must be less than the frame's sides {H}x{W} (reflect padding)")
    out = []
    for size in (H, W):
        idx = _reflect_right(np.arange(size, dtype=np.int32), pre_pad, "pre_pad")
        idx = _reflect_right(idx, (-len(idx)) % mod, "mod pad")
        out.append(np.ascontiguousarray(idx, np.int32))
    return out[0], out[1]


def plan_tiles(H: int, W: int, tile: int, tile_pad: int, scale: int = 1) -> List[Tile]:
    """`RealESRGANer.tile_process`'s loops over an H x W (padded) image: ceil(W / tile) x ceil(H / tile) tiles, row by row.
    Per tile: `y0, x0, h, w` - the padded input box, `tile_pad` of context on each side clipped at the image;
    `crop_y, crop_x` - where the tile's own pixels start inside the network's output, (start - start_pad) * scale;
    `out_y, out_x, out_h, out_w` - where they go in the output, start * scale and tile_len * scale.  `tile=0` is one
    tile, the whole image."""
    H, W, tile, tile_pad, s = int(H), int(W), int(tile), int(tile_pad), int(scale)
    if H < 1 or W < 1 or tile < 0 or tile_pad < 0 or s < 1:
        raise ValueError(f"plan_tiles: bad arguments H={H} W={W} tile={tile} tile_pad={tile_pad} scale={s}")
    if tile == 0:
        return [Tile(0, 0, H, W, 0, 0, 0, 0, H * s, W * s)]
    tiles = []
    for y in range(math.ceil(H / tile)):
        for x in range(math.ceil(W / tile)):
            sx, sy = x * tile, y * tile
            ex, ey = min(sx + tile, W), min(sy + tile, H)
            sxp, exp_ = max(sx - tile_pad, 0), min(ex + tile_pad, W)
            syp, eyp = max(sy - tile_pad, 0), min(ey + tile_pad, H)
            tiles.append(Tile(syp, sxp, eyp - syp, exp_ - sxp, (sy - syp) * s, (sx - sxp) * s, sy * s, sx * s,
                              (ey - sy) * s, (ex - sx) * s))
    return tiles


# ----------------------------------------------------------------------------- tiles on the device
def gather_tiles_device(frames_d: torch.Tensor, desc: np.ndarray, th: int, tw: int, rows: np.ndarray, cols: np.ndarray,
                        rows_d: torch.Tensor, cols_d: torch.Tensor) -> torch.Tensor:
    """[T,th,tw,3]: tile t is rows `rows[y0 : y0 + th]`, columns `cols[x0 : x0 + tw]` of frame `f`, desc[t] = (f, y0, x0)."""
    _chk_frames(frames_d, "gather_tiles_device", (3,))
    n, H, W, _ = frames_d.shape
    desc = np.ascontiguousarray(desc, np.int32).reshape(-1, 3)
    rows, cols = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(cols, np.int32)
    T = desc.shape[0]
    dev = frames_d.device
    with torch.cuda.device(dev):
        out = torch.empty((T, int(th), int(tw), 3), dtype=torch.uint8, device=dev)
        desc_d = torch.from_numpy(desc).to(dev)
        L.check(L.lib().elvis_sr_gather_tiles_u8(L.ptr(frames_d), L.ptr(out), n, H, W, T, int(th), int(tw), desc.ctypes.data,
                                                 L.ptr(desc_d), rows.ctypes.data, L.ptr(rows_d), len(rows), cols.ctypes.data,
                                                 L.ptr(cols_d), len(cols), L.stream_handle(dev)), dev)
    return out


def paste_tiles_device(tiles_d: torch.Tensor, desc: np.ndarray, out_d: torch.Tensor) -> torch.Tensor:
    """Write the crop desc[t] = (frame, crop y, crop x, destination y, x, crop height, width) of every tile of
    `tiles_d` [T,tth,ttw,3] into `out_d` [n,OH,OW,3]; what lies beyond OH x OW is dropped."""
    _chk_frames(tiles_d, "paste_tiles_device", (3,))
    _chk_frames(out_d, "paste_tiles_device", (3,))
    desc = np.ascontiguousarray(desc, np.int32).reshape(-1, 7)
    T, tth, ttw, _ = tiles_d.shape
    if desc.shape[0] != T or out_d.device != tiles_d.device:
        raise ValueError(f"paste_tiles_device: {desc.shape[0]} descriptors for {T} tiles, or tensors on two devices")
    n, OH, OW, _ = out_d.shape
    dev = out_d.device
    with torch.cuda.device(dev):
        desc_d = torch.from_numpy(desc).to(dev)
        L.check(L.lib().elvis_sr_paste_tiles_u8(L.ptr(tiles_d), L.ptr(out_d), T, tth, ttw, n, OH, OW, desc.ctypes.data,
                                                L.ptr(desc_d), L.stream_handle(dev)), dev)
    return out_d


class RealESRGANer:
    """The object the reference calls (`realesrgan.RealESRGANer`, built at elvis.py:2482-2490) around an `SRModel` of
    `get_realesrgan_upsampler`: `tile`, `tile_pad` and `pre_pad` as the package applies them, `enhance` host to host and
    `enhance_device` on a resident clip.  `.scale` is the network's.  An odd `tile` with an x2 model is a ValueError: the
    package's x2 network cannot take an odd tile (its pixel-unshuffle by 2).  DEPARTURE: an odd `tile_pad` with an x2
    model also gives odd tile boxes (`tile=8, tile_pad=3`: 11 wide at the frame's edge), on which the package fails in
    the same pixel-unshuffle; here they run, through the model's own reflect pad of an odd side to even
    (`realesrgan.RRDBNetModel._forward_batch`), which the package does not have.  An even `tile_pad` - the reference's
    default 10 - gives even boxes inside the even padded image and is the package's computation."""

    def __init__(self, model, *, tile: int = 0, tile_pad: int = 10, pre_pad: int = 0):
        self.model = model
        self.scale = int(model.scale)
        self.device = model.device
        self.tile, self.tile_pad, self.pre_pad = int(tile), int(tile_pad), int(pre_pad)
        if self.tile < 0 or self.tile_pad < 0 or self.pre_pad < 0:
            raise ValueError(f"RealESRGANer: tile={tile}, tile_pad={tile_pad} and pre_pad={pre_pad} must not be negative")
        if self.scale == 2 and self.tile % 2:
            raise ValueError(f"RealESRGANer: tile={tile} is odd; an x2 model needs an even tile")
        self._maps: Dict[tuple, tuple] = {}

    def _index_maps(self, H: int, W: int):
        key = (H, W)
        hit = self._maps.get(key)
        if hit is None:
            if len(self._maps) > 16:
                self._maps.clear()
            rows, cols = reflect_index_maps(H, W, self.pre_pad, 2 if self.scale == 2 else 1)
            hit = self._maps[key] = (rows, cols, torch.from_numpy(rows).to(self.device), torch.from_numpy(cols).to(self.device))
        return hit

    def _forward(self, lr: torch.Tensor, swap_rb: bool) -> torch.Tensor:
        try:
            return self.model.forward(lr, swap_rb=swap_rb)
        except RuntimeError as exc:       # elvis.py:2517-2519
            raise RuntimeError(f"Real-ESRGAN failed on {self.device}: {exc}") from exc

    def network_device(self, frames_d: torch.Tensor, swap_rb: bool = True) -> torch.Tensor:
        """pre_process, tile_process (or `process` for tile=0) and post_process: [n,H,W,3] -> [n,s*H,s*W,3]."""
        _chk_frames(frames_d, "RealESRGANer", (3,))
        if frames_d.device != self.device:
            raise ValueError(f"RealESRGANer: frames on {frames_d.device}, model on {self.device}")
        n, H, W, _ = frames_d.shape
        s = self.scale
        with torch.cuda.device(self.device):
            rows, cols, rows_d, cols_d = self._index_maps(H, W)
            Hp, Wp = len(rows), len(cols)
            if self.tile == 0 and (Hp, Wp) == (H, W):
                return self._forward(frames_d, swap_rb)
            classes: Dict[tuple, list] = {}
            for t in plan_tiles(Hp, Wp, self.tile, self.tile_pad, s):
                if t.out_y < s * H and t.out_x < s * W:        # a tile that lies in the padding leaves nothing
                    classes.setdefault((t.h, t.w), []).append(t)
            out = torch.empty((n, s * H, s * W, 3), dtype=torch.uint8, device=self.device)
            for (th, tw), tiles in classes.items():
                todo = [(f, t) for f in range(n) for t in tiles]
                step = self.model.max_batch(th, tw)
                for i in range(0, len(todo), step):
                    part = todo[i:i + step]
                    lr = gather_tiles_device(frames_d, np.array([(f, t.y0, t.x0) for f, t in part], np.int32), th, tw,
                                             rows, cols, rows_d, cols_d)
                    sr = self._forward(lr, swap_rb)
                    paste_tiles_device(sr, np.array([(f, t.crop_y, t.crop_x, t.out_y, t.out_x, t.out_h, t.out_w)
                                                     for f, t in part], np.int32), out)
            return out

    def enhance_device(self, frames_d: torch.Tensor, outscale: Optional[float] = None, swap_rb: bool = True) -> torch.Tensor:
        """`enhance` on a resident clip: [n,H,W,3] u8 BGR on the device -> the network's output, resized with Lanczos4
        to (int(H * outscale), int(W * outscale)) when `outscale` is given and is not the network's scale.  `swap_rb=False`
        takes and gives RGB (the network sees the same image either way)."""
        out = self.network_device(frames_d, swap_rb)
        if outscale is not None and float(outscale) != float(self.scale):
            H, W = frames_d.shape[1:3]
            out = resize_lanczos4_device(out, int(H * outscale), int(W * outscale))
        return out

    def enhance(self, img: np.ndarray, outscale: Optional[float] = None):
        """`RealESRGANer.enhance(img, outscale)` for what the reference passes (elvis.py:2515, presley.py:1308): one BGR
        uint8 HWC image in host memory -> (the BGR output, "RGB"), the package's `img_mode` of a three-channel image.
        2-D gray, RGBA and 16-bit images, which the package handles and the reference never passes, are a ValueError."""
        img = np.asarray(img)
        if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
            raise ValueError(f"RealESRGANer.enhance takes one uint8 (H, W, 3) image; gray, RGBA and 16-bit inputs are "
                             f"not built, got {img.shape} {img.dtype}")
        with torch.cuda.device(self.device):
            out = self.enhance_device(frames_to_device([img], self.device), outscale)
            return frames_to_host(out)[0], "RGB"


def upscale_with_realesrgan(frames: List[np.ndarray], upsampler: RealESRGANer, **kwargs) -> List[np.ndarray]:
    """Presley's `upscale_with_realesrgan` (presley.py:1279-1314): RGB uint8 frames, each enhanced at `outscale` =
    int(degradation_level) (default 4) and resized back to its own size with Lanczos4; level 0 returns copies."""
    outscale = int(kwargs.get("degradation_level", 4))
    if outscale == 0:
        return [frame.copy() for frame in frames]
    restored = []
    with torch.cuda.device(upsampler.device):
        for frame in frames:
            h, w = frame.shape[:2]
            d = frames_to_device([frame], upsampler.device)
            up = upsampler.enhance_device(d, outscale=outscale, swap_rb=False)
            restored.append(frames_to_host(resize_lanczos4_device(up, h, w))[0])
    return restored
