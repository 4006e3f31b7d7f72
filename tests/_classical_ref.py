"""numpy restatement of the classical restorers (elvis_amd/classical.py, csrc/classical.hip) - what the GPU output
is pinned against, bit for bit.  Independent of the device code apart from the shared tap tables
(`classical.lanczos_taps`, `classical.gaussian_taps_u8`, themselves pinned by check values in
tests/test_classical_host.py).

Two layers:
  * restated OpenCV primitives (INTER_AREA at an integer scale, 8-bit INTER_LANCZOS4, the bit-exact CV_8U
    GaussianBlur with BORDER_REFLECT_101, float32 addWeighted) and literal ports of the four reference functions
    (elvis.py:2773-2866, utils.py:1253-1392) with their block loops, the cv2 calls replaced by those primitives;
  * a vectorised restatement over whole clips (blocks grouped by level and tile geometry, the separable blur
    folded into integer matrices), fast enough for a 1080p frame.  The CPU tests pin the two against each other.
"""
from __future__ import annotations

from typing import List

import numpy as np

from elvis_amd.classical import gaussian_taps_u8, lanczos_taps


# ----------------------------------------------------------------------------- restated OpenCV primitives
def reflect101(i: int, n: int) -> int:
    """cv::borderInterpolate(i, n, BORDER_REFLECT_101), reflecting as often as needed."""
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


def resize_area_u8(img: np.ndarray, size: int) -> np.ndarray:
    """cv2.resize(img, (size, size), INTER_AREA) for a square u8 image at an integer scale (resizeAreaFast_)."""
    b, _, c = img.shape
    fac = b // size
    out = np.zeros((size, size, c), np.uint8)
    for y in range(size):
        for x in range(size):
            total = img[y * fac:(y + 1) * fac, x * fac:(x + 1) * fac].astype(np.int64).sum(axis=(0, 1))
            if fac == 2:
                v = (total + 2) >> 2
            else:
                v = np.rint(total.astype(np.float32) * np.float32(1.0 / (fac * fac))).astype(np.int64)
            out[y, x] = np.minimum(v, 255)
    return out


def resize_lanczos4_u8(img: np.ndarray, size: int) -> np.ndarray:
    """cv2.resize(img, (size, size), INTER_LANCZOS4) for a square u8 image upscaled by an integer factor:
    int taps, horizontal then vertical pass, BORDER_REPLICATE, (v + 2^21) >> 22 saturated."""
    s, _, c = img.shape
    first, taps = lanczos_taps(size // s, size)
    taps = taps.astype(np.int64)
    hp = np.zeros((s, size, c), np.int64)
    for r in range(s):
        for d in range(size):
            for k in range(8):
                hp[r, d] += img[r, min(max(first[d] + k, 0), s - 1)].astype(np.int64) * taps[d, k]
    out = np.zeros((size, size, c), np.uint8)
    for y in range(size):
        acc = np.zeros((size, c), np.int64)
        for k in range(8):
            acc += hp[min(max(first[y] + k, 0), s - 1)] * taps[y, k]
        out[y] = np.clip((acc + (1 << 21)) >> 22, 0, 255)
    return out


def gaussian_blur_u8(img: np.ndarray, sigma: int) -> np.ndarray:
    """cv2.GaussianBlur(img, (0, 0), sigma) on u8 (integer sigma): ksize = cvRound(6 sigma + 1) | 1, 8.8 taps,
    u8 x tap horizontal pass, u16 x tap vertical pass, one rounding (acc + 0x8000) >> 16, BORDER_REFLECT_101."""
    n = int(np.rint(sigma * 6 + 1)) | 1
    taps = gaussian_taps_u8(sigma).astype(np.int64)
    assert len(taps) == n
    r = n // 2
    th, tw, _ = img.shape
    src = img.astype(np.int64)
    hidx = np.array([[reflect101(x + k - r, tw) for k in range(n)] for x in range(tw)])
    hp = (src[:, hidx, :] * taps[None, None, :, None]).sum(axis=2)
    vidx = np.array([[reflect101(y + k - r, th) for k in range(n)] for y in range(th)])
    acc = (hp[vidx, :, :] * taps[None, :, None, None]).sum(axis=1)
    return ((acc + 0x8000) >> 16).astype(np.uint8)


def add_weighted_u8(a: np.ndarray, alpha: float, b: np.ndarray, beta: float) -> np.ndarray:
    """cv2.addWeighted(a, alpha, b, beta, 0) on u8: float32 arithmetic, cvRound, saturate."""
    v = a.astype(np.float32) * np.float32(alpha) + b.astype(np.float32) * np.float32(beta) + np.float32(0)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def nearest_resize(m: np.ndarray, rows: int, cols: int) -> np.ndarray:
    """cv2.resize(m, (cols, rows), INTER_NEAREST): source index floor(dst * src / dst)."""
    ri = [(i * m.shape[0]) // rows for i in range(rows)]
    ci = [(j * m.shape[1]) // cols for j in range(cols)]
    return m[ri][:, ci]


def extract_tile_with_halo(frame, y, x, tile_h, tile_w, halo):
    """utils.py:1227-1250."""
    h, w = frame.shape[:2]
    y0, x0 = max(0, y - halo), max(0, x - halo)
    y1, x1 = min(h, y + tile_h + halo), min(w, x + tile_w + halo)
    tile = frame[y0:y1, x0:x1].copy()
    crop = (y - y0, x - x0, y - y0 + tile_h, x - x0 + tile_w)
    return tile, crop


# ----------------------------------------------------------------------------- literal ports of the reference
def _split(image, b):
    h, w, c = image.shape
    if h % b or w % b:
        raise ValueError("Image dimensions must be divisible by block_size.")
    return image.reshape(h // b, b, w // b, b, c).swapaxes(1, 2)


def _combine(blocks):
    by, bx, b, _, c = blocks.shape
    return blocks.swapaxes(1, 2).reshape(by * b, bx * b, c)


def ref_restore_downsample_opencv_lanczos(downsampled_image, downscale_maps, block_size):
    """elvis.py:2773-2820 with the restated primitives."""
    downscale_factors = np.power(2, downscale_maps).astype(np.int32)
    max_factor = int(downscale_factors.max())
    if max_factor == 1:
        return downsampled_image
    num_blocks_y, num_blocks_x = downscale_maps.shape
    blocks = _split(downsampled_image, block_size)
    restored_blocks = np.zeros_like(blocks)
    for i in range(num_blocks_y):
        for j in range(num_blocks_x):
            factor = downscale_factors[i, j]
            if factor > 1:
                small_size = max(1, block_size // factor)
                small_block = resize_area_u8(blocks[i, j], small_size)
                restored_blocks[i, j] = resize_lanczos4_u8(small_block, block_size)
            else:
                restored_blocks[i, j] = blocks[i, j]
    return _combine(restored_blocks)


def ref_restore_blur_opencv_unsharp_mask(blurred_image, blur_maps, block_size):
    """elvis.py:2822-2866 with the restated primitives."""
    num_blocks_y, num_blocks_x = blur_maps.shape
    blocks = _split(blurred_image, block_size)
    restored_blocks = np.zeros_like(blocks)
    for i in range(num_blocks_y):
        for j in range(num_blocks_x):
            block = blocks[i, j]
            blur_strength = int(blur_maps[i, j])
            if blur_strength > 0:
                amount = blur_strength * 0.5
                radius = max(1, blur_strength)
                blurred = gaussian_blur_u8(block, radius)
                sharpened = add_weighted_u8(block, 1.0 + amount, blurred, -amount)
                restored_blocks[i, j] = np.clip(sharpened, 0, 255).astype(np.uint8)
            else:
                restored_blocks[i, j] = block
    return _combine(restored_blocks)


def ref_restore_with_opencv_unsharp(frames, degradation_maps, block_size, halo=0, temporal_blend=0.0) -> List[np.ndarray]:
    """utils.py:1315-1392 with the restated primitives (utils.py:1253-1312, `restore_with_opencv_lanczos`, is the
    same code)."""
    restored = []
    prev_output = None
    for i, frame in enumerate(frames):
        h, w = frame.shape[:2]
        blocks_y, blocks_x = h // block_size, w // block_size
        blur_map = degradation_maps[i] if len(degradation_maps) > i else np.zeros((blocks_y, blocks_x))
        if blur_map.shape != (blocks_y, blocks_x):
            blur_map = nearest_resize(blur_map.astype(np.float32), blocks_y, blocks_x).astype(np.int32)
        output = frame.copy()
        for by in range(blocks_y):
            for bx in range(blocks_x):
                blur_level = blur_map[by, bx]
                if blur_level > 0:
                    y, x = by * block_size, bx * block_size
                    if halo > 0:
                        tile, crop = extract_tile_with_halo(frame, y, x, block_size, block_size, halo)
                    else:
                        tile = frame[y:y + block_size, x:x + block_size].copy()
                        crop = (0, 0, block_size, block_size)
                    amount = blur_level * 0.5
                    radius = max(1, blur_level)
                    blurred = gaussian_blur_u8(tile, int(radius))
                    sharpened = add_weighted_u8(tile, 1.0 + amount, blurred, -amount)
                    sharpened = np.clip(sharpened, 0, 255).astype(np.uint8)
                    output[y:y + block_size, x:x + block_size] = sharpened[crop[0]:crop[2], crop[1]:crop[3]]
        if temporal_blend > 0 and prev_output is not None:
            output = (temporal_blend * prev_output + (1 - temporal_blend) * output).astype(np.uint8)
        prev_output = output.copy()
        restored.append(output)
    return restored


ref_restore_with_opencv_lanczos = ref_restore_with_opencv_unsharp


# ----------------------------------------------------------------------------- vectorised restatement
def _blocks(frames, levels, b):
    n, h, w, c = frames.shape
    by, bx = levels.shape[1:]
    return frames[:, :by * b, :bx * b].reshape(n, by, b, bx, b, c).transpose(0, 1, 3, 2, 4, 5)


def _unblocks(out, blocks):
    n, by, bx, b, _, c = blocks.shape
    out[:, :by * b, :bx * b] = blocks.transpose(0, 1, 3, 2, 4, 5).reshape(n, by * b, bx * b, c)
    return out


def lanczos_restore(frames: np.ndarray, levels: np.ndarray, b: int) -> np.ndarray:
    """[n,H,W,C] u8, [n,H//b,W//b] levels (clamped to [0, 16]): per block INTER_AREA to max(1, b >> L), then
    INTER_LANCZOS4 back to b."""
    blocks = _blocks(frames, levels, b)
    res = blocks.copy()
    lv = np.clip(levels, 0, 16)
    lb = int(np.log2(b))
    for level in np.unique(lv[lv > 0]):
        sel = lv == level
        blk = blocks[sel].astype(np.int64)
        nb, c = blk.shape[0], blk.shape[-1]
        lf = min(int(level), lb)
        fac, s = 1 << lf, b >> lf
        sums = blk.reshape(nb, s, fac, s, fac, c).sum(axis=(2, 4))
        if fac == 2:
            small = (sums + 2) >> 2
        else:
            small = np.rint(sums.astype(np.float32) * np.float32(1.0 / (fac * fac))).astype(np.int64)
        small = np.minimum(small, 255)
        first, taps = lanczos_taps(fac, b)
        idx = np.clip(first[:, None] + np.arange(8), 0, s - 1)
        t = taps.astype(np.int64)
        hp = (small[:, :, idx, :] * t[None, None, :, :, None]).sum(axis=3)           # nb, s, b, c
        v = (hp[:, idx, :, :] * t[None, :, :, None, None]).sum(axis=2)               # nb, b, b, c
        res[sel] = np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
    return _unblocks(frames.copy(), res)


def _fold(taps: np.ndarray, n: int, off: int, b: int) -> np.ndarray:
    """[b, n] integer matrix of the blur of a length-n signal at positions off .. off + b - 1 (REFLECT_101)."""
    r = len(taps) // 2
    m = np.zeros((b, n), np.int64)
    for i in range(b):
        for k, t in enumerate(taps):
            m[i, reflect101(off + i + k - r, n)] += int(t)
    return m


def _geometry(nblocks: int, b: int, halo: int, size: int):
    start = np.arange(nblocks) * b
    before = np.minimum(halo, start)
    t0 = start - before
    return t0, np.minimum(size, start + b + halo) - t0, before


def unsharp_restore(frames: np.ndarray, levels: np.ndarray, b: int, halo: int = 0) -> np.ndarray:
    """[n,H,W,C] u8, [n,H//b,W//b] levels (clamped to [0, 16]): per block of level L > 0 the unsharp mask
    (sigma L, amount L/2) of its tile (the block grown by `halo`, clipped at the frame); other pixels copied."""
    out = frames.copy()
    ry0, rth, rtop = _geometry(levels.shape[1], b, halo, frames.shape[1])
    cx0, ctw, cleft = _geometry(levels.shape[2], b, halo, frames.shape[2])
    lv = np.clip(levels, 0, 16)
    f, i, j = np.nonzero(lv > 0)
    if not len(f):
        return out
    keys = np.stack([lv[f, i, j], rth[i], rtop[i], ctw[j], cleft[j]], axis=1)
    uniq, inv = np.unique(keys, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    ar = np.arange(b)
    for g, (level, th, top, tw, left) in enumerate(uniq):
        m = inv == g
        ff, ii, jj = f[m], i[m], j[m]
        rows = ry0[ii][:, None] + np.arange(th)
        cols = cx0[jj][:, None] + np.arange(tw)
        tile = frames[ff[:, None, None], rows[:, :, None], cols[:, None, :]].astype(np.int64)
        taps = gaussian_taps_u8(int(level))
        acc = np.einsum("ir,nrqc->niqc", _fold(taps, th, top, b), tile)
        acc = np.einsum("jq,niqc->nijc", _fold(taps, tw, left, b), acc)
        blur = (acc + 0x8000) >> 16
        x = tile[:, top:top + b, left:left + b]
        v2 = (2 + level) * x - level * blur
        res = np.clip(np.rint(v2 / 2.0), 0, 255).astype(np.uint8)
        out[ff[:, None, None], (ii * b)[:, None, None] + ar[None, :, None], (jj * b)[:, None, None] + ar[None, None, :]] = res
    return out


def temporal_blend(frames: np.ndarray, tb: float) -> np.ndarray:
    """utils.py:1308-1312 over a [n,H,W,C] u8 clip."""
    out = frames.copy()
    for f in range(1, len(frames)):
        out[f] = (tb * out[f - 1] + (1 - tb) * frames[f]).astype(np.uint8)
    return out
