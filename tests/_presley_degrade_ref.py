"""numpy restatement of Presley's adaptive degraders (elvis_amd/degrade.py, csrc/presley_degrade.hip) - what the GPU output is
pinned against, bit for bit.  Written from the rules, not from the kernels: the area resize walks OpenCV's table entry
by entry over whole planes, the Gaussian pass is the 2-D closed form (25 products, one rounding) instead of two
separable passes, and the taps are literals.  The INTER_LINEAR coefficients are oracle/degrade_ref.py's.

Three layers:
  * restated OpenCV primitives behind `cv` (the two cv2 calls the reference makes: `resize` with INTER_AREA or
    INTER_LINEAR on a square u8 block, `GaussianBlur(block, (5, 5), sigmaX=1.0)`);
  * the seven reference functions (utils.py:1101-1217, presley.py:968-1039) block by block, calling `cv` where the
    reference calls cv2.  `Recorder` can stand in for `cv` (and for the cv2 stub in
    tools/make_presley_degrade_golden.py): it notes per block what was asked and returns zeros, which is how the
    control flow is pinned against the reference's own code;
  * `scale_clip` / `blur_clip`: the same arithmetic over whole clips, blocks grouped by map value.
"""
from __future__ import annotations

import math
from typing import Callable, List, Tuple

import numpy as np

from oracle.degrade_ref import _linear_coef

INTER_LINEAR, INTER_AREA = 1, 3           # cv2's flag values
TAPS = (14, 62, 104, 62, 14)              # GaussianBlur (5, 5), sigma 1 on CV_8U: 8.8 fixed point, sum 256
MAX_ROUNDS = 64


# ----------------------------------------------------------------------------- restated OpenCV primitives
def reflect101(i: int, n: int) -> int:
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


def area_entries(src: int, dst: int) -> List[Tuple[int, int, np.float32]]:
    """computeResizeAreaTab (OpenCV 4.x resize.cpp) for one axis: (destination, source, float32 weight) in order."""
    scale = 1.0 / (dst / src)
    out = []
    for dx in range(dst):
        fsx1 = dx * scale
        fsx2 = fsx1 + scale
        cell_width = min(scale, src - fsx1)
        sx1 = math.ceil(fsx1)
        sx2 = min(math.floor(fsx2), src - 1)
        sx1 = min(sx1, sx2)
        if sx1 - fsx1 > 1e-3:
            out.append((dx, sx1 - 1, np.float32((sx1 - fsx1) / cell_width)))
        for sx in range(sx1, sx2):
            out.append((dx, sx, np.float32(1.0 / cell_width)))
        if fsx2 - sx2 > 1e-3:
            out.append((dx, sx2, np.float32(min(min(fsx2 - sx2, 1.0), cell_width) / cell_width)))
    return out


def resize_area_u8(blocks: np.ndarray, d: int) -> np.ndarray:
    """cv2.resize(INTER_AREA) of square u8 images [..., b, b, c] to d x d.  b % d == 0: the box sum, (sum + 2) >> 2 at
    ratio 2 and rint(float32(sum) * (1.f / area)) otherwise.  Any other d: ResizeArea_<uchar, float> - per source row
    buf[dx] += S[sx] * alpha over the table, per destination row sum[dx] += beta * buf[dx] over the same table, in
    float32 from 0, then saturate_cast<uchar> (round-half-even)."""
    lead, (b, _, c) = blocks.shape[:-3], blocks.shape[-3:]
    x = blocks.reshape((-1, b, b, c))
    if b % d == 0:
        fac = b // d
        sums = x.reshape(-1, d, fac, d, fac, c).astype(np.int64).sum(axis=(2, 4))
        if fac == 1:
            small = sums
        elif fac == 2:
            small = (sums + 2) >> 2
        else:
            small = np.rint(sums.astype(np.float32) * np.float32(1.0 / (fac * fac))).astype(np.int64)
    else:
        tab = area_entries(b, d)
        src = x.astype(np.float32)
        buf = np.zeros((x.shape[0], b, d, c), np.float32)
        for dx, sx, alpha in tab:
            buf[:, :, dx] = buf[:, :, dx] + src[:, :, sx] * alpha
        acc = np.zeros((x.shape[0], d, d, c), np.float32)
        for dy, sy, beta in tab:
            acc[:, dy] = acc[:, dy] + beta * buf[:, sy]
        small = np.rint(acc).astype(np.int64)
    return np.clip(small, 0, 255).astype(np.uint8).reshape(lead + (d, d, c))


def resize_linear_u8(small: np.ndarray, b: int) -> np.ndarray:
    """cv2.resize(INTER_LINEAR) of square u8 images [..., d, d, c] up to b x b: 11-bit coefficients, horizontal pass in
    int32, vertical pass ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2."""
    lead, (d, _, c) = small.shape[:-3], small.shape[-3:]
    s = small.reshape((-1, d, d, c)).astype(np.int64)
    coef = [_linear_coef(i, d, b) for i in range(b)]
    i0 = np.array([k[0] for k in coef])
    i1 = np.minimum(i0 + 1, d - 1)
    w0 = np.array([k[1] for k in coef], np.int64)
    w1 = np.array([k[2] for k in coef], np.int64)
    rows = s[:, :, i0] * w0[None, None, :, None] + s[:, :, i1] * w1[None, None, :, None]      # nb, d, b, c
    v = ((w0[None, :, None, None] * (rows[:, i0] >> 4)) >> 16) + ((w1[None, :, None, None] * (rows[:, i1] >> 4)) >> 16)
    return np.clip((v + 2) >> 2, 0, 255).astype(np.uint8).reshape(lead + (b, b, c))


def gaussian_pass_u8(blocks: np.ndarray) -> np.ndarray:
    """One cv2.GaussianBlur(img, (5, 5), sigmaX=1.0) of u8 images [..., h, w, c], each its own image: the closed form
    (sum_ij t_i t_j x[r(y + i - 2)][r(x + j - 2)] + 32768) >> 16 with r = BORDER_REFLECT_101."""
    h, w = blocks.shape[-3], blocks.shape[-2]
    x = blocks.astype(np.int64)
    ry = [[reflect101(y + i - 2, h) for y in range(h)] for i in range(5)]
    rx = [[reflect101(q + j - 2, w) for q in range(w)] for j in range(5)]
    acc = np.zeros(x.shape, np.int64)
    for i in range(5):
        rows = np.take(x, ry[i], axis=-3)
        for j in range(5):
            acc += TAPS[i] * TAPS[j] * np.take(rows, rx[j], axis=-2)
    return ((acc + 32768) >> 16).astype(np.uint8)


class Restated:
    """The two cv2 functions the reference's degraders call, restated."""
    INTER_LINEAR, INTER_AREA = INTER_LINEAR, INTER_AREA

    @staticmethod
    def resize(img, dsize, interpolation=INTER_LINEAR):
        assert img.ndim == 3 and img.dtype == np.uint8 and img.shape[0] == img.shape[1] and dsize[0] == dsize[1]
        if interpolation == INTER_AREA:
            assert dsize[0] <= img.shape[0]
            return resize_area_u8(img, dsize[0])
        assert interpolation == INTER_LINEAR and dsize[0] >= img.shape[0]
        return img.copy() if dsize[0] == img.shape[0] else resize_linear_u8(img, dsize[0])

    @staticmethod
    def GaussianBlur(img, ksize, sigmaX=0.0):
        assert tuple(ksize) == (5, 5) and sigmaX == 1.0 and img.dtype == np.uint8
        return gaussian_pass_u8(img)


cv = Restated()


def id_frame(h: int, w: int, block: int, channels: int = 3) -> np.ndarray:
    """A frame whose every whole block carries its raster index + 1 in channels 0 (low byte) and 1 (high byte), so that
    a stand-in for cv2 can tell which block it was handed (zeros: the output of an earlier stand-in call)."""
    by, bx = h // block, w // block
    ids = np.arange(by * bx, dtype=np.int64).reshape(by, bx) + 1
    frame = np.zeros((h, w, channels), np.uint8)
    frame[:by * block, :bx * block, 0] = np.kron(ids & 255, np.ones((block, block), np.int64))
    frame[:by * block, :bx * block, 1] = np.kron(ids >> 8, np.ones((block, block), np.int64))
    return frame


class Recorder:
    """Stands in for cv2 on an `id_frame`: per block, the target size and flag of the first and second resize and the
    number of GaussianBlur calls (kernel size and sigma in `kernels`); every call returns zeros of the right shape."""
    INTER_LINEAR, INTER_AREA = INTER_LINEAR, INTER_AREA

    def __init__(self, by: int, bx: int):
        self.bx = bx
        self.sizes = np.zeros((by, bx, 2), np.int32)
        self.flags = np.full((by, bx, 2), -1, np.int32)
        self.resizes = np.zeros((by, bx), np.int32)
        self.blurs = np.zeros((by, bx), np.int32)
        self.kernels = set()
        self.block = None

    def _where(self, img):
        ident = int(img[0, 0, 0]) + 256 * int(img[0, 0, 1])
        if ident:
            self.block = divmod(ident - 1, self.bx)
        return self.block

    def resize(self, img, dsize, interpolation=INTER_LINEAR):
        i, j = self._where(img)
        k = self.resizes[i, j]
        assert k < 2 and dsize[0] == dsize[1]
        self.sizes[i, j, k], self.flags[i, j, k] = dsize[0], interpolation
        self.resizes[i, j] += 1
        return np.zeros((dsize[1], dsize[0], img.shape[2]), np.uint8)

    def GaussianBlur(self, img, ksize, sigmaX=0.0):
        i, j = self._where(img)
        self.blurs[i, j] += 1
        self.kernels.add((int(ksize[0]), int(ksize[1]), float(sigmaX)))
        return np.zeros_like(img)


def golden_cases(path: str) -> Tuple[List[dict], set]:
    """tests/golden/presley_degrade.npz (tools/make_presley_degrade_golden.py) unpacked: per case the family, block,
    max_value, extra rows and columns, the importance input and, per block, what the reference returned and asked of
    cv2: map, touched, size0, flag0, size1, flag1, resizes, blurs."""
    z = np.load(path)
    cases, row, at = [], 0, {4: 0, 8: 0}
    for fam, b, max_value, eh, ew, by, bx, item in z["params"]:
        imp = z[f"importance_f{item}"][at[item]:at[item] + by * bx].reshape(by, bx)
        rec = z["records"][row:row + by * bx].reshape(by, bx, 8)
        at[item] += by * bx
        row += by * bx
        case = dict(family=str(z["families"][fam]), block=int(b), max_value=int(max_value), extra=(int(eh), int(ew)), importance=imp)
        case.update({k: rec[..., i] for i, k in enumerate(("map", "touched", "size0", "flag0", "size1", "flag1", "resizes", "blurs"))})
        cases.append(case)
    return cases, {tuple(k) for k in z["kernels"].tolist()}


# ----------------------------------------------------------------------------- the seven functions, block by block
def _each_block(frame: np.ndarray, values: np.ndarray, b: int, fn: Callable) -> np.ndarray:
    """The loop all of them share: a copy of the frame in which every whole block (i, j) with values[i, j] > 0 is
    replaced by fn(block, values[i, j]), in raster order; whatever lies past the last whole block stays."""
    out = frame.copy()
    for i in range(frame.shape[0] // b):
        for j in range(frame.shape[1] // b):
            if values[i, j] > 0:
                where = (slice(i * b, (i + 1) * b), slice(j * b, (j + 1) * b))
                out[where] = fn(np.ascontiguousarray(frame[where]), values[i, j])
    return out


def _need_grid(frame, per_block, b):
    if np.shape(per_block) != (frame.shape[0] // b, frame.shape[1] // b):
        raise ValueError("not the block grid")        # the build's departure: the reference resizes it bilinearly


def generate_degradation_map(importance, max_value):
    """presley.py:968-975: round-half-even of (1 - importance) * max_value in the array's dtype, int32, clipped."""
    return np.clip(np.round((1 - importance) * max_value).astype(np.int32), 0, max_value)


def downscale_block(block, scale):
    """presley.py:978-983: INTER_AREA to max(1, b // scale), INTER_LINEAR back."""
    b = block.shape[0]
    d = max(1, b // scale)
    return cv.resize(cv.resize(block, (d, d), interpolation=cv.INTER_AREA), (b, b), interpolation=cv.INTER_LINEAR)


def blur_block(block, rounds):
    """presley.py:986-990: `rounds` calls of GaussianBlur (5, 5), sigma 1."""
    for _ in range(rounds):
        block = cv.GaussianBlur(block, (5, 5), sigmaX=1.0)
    return block


def degrade_frame(frame, degradation_map, block_size, method: Callable):
    """presley.py:993-1013."""
    return _each_block(frame, degradation_map, block_size, method)


def degrade_video_adaptive(frames, importance_scores, block_size, max_value, method: Callable):
    """presley.py:1016-1039: (frames, maps) over the zipped clip."""
    maps = [generate_degradation_map(imp, max_value) for _, imp in zip(frames, importance_scores)]
    return [degrade_frame(f, m, block_size, method) for f, m in zip(frames, maps)], maps


def degrade_adaptive_downsample(frame, importance, block_size, max_scale=4):
    """utils.py:1101-1168: bins of floor((1 - importance) * max_scale) clipped to [0, max_scale - 1]; bin 0 keeps the
    block, bin k degrades it by the scale k + 1."""
    _need_grid(frame, importance, block_size)
    bins = np.clip(np.floor((1 - importance) * max_scale).astype(np.int32), 0, max_scale - 1)
    scales = np.where(bins == 0, 0, bins + 1).astype(np.int32)
    return _each_block(frame, scales, block_size, downscale_block), scales


def degrade_adaptive_blur(frame, importance, block_size, max_rounds=10):
    """utils.py:1171-1217: the map rule of generate_degradation_map, then `rounds` blur calls per block."""
    _need_grid(frame, importance, block_size)
    rounds = generate_degradation_map(importance, max_rounds)
    return _each_block(frame, rounds, block_size, blur_block), rounds


# ----------------------------------------------------------------------------- whole clips, grouped by map value
def _blocks(frames, grid, b):
    n, _, _, c = frames.shape
    by, bx = grid
    return frames[:, :by * b, :bx * b].reshape(n, by, b, bx, b, c).transpose(0, 1, 3, 2, 4, 5)


def _unblocks(out, blocks):
    n, by, bx, b, _, c = blocks.shape
    out[:, :by * b, :bx * b] = blocks.transpose(0, 1, 3, 2, 4, 5).reshape(n, by * b, bx * b, c)
    return out


def scale_clip(frames: np.ndarray, scales: np.ndarray, b: int) -> np.ndarray:
    """[n,H,W,C] u8, [n,H//b,W//b] scales: a block of scale >= 2 goes INTER_AREA to max(1, b // scale) and INTER_LINEAR
    back; scale <= 1 and the pixels past the last whole block are copied."""
    blocks = _blocks(frames, scales.shape[1:], b)
    res = blocks.copy()
    for scale in np.unique(scales[scales > 1]):
        sel = scales == scale
        res[sel] = resize_linear_u8(resize_area_u8(blocks[sel], max(1, b // int(scale))), b)
    return _unblocks(frames.copy(), res)


def blur_clip(frames: np.ndarray, rounds: np.ndarray, b: int) -> np.ndarray:
    """[n,H,W,C] u8, [n,H//b,W//b] rounds (clamped to [0, 64]): `rounds` Gaussian passes per block; rounds <= 0 and the
    pixels past the last whole block are copied."""
    blocks = _blocks(frames, rounds.shape[1:], b)
    res = blocks.copy()
    left = np.clip(rounds, 0, MAX_ROUNDS)
    while (left > 0).any():
        sel = left > 0
        res[sel] = gaussian_pass_u8(res[sel])
        left = left - sel
    return _unblocks(frames.copy(), res)
