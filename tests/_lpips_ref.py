"""The LPIPS (AlexNet) contract of include/elvis_amd.h and DESIGN.md 7 in torch float64 on the CPU, importable without a
GPU: the oracle of tests/test_gpu_lpips.py and tests/test_lpips_host.py, the case matrix, and the mutants - the contract
with one clause changed, each of which must move the score of its named case by at least 100 bars.

BUILD-DEFINED: this states what elvis_amd.lpips computes; it does not claim parity with the lpips package.

    input     u8 [n,H,W,3], order "bgr" or "rgb"; where mask == 0 the pixel's three bytes are 0; the rect (y0, y1, x0, x1)
              of the masked frame is what the network sees
    stem      t = byte / 127.5 - 1, x = (t - shift_c) / scale_c in RGB order; zero padding is 0 AFTER the affine
    trunk     conv 3->64 11x11 s4 p2, ReLU (tap 0); max-pool 3x3 s2 floor; conv 64->192 5x5 p2, ReLU (tap 1); max-pool;
              conv 192->384, 384->256, 256->256 3x3 p1, ReLU (taps 2, 3, 4)
    distance  xh = x / (sqrt(sum_c x^2) + 1e-10); v = sum_c w_c (xh_c - yh_c)^2; tap value = mean of v over the pixels;
              score = sum of the five tap values in tap order
(Putting the 1e-10 inside the sqrt would differ by 1e-11 relative: the rule is stated, not tested.)
"""
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
CONV_IDX = (0, 3, 6, 8, 10)
TAP_CHANNELS = (64, 192, 384, 256, 256)
MIN_SIDE = 31

# The end-to-end bar (relative to max(|ref|, 1e-6)).  CPU_F32_WORST is the largest distance of this file's restatement
# run in float32 on the CPU from the same in float64, over CASES with the seed-0 weights of weights.make_lpips_weights
# (tests/test_lpips_host.py re-measures it and asserts it has not grown); the device bar is 32 times that: the margin
# covers another summation order and the device's sqrt / divide.
#     CPU float32 worst 1.986e-6   |   device bar 6.37e-5   |   worst device value observed 1.72e-6 (MI355X, the one-LSB case)
CPU_F32_WORST = 1.99e-6
DEVICE_BAR = 32 * CPU_F32_WORST
MUTANT_MIN_BARS = 100

MUTANT_NAMES = ("ceil_mode", "channels_not_swapped", "masked_to_zero", "padding_affine0", "abs_diff", "spatial_sum",
                "rect_origin_ignored", "mask_ignored")


def affine(bytes_rgb: torch.Tensor, dtype) -> torch.Tensor:
    """[..., 3] byte values in RGB order -> the stem's input, in `dtype` arithmetic."""
    shift = torch.tensor(SHIFT, dtype=dtype)
    scale = torch.tensor(SCALE, dtype=dtype)
    return ((bytes_rgb.to(dtype) / 127.5 - 1.0) - shift) / scale


def affine_f32(bytes_rgb: np.ndarray) -> np.ndarray:
    """The kernel's own fp32 affine, IEEE operation by operation (numpy float32): what the stem multiplies."""
    b = bytes_rgb.astype(np.float32)
    return ((b / np.float32(127.5) - np.float32(1.0)) - np.asarray(SHIFT, np.float32)) / np.asarray(SCALE, np.float32)


def network_input(frames: np.ndarray, order="bgr", mask=None, rect=None, dtype=torch.float64, mutant=None) -> torch.Tensor:
    """u8 [n,H,W,3] -> [n,3,h,w] (NCHW, RGB) as the first conv sees it, without its padding."""
    x = torch.from_numpy(np.array(frames)).to(torch.int64)
    if order == "bgr" and mutant != "channels_not_swapped":
        x = x.flip(-1)
    keep = None
    if mask is not None and mutant != "mask_ignored":
        keep = torch.from_numpy(np.array(mask)) != 0
        if mutant != "masked_to_zero":
            x = torch.where(keep[..., None], x, torch.zeros_like(x))
    x = affine(x, dtype)
    if keep is not None and mutant == "masked_to_zero":
        x = torch.where(keep[..., None], x, torch.zeros_like(x))
    if rect is not None:
        y0, y1, x0, x1 = rect
        if mutant == "rect_origin_ignored":
            y0, y1, x0, x1 = 0, y1 - y0, 0, x1 - x0
        x = x[:, y0:y1, x0:x1]
    return x.permute(0, 3, 1, 2).contiguous()


def taps(x: torch.Tensor, sd, mutant=None):
    """The five ReLU outputs of the trunk for x [n,3,h,w] in x's dtype."""
    dt = x.dtype
    w = lambda i: sd[f"features.{i}.weight"].to(dt)
    b = lambda i: sd[f"features.{i}.bias"].to(dt)
    ceil = mutant == "ceil_mode"
    if mutant == "padding_affine0":
        pad = affine(torch.zeros(3, dtype=torch.int64), dt)
        xp = pad[None, :, None, None].expand(x.shape[0], 3, x.shape[2] + 4, x.shape[3] + 4).clone()
        xp[:, :, 2:-2, 2:-2] = x
        t0 = F.relu(F.conv2d(xp, w(0), b(0), stride=4, padding=0))
    else:
        t0 = F.relu(F.conv2d(x, w(0), b(0), stride=4, padding=2))
    t1 = F.relu(F.conv2d(F.max_pool2d(t0, 3, 2, ceil_mode=ceil), w(3), b(3), padding=2))
    t2 = F.relu(F.conv2d(F.max_pool2d(t1, 3, 2, ceil_mode=ceil), w(6), b(6), padding=1))
    t3 = F.relu(F.conv2d(t2, w(8), b(8), padding=1))
    t4 = F.relu(F.conv2d(t3, w(10), b(10), padding=1))
    return [t0, t1, t2, t3, t4]


def tap_distance(x: torch.Tensor, y: torch.Tensor, lin: torch.Tensor, mutant=None) -> torch.Tensor:
    """One tap: x, y [n,C,h,w], lin [C] -> float64 [n]."""
    xh = x / (torch.sqrt((x * x).sum(1, keepdim=True)) + 1e-10)
    yh = y / (torch.sqrt((y * y).sum(1, keepdim=True)) + 1e-10)
    d = xh - yh
    d = d.abs() if mutant == "abs_diff" else d * d
    v = (d * lin.to(x.dtype)[None, :, None, None]).sum(1).to(torch.float64)
    return v.sum((1, 2)) if mutant == "spatial_sum" else v.mean((1, 2))


def score(a: np.ndarray, b: np.ndarray, sd, order="bgr", mask=None, rect=None, dtype=torch.float64, mutant=None) -> np.ndarray:
    """The contract: u8 [n,H,W,3] x2 -> float64 [n]."""
    assert mutant is None or mutant in MUTANT_NAMES
    with torch.no_grad():
        ta = taps(network_input(a, order, mask, rect, dtype, mutant), sd, mutant)
        tb = taps(network_input(b, order, mask, rect, dtype, mutant), sd, mutant)
        total = torch.zeros(a.shape[0], dtype=torch.float64)
        for k in range(5):
            total = total + tap_distance(ta[k], tb[k], sd[f"lin{k}.model.1.weight"].reshape(-1), mutant)
    return total.numpy()


class Net:
    """A torch-module-shaped restatement for tools/make_lpips_golden.py: `net(ref, dec)` on [1,3,h,w] tensors in
    [-1, 1], RGB, as the reference's loop calls `lpips_model(ref_tensor, dec_tensor).item()`."""

    def __init__(self, sd, dtype=torch.float32):
        self.sd, self.dtype = sd, dtype

    def parameters(self):
        return iter([self.sd["features.0.weight"]])

    def __call__(self, ref, dec):
        shift = torch.tensor(SHIFT, dtype=self.dtype)[None, :, None, None]
        scale = torch.tensor(SCALE, dtype=self.dtype)[None, :, None, None]
        ta = taps((ref.to(self.dtype) - shift) / scale, self.sd)
        tb = taps((dec.to(self.dtype) - shift) / scale, self.sd)
        total = torch.zeros(ref.shape[0], dtype=torch.float64)
        for k in range(5):
            total = total + tap_distance(ta[k], tb[k], self.sd[f"lin{k}.model.1.weight"].reshape(-1))
        return total.reshape(-1, 1, 1, 1)


# ============================================================================================ cases
@dataclass(frozen=True)
class Case:
    id: str
    shape: Tuple[int, int, int]                       # n, H, W
    order: str = "bgr"
    rect: Optional[Tuple[int, int, int, int]] = None
    masked: bool = False                              # a mask that keeps about 60 % of the pixels
    pair: str = "noisy"                               # noisy | identical | one_lsb | black_white

    @property
    def seed(self):
        return zlib.crc32(self.id.encode())

    @property
    def kernels(self):
        return (f"lpips_stem_kernel<{int(self.order == 'bgr')}>", "lpips_maxpool_kernel", "lpips_conv5_kernel", "lpips_distance_kernel",
                "lpips_finish_kernel")


CASES = (
    Case("min_31x31", (1, 31, 31)),                                       # the minimum: a 1 x 1 last feature map
    Case("s32x35", (1, 32, 35)),                                          # floor and ceil pooling differ; the last conv column is dropped
    Case("s33x38", (1, 33, 38)),
    Case("s67x95", (1, 67, 95)),                                          # more than one tile of the stem and of the 5x5 conv
    Case("s47x64", (1, 47, 64)),
    Case("s32x35_rgb", (1, 32, 35), order="rgb"),
    Case("rect_odd_masked", (2, 70, 90), rect=(5, 64, 9, 82), masked=True),
    Case("n3_33x38", (3, 33, 38)),
    Case("identical", (1, 32, 35), pair="identical"),
    Case("one_lsb", (1, 32, 35), pair="one_lsb"),
    Case("black_white", (1, 31, 31), pair="black_white"),
)
BY_ID = {c.id: c for c in CASES}
MUTANTS = {
    "ceil_mode": "s33x38",
    "channels_not_swapped": "s47x64",
    "masked_to_zero": "rect_odd_masked",
    "padding_affine0": "min_31x31",
    "abs_diff": "s47x64",
    "spatial_sum": "s47x64",
    "rect_origin_ignored": "rect_odd_masked",
    "mask_ignored": "rect_odd_masked",
}
assert set(MUTANTS) == set(MUTANT_NAMES)

_INPUTS, _EXPECTED, _WEIGHTS = {}, {}, {}


def weights(seed: int = 0):
    if seed not in _WEIGHTS:
        from elvis_amd.weights import make_lpips_weights
        _WEIGHTS[seed] = make_lpips_weights(seed)
    return _WEIGHTS[seed]


def inputs(case: Case):
    """(a, b, mask or None): read-only uint8 arrays, the same for every call."""
    if case.id not in _INPUTS:
        rng = np.random.default_rng(case.seed)
        n, h, w = case.shape
        yy, xx = np.mgrid[:h, :w]
        base = np.stack([np.stack([110 + 80 * np.sin((yy + 3 * f) / 5.0 + k) * np.cos((xx - f) / 7.0 - k) for k in range(3)], axis=-1)
                         for f in range(n)])
        a = np.clip(base + rng.normal(0, 8, base.shape), 0, 255).astype(np.uint8)
        if case.pair == "identical":
            b = a.copy()
        elif case.pair == "one_lsb":
            b = a.copy()
            b[0, h // 2, w // 2, 1] ^= 1
        elif case.pair == "black_white":
            a, b = np.zeros_like(a), np.full_like(a, 255)
        else:
            b = np.clip(a.astype(np.float64) + rng.normal(0, 12, a.shape), 0, 255).astype(np.uint8)
        m = None
        if case.masked:
            m = (rng.random((n, h, w)) < 0.6).astype(np.uint8) * rng.choice(np.array([1, 2, 128, 255], np.uint8), (n, h, w))
        for arr in (a, b, m):
            if arr is not None:
                arr.setflags(write=False)
        _INPUTS[case.id] = (a, b, m)
    return _INPUTS[case.id]


def expected(case_id: str, mutant=None, dtype=torch.float64) -> np.ndarray:
    """float64 [n] of a case, computed once and shared."""
    key = (case_id, mutant, dtype)
    if key not in _EXPECTED:
        case = BY_ID[case_id]
        a, b, m = inputs(case)
        out = score(a, b, weights(), case.order, m, case.rect, dtype, mutant)
        out.setflags(write=False)
        _EXPECTED[key] = out
    return _EXPECTED[key]


def rel(got, ref) -> float:
    """The largest |got - ref| / max(|ref|, 1e-6)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-6)).max())
