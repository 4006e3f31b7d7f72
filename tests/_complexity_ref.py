"""The block-complexity contract (include/elvis_amd.h) in numpy float64, written without the kernel's tiling:
the luma of the whole clip, its blocks by one reshape, both DCT passes by one einsum over all blocks at once.  Also the
named mutants - each changes one clause of the contract - and the case lists of tests/test_complexity_host.py and
tests/test_gpu_complexity.py.  The device output is held to `BAR` against this; the mutants are at least a thousand bars
away on their named cases (tests/test_complexity_host.py)."""
import functools
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

# |device - reference| <= BAR * max(1, |reference|).  Derived, not measured.  With u = 1.1e-16 (float64): a coefficient is
# two nested dot products of length B <= 32 over |X'| <= 510 and basis entries <= sqrt(2 / B) = 0.25, so its absolute error
# is at most about 2 * 32 * u * (32 * 0.25)^2 * 510 ~ 2.3e-10 whatever the order of the additions (and far less on
# average); the weights are at most e, the sum of B^2 such terms is divided by B^2 (an average), and its own additions
# add B^2 * u ~ 1.1e-13 relative.  That is a few 1e-10 at the very worst (every rounding at its maximum and of one
# sign, at B = 32) for any evaluation order, under 1e-9 * max(1, |value|); values reach 510 e ~ 1.4e3, where the relative
# form applies.  Two float64 evaluation orders on the host (einsum against matrix products) differ by some 1e-15.
BAR = 1e-9
BLOCKS = (8, 16, 32)
STRIP_PIXELS = 1024                      # CX_TILE of csrc/complexity.hip: a workgroup takes 1024 / B^2 neighbouring blocks
MUTANT_MIN = 1e-6                        # what every mutant must move its case by: a thousand bars

MUTANTS = {                              # mutant -> the case it must move
    "dc_weight_kept": "named_b16_rgb_prev",
    "transposed_passes": "named_b16_rgb_prev",
    "s0_equals_sk": "named_b16_rgb_prev",
    "division_dropped": "named_b16_rgb_prev",
    "tc_against_next_frame": "named_b16_rgb_prev",
    "origin_shifted_by_remainder": "named_b8_gray_remainder",
    "rgb_bgr_swapped": "named_b32_bgr",
    "full_range_luma": "named_b32_bgr",
    "prev_ignored": "named_b16_rgb_prev",
}


# ============================================================================================ the contract
def luma(frames: np.ndarray, order: str = "rgb", mutant: Optional[str] = None) -> np.ndarray:
    """u8 [n,H,W,C] -> int64 [n,H,W]: the byte (C == 1) or the Y the encoder is handed (C == 3)."""
    f = frames.astype(np.int64)
    if f.shape[3] == 1:
        return f[..., 0]
    if mutant == "rgb_bgr_swapped":
        order = "bgr" if order == "rgb" else "rgb"
    r, g, b = (f[..., 0], f[..., 1], f[..., 2]) if order == "rgb" else (f[..., 2], f[..., 1], f[..., 0])
    if mutant == "full_range_luma":
        return (299 * r + 587 * g + 114 * b) // 1000
    return (269484 * r + 528482 * g + 102760 * b + (1 << 19) + (16 << 20)) >> 20


def tables(block: int, mutant: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
    k = np.arange(block)
    scale = np.full(block, np.sqrt(2.0 / block))
    if mutant != "s0_equals_sk":
        scale[0] = np.sqrt(1.0 / block)
    dct = scale[:, None] * np.cos(np.pi * (2 * k[None, :] + 1) * k[:, None] / (2 * block))
    weight = np.exp(np.abs((np.outer(k, k) / block ** 2) ** 2 - 1.0))
    if mutant != "dc_weight_kept":
        weight[0, 0] = 0.0
    return dct, weight


def blocks_of(planes: np.ndarray, block: int, mutant: Optional[str] = None) -> np.ndarray:
    """int64 [n,H,W] -> [n,By,Bx,B,B]; the remainder rows and columns belong to no block."""
    n, h, w = planes.shape
    by, bx = h // block, w // block
    y0, x0 = (h - by * block, w - bx * block) if mutant == "origin_shifted_by_remainder" else (0, 0)
    return planes[:, y0:y0 + by * block, x0:x0 + bx * block].reshape(n, by, block, bx, block).transpose(0, 1, 3, 2, 4)


def energy(x: np.ndarray, block: int, mutant: Optional[str] = None) -> np.ndarray:
    """Integer blocks [..., B, B] -> (sum weight |D X' D^T|) / B^2, X' = X - X[0][0]."""
    dct, weight = tables(block, mutant)
    xp = (x - x[..., :1, :1]).astype(np.float64)
    if mutant == "transposed_passes":
        cf = np.einsum("yk,...yx,xl->...kl", dct, xp, dct)
    else:
        cf = np.einsum("ky,...yx,lx->...kl", dct, xp, dct)
    total = (weight * np.abs(cf)).sum(axis=(-2, -1))
    return total if mutant == "division_dropped" else total / block ** 2


def complexity(frames: np.ndarray, block: int, order: str = "rgb", prev: Optional[np.ndarray] = None,
               mutant: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
    """frames u8 [n,H,W,C], prev None or u8 [H,W,C] -> (SC, TC), float64 [n,By,Bx]."""
    if mutant == "prev_ignored":
        prev = None
    x = blocks_of(luma(frames, order, mutant), block, mutant)
    sc = energy(x, block, mutant)
    if mutant == "tc_against_next_frame":
        other = np.concatenate([x[1:], x[-1:]])
    else:
        first = x[:1] if prev is None else blocks_of(luma(prev[None], order, mutant), block, mutant)
        other = np.concatenate([first, x[:-1]])
    return sc, energy(x - other, block, mutant)


def within_bar(got: np.ndarray, want: np.ndarray) -> bool:
    return got.shape == want.shape and bool((np.abs(got - want) <= BAR * np.maximum(1.0, np.abs(want))).all())


def worst(got: np.ndarray, want: np.ndarray) -> float:
    """The largest |got - want| / max(1, |want|): 1.0 * BAR is the limit."""
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()) if want.size else 0.0


# ============================================================================================ cases
@dataclass(frozen=True)
class Case:
    id: str
    block: int
    shape: Tuple[int, int, int, int]          # n, h, w, c
    order: str = "rgb"
    prev: bool = False

    @property
    def kernel(self) -> str:                  # what elvis_last_launch reports after the call
        return f"block_complexity_kernel<{self.block},{self.shape[3]},{int(self.order == 'bgr')}>"

    @property
    def grid(self) -> Tuple[int, int]:
        return self.shape[1] // self.block, self.shape[2] // self.block


COLOURS = ((1, "rgb"), (3, "rgb"), (3, "bgr"))


def sizes(block: int):
    return (block, block + 1, 2 * block - 1, 2 * block, 3 * block + 5)


def _matrix():
    out = []
    for b in BLOCKS:
        for c, order in COLOURS:
            for h in sizes(b):
                for w in sizes(b):
                    for n in (1, 2, 3):
                        out.append(Case(f"m_b{b}_c{c}{order}_{h}x{w}_n{n}", b, (n, h, w, c), order, prev=(h + w + n) % 2 == 1))
            # more blocks in a row than one workgroup takes at any block size (16, 4 and 1), and a last strip that is not full
            out.append(Case(f"wide_b{b}_c{c}{order}", b, (2, 3 * b + 1, 17 * b + 3, c), order, prev=True))
    return out


MATRIX = _matrix()
NAMED = [
    Case("named_b16_rgb_prev", 16, (3, 37, 53, 3), "rgb", prev=True),
    Case("named_b8_gray_remainder", 8, (2, 21, 29, 1)),
    Case("named_b32_bgr", 32, (2, 32, 69, 3), "bgr"),
]
CASES = MATRIX + NAMED
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def inputs(case: Case) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """Random bytes, seeded by the case's name: (frames u8 [n,h,w,c], prev u8 [h,w,c] or None)."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    n, h, w, c = case.shape
    frames = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
    return frames, (rng.integers(0, 256, (h, w, c), dtype=np.uint8) if case.prev else None)


@functools.lru_cache(maxsize=None)
def expected(case_id: str) -> Tuple[np.ndarray, np.ndarray]:
    """(SC, TC) of a case, computed once; the arrays are read-only."""
    case = BY_ID[case_id]
    frames, prev = inputs(case)
    sc, tc = complexity(frames, case.block, case.order, prev)
    sc.setflags(write=False)
    tc.setflags(write=False)
    return sc, tc
