"""A bit-exact numpy model of csrc/gn_fused.hip (gn_partials_affine_kernel), independent of the two launches it replaced,
the paths of the kernel a case reaches, and the case lists of tests/test_gpu_gn_fused.py.

The model is the order of operations the source's header states, nothing of its tiling:
  * per (image, channel, statistic) 256 virtual lanes; lane v adds tiles v, v + 256, ... in float64 from 0;
  * the tree  lane[v] += lane[v + o], o = 128 ... 1;
  * the group's sum over its channels, ascending, from 0;
  * gn_affine_kernel's arithmetic with its float32 casts.
Every operation is one IEEE add, multiply, divide or square root (the library is built with -ffp-contract=off and numpy
does not contract), so the bits are the kernel's.  `mutant=` changes one of the three orders; tests/test_gn_fused_host.py
shows that each changes a bit of pa or pb on the case named for it.

Inputs.  fp32 values a few binades apart add exactly in float64 in ANY order - 53 bits hold them all - so on such inputs
no order can be told from another, and a last-bit difference of a float64 sum would not reach the float32 pa and pb
anyway.  `partials` therefore plants pairs +X, -X of about 2^56 among ordinary values: between the two, an accumulator
drops the low bits of whatever it holds, so every order of the sum gives a visibly different mean.

`paths` restates, from the source's own expressions (asserted as literal text by the host test), which parts of the kernel
run for (c, groups, tiles).
"""
from __future__ import annotations

from typing import Dict, Optional, Set, Tuple

import numpy as np

MUTANTS = ("sequential", "pairwise_from_low", "group_sum_descending")
LANES = 256
GNF_MAX_F = 64
TILES = (1, 2, 7, 255, 256, 257, 511, 512, 513, 768, 769)
PATHS = ("short_last_workgroup", "idle_threads", "double_sweep", "single_sweep", "ragged_tail", "no_tail", "F64_full_row")

# literal text of csrc/gn_fused.hip that `span_of`, `row_lanes` and `paths` restate
SOURCE_TEXT = (
    "constexpr int GNF_MAX_F = 64;",
    "constexpr int K = 256 / RL;",
    "const int span = (c - ch0 < cb ? c - ch0 : cb) * 2;",
    "const int F = cb * 2;",
    "const int r = tid / F, f = tid - r * F;",
    "const bool active = r < RL && f < span;",
    "if constexpr (K <= 32) {",
    "for (; t0 + 512 <= tiles_per_image; t0 += 512) {",
    "for (; t0 + 256 <= tiles_per_image; t0 += 256) {",
    "if (t0 < tiles_per_image) {",
    "const int left = tiles_per_image - t0 - r;",
    "const long long off = RL * k < left ? k * kstride : -(long long)r * c * 2;",
    "if (cpg * 2 > GNF_MAX_F) return 0;",
    "return (16 + cpg - 1) / cpg * cpg;",
    "if (cb * 2 <= 32) {",
    "const dim3 grid((c + cb - 1) / cb, n);",
)


# ============================================================================================ the kernel's geometry
def span_of(c: int, groups: int) -> int:
    """elvis_gn_partials_affine_span: channels a workgroup spans (0: a group is wider than the kernel's row)."""
    if c <= 0 or groups <= 0 or c % groups:
        return 0
    cpg = c // groups
    if cpg * 2 > GNF_MAX_F:
        return 0
    return (16 + cpg - 1) // cpg * cpg


def row_lanes(c: int, groups: int) -> int:
    """RL of the instantiation the entry launches."""
    return 8 if span_of(c, groups) * 2 <= 32 else 4


def paths(c: int, groups: int, tiles: int) -> Set[str]:
    cb = span_of(c, groups)
    F, RL = cb * 2, row_lanes(c, groups)
    K = LANES // RL
    out = set()
    if c % cb:
        out.add("short_last_workgroup")              # the last ch0 has c - ch0 < cb
    if (LANES - 1) // F >= RL:
        out.add("idle_threads")                      # a thread with r = tid / F >= RL
    if F == GNF_MAX_F:
        out.add("F64_full_row")
    t0 = 0
    if K <= 32:
        while t0 + 512 <= tiles:
            out.add("double_sweep")
            t0 += 512
    while t0 + 256 <= tiles:
        out.add("single_sweep")
        t0 += 256
    if t0 < tiles:
        # some thread clamps a row: RL k >= left = tiles - t0 - r for r = RL - 1, k = K - 1 whenever fewer than 256 remain
        assert RL * (K - 1) >= tiles - t0 - (RL - 1)
        out.add("ragged_tail")
    else:
        out.add("no_tail")
    return out


# ============================================================================================ the model
def _lane_total(p: np.ndarray, mutant: Optional[str]) -> np.ndarray:
    """p float32 [n, tiles, c, 2] -> float64 [n, c, 2]."""
    n, tiles, c, _ = p.shape
    p64 = p.astype(np.float64)
    if mutant == "sequential":
        acc = np.zeros((n, c, 2), np.float64)
        for t in range(tiles):
            acc = acc + p64[:, t]
        return acc
    sweeps = -(-tiles // LANES)
    padded = np.zeros((n, sweeps * LANES, c, 2), np.float64)      # a lane without a tile adds +0: the same bits
    padded[:, :tiles] = p64
    padded = padded.reshape(n, sweeps, LANES, c, 2)
    lane = np.zeros((n, LANES, c, 2), np.float64)
    for k in range(sweeps):
        lane = lane + padded[:, k]
    if mutant == "pairwise_from_low":
        while lane.shape[1] > 1:
            lane = lane[:, 0::2] + lane[:, 1::2]
        return lane[:, 0]
    o = LANES // 2
    while o > 0:
        lane = np.concatenate([lane[:, :o] + lane[:, o:2 * o], lane[:, 2 * o:]], axis=1)
        o //= 2
    return lane[:, 0]


def model(p: np.ndarray, gamma, beta, scale, shift, hw: int, groups: int, eps: float, mutant: Optional[str] = None,
          info: Optional[Dict] = None) -> Tuple[np.ndarray, np.ndarray]:
    """p float32 [n, tiles, c, 2]; gamma, beta, scale, shift float32 [c] or None -> (pa, pb) float32 [n, c].
    `info`, when given, receives `var`: the variance of every (image, group) before the clamp."""
    assert mutant is None or mutant in MUTANTS, mutant
    p = np.asarray(p)
    assert p.dtype == np.float32 and p.ndim == 4 and p.shape[3] == 2
    n, tiles, c, _ = p.shape
    cpg = c // groups
    tot = _lane_total(p, mutant).reshape(n, groups, cpg, 2)
    s = np.zeros((n, groups), np.float64)
    ss = np.zeros((n, groups), np.float64)
    order = range(cpg - 1, -1, -1) if mutant == "group_sum_descending" else range(cpg)
    for k in order:
        s = s + tot[:, :, k, 0]
        ss = ss + tot[:, :, k, 1]
    cnt = np.float64(hw) * np.float64(cpg)
    mean = s / cnt
    var = ss / cnt - mean * mean
    if info is not None:
        info["var"] = var.copy()
    var = np.where(var < 0, 0.0, var)
    rstd = (1.0 / np.sqrt(var + np.float64(np.float32(eps)))).astype(np.float32)
    rep = lambda t: np.repeat(t, cpg, axis=1)
    f32 = lambda t, fill: np.full(c, fill, np.float32) if t is None else np.asarray(t, np.float32)
    a = rep(rstd) * f32(gamma, 1.0)[None]
    b = f32(beta, 0.0)[None] - rep(mean.astype(np.float32)) * a
    if scale is not None:
        sc = np.float32(1.0) + np.asarray(scale, np.float32)[None]
        a = a * sc
        b = b * sc + (np.asarray(shift, np.float32)[None] if shift is not None else np.float32(0.0))
    elif shift is not None:
        b = b + np.asarray(shift, np.float32)[None]
    assert a.dtype == np.float32 and b.dtype == np.float32
    return a, b


# ============================================================================================ inputs
_made: Dict[tuple, np.ndarray] = {}


def partials(n: int, tiles: int, c: int, cpg: int = 1) -> np.ndarray:
    """float32 [n, tiles, c, 2] per-tile (sum, sum of squares) of 256-pixel tiles, read-only.  The base is what
    tests/test_gpu_gn_fused.py always used: sums of either sign around +20 +- 50 and squares consistent with them.  On
    top, every channel with two tiles or more has +X at one tile and -X at another, X about 2^56: whatever a float64
    accumulator holds between the two loses its bits below 16, and WHICH values it holds then is the order of the sum.
    With cpg >= 2, tile 0 of the first two channels of every group holds +Y and -Y, Y about 2^57, which does the same to
    the group's sum over its channels.  Any reordering moves the mean by far more than a float32 ulp."""
    key = (n, tiles, c, cpg)
    if key not in _made:
        rng = np.random.default_rng([n, tiles, c, cpg])
        s = (rng.standard_normal((n, tiles, c)) * 50.0 + 20.0).astype(np.float32)
        ss = (s.astype(np.float64) ** 2 / 256.0 + np.abs(rng.standard_normal((n, tiles, c))) * 100.0 + 50.0).astype(np.float32)
        if tiles >= 2:
            for i in range(n):
                for ch in range(c):
                    a, b = rng.choice(tiles, 2, replace=False)
                    x = np.float32(np.exp2(56.0) * (1.0 + rng.random()))
                    s[i, a, ch], s[i, b, ch] = x, -x
        if cpg >= 2:
            y = (np.exp2(57.0) * (1.0 + rng.random((n, c // cpg)))).astype(np.float32)
            s[:, 0, 0::cpg], s[:, 0, 1::cpg] = y, -y
        out = np.stack([s, ss], -1)
        out.setflags(write=False)
        _made[key] = out
    return _made[key]


def params(c: int, on: bool):
    rng = np.random.default_rng(77 + c)
    gam = (rng.random(c) + 0.5).astype(np.float32)
    bet = (rng.standard_normal(c) * 0.3).astype(np.float32)
    sc = (rng.standard_normal(c) * 0.3).astype(np.float32)
    sh = (rng.standard_normal(c) * 0.3).astype(np.float32)
    return gam, bet, (sc if on else None), (sh if on else None)


def clamp_values(groups: int) -> np.ndarray:
    """One float32 v per group whose square is not a float32 and rounds DOWN: fl32(v v) < v v."""
    out, v = [], np.float32(1.1)
    while len(out) < groups:
        v = np.float32(v + np.float32(0.37))
        if float(np.float32(v * v)) < float(v) * float(v):
            out.append(v)
    return np.array(out, np.float32)


def clamp_partials(n: int, tiles: int, c: int, groups: int) -> np.ndarray:
    """Every tile of every channel of group g holds (256 v_g, fl32(256 v_g^2)).  The sums are exact in float64 (24-bit
    values times a small integer), the mean is v_g exactly, ss / cnt is fl32(v_g^2) exactly, and so the variance is
    fl32(v_g^2) - v_g^2 < 0 exactly: the clamp decides pa and pb."""
    v = np.repeat(clamp_values(groups), c // groups)
    row = np.stack([np.float32(256) * v, np.float32(256) * (v * v)], -1)          # x 256 is exact
    out = np.broadcast_to(row[None, None], (n, tiles, c, 2)).astype(np.float32)
    return np.ascontiguousarray(out)


# ============================================================================================ the cases
# (c, groups): cpg, span, F = 2 span, RL; the spans are the source's formula (asserted by both tests)
SHAPES = {(64, 32): 16, (96, 32): 18, (48, 16): 18, (24, 8): 18, (8, 8): 16, (16, 16): 16, (256, 32): 16, (320, 32): 20,
          (512, 32): 16, (640, 32): 20, (1024, 32): 32, (34, 2): 17, (90, 6): 30}
# every tile count on these five: RL = 8 whole, RL = 4 with idle threads and a short last workgroup, one short workgroup
# alone, the full 64-float row, an odd span
FULL = ((64, 32), (96, 32), (8, 8), (1024, 32), (34, 2))
N_IMAGES = 2
EPS = 1e-6


def gpu_cases():
    """(c, groups, tiles) of test_new_spans_equal_the_model_and_the_two_launches."""
    out = []
    for i, shape in enumerate(SHAPES):
        picks = TILES if shape in FULL else tuple(TILES[(i + j) % len(TILES)] for j in (0, 4, 8))
        out += [shape + (t,) for t in picks]
    return out


CLAMP_CASES = ((96, 32, 7), (8, 8, 257), (1024, 32, 2))

# mutant -> the (c, groups, tiles) of gpu_cases() on which it changes a bit of pa or pb
MUTANT_CASES = {"sequential": (64, 32, 769), "pairwise_from_low": (96, 32, 255), "group_sum_descending": (1024, 32, 7)}
