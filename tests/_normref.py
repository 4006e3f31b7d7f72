"""References with explicit error models for the kernels of csrc/norm.hip and csrc/misc.hip, and the case matrix of
tests/test_gpu_norm_misc_matrix.py (importable without a GPU: the ledger, the CPU pins and the mutation self-test of
tests/test_norm_misc_ledger.py use it on the CPU).

Two kinds of reference, by what the kernel promises:

  error-bounded  float64 of the operation on the stored inputs, returned as a `Bound` (tests/_modelref.py): `ref` and
                 the absolute term e1 of the value the kernel rounds to its output type, every piece derived from the
                 kernel's code below.  GroupNorm sums / affine / end to end, affine_act, LayerNorm, bicubic.
  exact          numpy float32, one IEEE operation per step (the kernels use __fmul_rn / __fadd_rn / __fdiv_rn and the
                 library is built with -ffp-contract=off), compared bit for bit.  VQ, u8 <-> float, reflect pad, crop,
                 dtype conversion.

U24 = 2^-24 is the fp32 unit roundoff; gamma(k) = (k + 2) U24 bounds an fp32 sum of k terms.  The keyword arguments
named "mutation hooks" exist for the self-test only.
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass, field
from fractions import Fraction
from typing import Optional

import numpy as np
import torch

from _convref import U24, elf_symbols, rne16, ulp16, ulp32  # noqa: F401
from _modelref import Bound, gamma, tier1, tier2  # noqa: F401

U53 = 2.0 ** -53
LN_FLT_MAX = 88.72283905206835        # expf / __expf overflow to +inf above this argument
TIER2_FLOOR = 0.998                   # interval form (tier2 of _modelref) on every f16 case; see exact_share_floor


@dataclass
class Bound64(Bound):
    """A Bound whose output is not rounded to f16 / fp32 (the fp64 sums): the bound is e1 alone."""

    def bound(self):
        return self.e1


def pitch_for(c: int) -> int:
    return (c + 7) // 8 * 8


def exact_share_floor(b: Bound):
    """(floor, near): `near` is the share of elements whose reference lies within e1 of an f16 rounding midpoint - only
    those may round either way when the kernel is within e1 - and floor = 1 - near rounded down to three decimals: the
    least share of outputs that must EQUAL RNE16(ref).  Computed from the float64 reference alone."""
    t = b.ref
    th = rne16(t)
    u = ulp16(t)
    mid = torch.minimum((t - (th + 0.5 * u)).abs(), (t - (th - 0.5 * u)).abs())
    near = float((mid <= b.e1).double().mean())
    return math.floor((1.0 - near) * 1000.0) / 1000.0, near


def exact_share(y: torch.Tensor, b: Bound) -> float:
    return float((y == rne16(b.ref)).double().mean())


# ============================================================================================ GroupNorm statistics
def gn_blocks(f16: bool, hw: int, c: int):
    """norm.hip gn_blocks restated: (workgroups per image, pixels per workgroup, pixel lanes pl_count)."""
    vec = 8 if f16 else 4
    cv = (c + vec - 1) // vec
    pl = max(256 // max(cv, 1), 1)
    ppb = max((hw + 2047) // 2048, pl * 16)
    return (hw + ppb - 1) // ppb, ppb, pl


def gn_workspace_floats(f16: bool, n: int, hw: int, c: int) -> int:
    return n * gn_blocks(f16, hw, c)[0] * c * 2


def gn_sums_k(f16: bool, hw: int, c: int) -> int:
    """Length of the fp32 accumulation chain of one partial: ceil(px_per_block / pl_count) per-thread terms (s += f,
    ss = fmaf(f, f, ss): one rounding each), then pl_count adds over the LDS planes."""
    _, ppb, pl = gn_blocks(f16, hw, c)
    return -(-ppb // pl) + pl


def gn_sums_ref(x: torch.Tensor, f16: bool, *, drop_slab: Optional[int] = None) -> Bound64:
    """x [n, hw, c] float64 of the stored values -> sums [n, c, 2] (sum, sum of squares).  The partial rows are then
    added in fp64 (tiles U53, negligible but counted).  drop_slab: mutation hook (one workgroup's pixels missing)."""
    n, hw, c = x.shape
    tiles, ppb, _ = gn_blocks(f16, hw, c)
    if drop_slab is not None:
        x = x.clone()
        x[:, drop_slab * ppb:(drop_slab + 1) * ppb] = 0
    g = gamma(gn_sums_k(f16, hw, c)) + (tiles + 8) * U53
    ref = torch.stack([x.sum(1), (x * x).sum(1)], -1)
    e1 = g * torch.stack([x.abs().sum(1), (x * x).sum(1)], -1) + 1e-300
    return Bound64(ref, e1, None, False)


def partials_ref(p: torch.Tensor, *, drop_row: Optional[int] = None) -> Bound64:
    """p [n, tiles, c, 2] float64 of the fp32 partials -> [n, c, 2]: ceil(tiles / 256) fp64 adds per thread and an 8-level
    tree: (tiles + 8) U53 of sum |p| covers any order."""
    if drop_row is not None:
        p = p.clone()
        p[:, drop_row] = 0
    return Bound64(p.sum(1), (p.shape[1] + 8) * U53 * p.abs().sum(1) + 1e-300, None, False)


# ============================================================================================ GroupNorm affine
def _group_stats(sums: torch.Tensor, hw: int, groups: int):
    """Exact (rational) mean and clamped variance of every group from fp64 sums [n, c, 2]; float64 [n, groups]."""
    n, c, _ = sums.shape
    cpg = c // groups
    cnt = hw * cpg
    mean = torch.empty(n, groups, dtype=torch.float64)
    var = torch.empty(n, groups, dtype=torch.float64)
    ex2 = torch.empty(n, groups, dtype=torch.float64)
    s_np = sums.numpy()
    for i in range(n):
        for g in range(groups):
            s = sum(Fraction(float(v)) for v in s_np[i, g * cpg:(g + 1) * cpg, 0])
            ss = sum(Fraction(float(v)) for v in s_np[i, g * cpg:(g + 1) * cpg, 1])
            m = s / cnt
            v = ss / cnt - m * m
            mean[i, g], var[i, g], ex2[i, g] = float(m), max(float(v), 0.0), float(ss / cnt)
    return mean, var, ex2


def _affine(mean, var, ex2, dm, dv, gamma_, beta, scale, shift, eps, cpg, *, eps_outside=False, rr_on_b=True):
    """pa, pb (float64, [n, c]) of gn_affine_kernel and their error terms.  mean / var / ex2 [n, groups]; dm, dv: what
    the kernel's mean and variance may be off by before this stage.  The kernel: fp64 group sums (cpg adds), mean, var =
    ss / cnt - mean^2 (about (cpg + 4) fp64 roundings of ex2 + mean^2, relevant when var << mean^2), the clamp,
    rstd = (float)(1 / sqrt(var + eps)); a = rstd * g; b = be - (float)mean * a; with scale: sc = 1 + scale, a *= sc,
    b = b * sc + shift (two roundings: no contraction); with shift alone: b += shift.
    rr is the relative error of rstd from the variance, ra the fp32 roundings gathered in a.  rr_on_b=False leaves rr
    out of pb's term (the end-to-end reference applies it to (x - mean) a instead)."""
    rep = lambda t: t.repeat_interleave(cpg, dim=1)
    dv = dv + (cpg + 4) * 2 * U53 * (ex2 + mean * mean)
    rstd = 1.0 / torch.sqrt(var + eps) if not eps_outside else 1.0 / (torch.sqrt(var) + eps)
    # |rstd' / rstd - 1| for any var' >= 0 within dv of var (not linearised: dv may exceed var + eps); sqrt and divide in fp64
    rr = torch.maximum(torch.sqrt((var + eps) / ((var - dv).clamp(min=0.0) + eps)) - 1.0,
                       1.0 - torch.sqrt((var + eps) / (var + dv + eps))) + 4 * U53      # the clamp caps the first
    mean, rstd, rr, dm = rep(mean), rep(rstd), rep(rr), rep(dm)
    c = mean.shape[1]
    ga = torch.ones(c, dtype=torch.float64) if gamma_ is None else gamma_
    be = torch.zeros(c, dtype=torch.float64) if beta is None else beta
    ra = 2 * U24                                   # rstd to fp32, times gamma
    a = rstd * ga
    ma = mean * a
    b = be - ma
    # a's error times |mean|, (float)mean, the product; the mean's own error times |a|; the subtraction
    db = ma.abs() * ((rr if rr_on_b else 0.0) + ra + 2 * U24) + dm * a.abs() * (1 + rr) + U24 * b.abs()
    if scale is not None:
        sc = 1.0 + scale                           # one rounding, then a *= sc
        a, ra = a * sc, ra + 2 * U24
        bs = b * sc
        b = bs + (shift if shift is not None else 0.0)
        db = db * sc.abs() + 2 * U24 * bs.abs() + (U24 * b.abs() if shift is not None else 0.0)
    elif shift is not None:
        b = b + shift
        db = db + U24 * b.abs()
    return a, b, a.abs() * (rr + ra), db, rr, ra


def gn_affine_ref(sums, gamma_, beta, scale, shift, hw, groups, eps, *, biased=True, eps_outside=False) -> Bound:
    """sums [n, c, 2] fp64 as given to the kernel (this stage alone) -> stack [pa, pb] of shape [2, n, c], fp32 outputs.
    Mutation hooks: biased=False (variance * cnt / (cnt - 1)), eps_outside (1 / (sqrt(var) + eps))."""
    n, c, _ = sums.shape
    cpg = c // groups
    mean, var, ex2 = _group_stats(sums, hw, groups)
    if not biased:
        var = var * (hw * cpg) / max(hw * cpg - 1, 1)
    z = torch.zeros_like(mean)
    a, b, da, db, _, _ = _affine(mean, var, ex2, z, z, gamma_, beta, scale, shift, eps, cpg, eps_outside=eps_outside)
    return Bound(torch.stack([a, b]), torch.stack([da, db]), None, False)


# ============================================================================================ affine_act / SiLU
def silu_terms(t: torch.Tensor, precise: bool, *, quick_gelu=False):
    """(silu(t) in float64, the error of the kernel's fp32 t / (1 + exp(-t)) for an exact fp32 t).
    expf (PRECISE, fp32 tensors): 1 ulp, 2^-23 relative.  __expf (f16 tensors): exp2 of the fp32 product -t * log2(e) on
    the transcendental unit - the product's rounding moves the exponential by U24 |t| relative, the rounded constant by
    another U24 |t|, and the unit itself is ALLOWED 2 ulp = 2^-22 (assumed: the device library's documentation is not
    part of this repository; DESIGN.md records the observed ratio).  With e = exp(-t) of relative error de the
    denominator 1 + e is off by de e / (1 + e) + U24 relative and the correctly rounded division adds U24.  Where
    exp(-t) overflows fp32 (-t > ln FLT_MAX) the kernel computes t / inf = -0 and the whole (tiny) reference is the
    error; 2^-126 covers flushed subnormals."""
    s = t * torch.sigmoid(1.702 * t) if quick_gelu else t * torch.sigmoid(t)
    de = torch.full_like(t, 2.0 ** -23) if precise else 2.0 ** -22 + 2 * U24 * t.abs()
    sg = torch.sigmoid(-t)                              # e / (1 + e)
    err = s.abs() * (de * sg + 2 * U24) + 2.0 ** -126
    err = torch.where(-t > LN_FLT_MAX - 1e-3 * 88, s.abs() + err, err)
    return s, err


SILU_LIP = 1.0999     # max |silu'|


def affine_act_ref(x, pa, pb, act: int, f16: bool, *, dpa=None, dpb=None, quick_gelu=False) -> Bound:
    """x [n, hw, c] stored values, pa / pb [n, c] (the fp32 values as float64) -> act(fma(x, a, b)).  One rounding of
    |t| for the fma (that rounding IS the output's for fp32 without an activation: 4 U53 only covers the reference's
    own), then SiLU.  dpa / dpb: what pa / pb may be off by (the end-to-end reference)."""
    a, b = pa[:, None, :], pb[:, None, :]
    t = x * a + b
    dt = U24 * t.abs() if (f16 or act == 2) else 4 * U53 * t.abs()
    if dpa is not None:
        dt = dt + x.abs() * dpa[:, None, :] + dpb[:, None, :]
    if act == 0:
        return Bound(t, dt, dt, f16)
    s, es = silu_terms(t, precise=not f16, quick_gelu=quick_gelu)
    e = SILU_LIP * dt + es
    return Bound(s, e, e, f16)


def groupnorm_ref(xs, f16: bool, gamma_, beta, scale, shift, groups: int, eps: float, act: int) -> Bound:
    """End to end: elvis_groupnorm_sums of every x in xs (the virtual channel concat; [n, hw, c_i] stored values) ->
    elvis_groupnorm_affine -> elvis_affine_act of every part; out [n, hw, sum c_i].
    The sums' errors (gn_sums_ref) move the mean by dm = dS / cnt and the variance by dv = dSS / cnt + 2 |mean| dm +
    dm^2: relative to var + eps that is eps32 (mean^2 + var) / var times the chain length - the cancellation of
    E[x^2] - mean^2 from fp32 partials, carried by the bound.  rstd's error multiplies (x - mean) a - the part of
    x pa + pb it is common to - so it is applied to |x - mean||a| here, not to |x a| and |mean a| separately; the fp32
    roundings of a, (float)mean, mean a and b are applied to |x a| and |mean a|."""
    n, hw, _ = xs[0].shape
    x = torch.cat(xs, -1)
    c = x.shape[-1]
    cpg = c // groups
    sb = [gn_sums_ref(t, f16) for t in xs]
    sums = torch.cat([b.ref for b in sb], 1)
    dsum = torch.cat([b.e1 for b in sb], 1)
    cnt = hw * cpg
    mean, var, ex2 = _group_stats(sums, hw, groups)
    dg = dsum.view(n, groups, cpg, 2).sum(2) / cnt
    dm = dg[..., 0]
    dv = dg[..., 1] + 2 * mean.abs() * dm + dm * dm
    z = torch.zeros_like(mean)
    a, b, _, db, rr, ra = _affine(mean, var, ex2, dm, dv, gamma_, beta, scale, shift, eps, cpg, rr_on_b=False)
    rep = lambda t: t.repeat_interleave(cpg, dim=1)[:, None, :]
    A = a.abs()[:, None, :]
    dt_pre = (x - rep(mean)).abs() * A * rr[:, None, :] + x.abs() * A * ra + db[:, None, :]
    zero = torch.zeros_like(a)
    out = affine_act_ref(x, a, b, act, f16, dpa=zero, dpb=zero)
    e = out.e1 + (SILU_LIP if act == 2 else 1.0) * dt_pre
    return Bound(out.ref, e, e, f16)


# ============================================================================================ LayerNorm
def ln_lpt(c: int, f16: bool) -> int:
    vec = 8 if f16 else 4
    lpt = 1
    while lpt < c // vec:
        lpt <<= 1
    return lpt


def layernorm_ref(x, gamma_, beta, eps: float, f16: bool, *, drop_lane: Optional[int] = None,
                  mean_over_lanes=False) -> Bound:
    """x [tokens, c] stored values.  layernorm_kernel: a lane adds its VEC values, log2(lpt) shuffle adds: a chain of
    k = VEC + log2(lpt) fp32 adds, gamma(k) sum|x|; mean = s / c (one rounding): dm.  d = x - mean' (one rounding each),
    q = sum d^2 by fmaf and the same tree: as sum (x - mean) = 0 a shifted mean adds exactly c dm^2 to q, the roundings
    (2 U24 + gamma(k)) q; q / c + eps, sqrtf, 1.0f / .: 4 roundings.  out = ((x - mean) * rstd) * g + b: three roundings
    of the product, one of the sum.  Mutation hooks: drop_lane (that lane's VEC values missing from the sum), mean_over_
    lanes (s / (lpt * VEC))."""
    T, c = x.shape
    vec = 8 if f16 else 4
    lpt = ln_lpt(c, f16)
    k = vec + int(math.log2(lpt))
    xs = x
    if drop_lane is not None:
        xs = x.clone()
        xs[:, drop_lane * vec:(drop_lane + 1) * vec] = 0
    mean = xs.sum(-1, keepdim=True) / (lpt * vec if mean_over_lanes else c)
    d = x - mean
    q = (d * d).sum(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(q / c + eps)
    t = d * rstd * gamma_ + beta
    dm = gamma(k) * x.abs().sum(-1, keepdim=True) / c + U24 * mean.abs()
    dq = c * dm * dm + (2 * U24 + gamma(k)) * q + 2 * U24 * dm * d.abs().sum(-1, keepdim=True)
    rr = torch.maximum(torch.sqrt((q + c * eps) / ((q - dq).clamp(min=0.0) + c * eps)) - 1.0,
                       1.0 - torch.sqrt((q + c * eps) / (q + dq + c * eps))) + 4 * U24
    e = dm * rstd * (1 + rr) * gamma_.abs() + d.abs() * rstd * gamma_.abs() * (rr + 3 * U24) + U24 * t.abs() + 1e-300
    return Bound(t, e, e, f16)


# ============================================================================================ bicubic
def _cubic_weights(t: torch.Tensor, A: float):
    c1 = lambda v: ((A + 2.0) * v - (A + 3.0)) * v * v + 1.0
    c2 = lambda v: ((A * v - 5.0 * A) * v + 8.0 * A) * v - 4.0 * A
    return torch.stack([c2(t + 1.0), c1(t), c1(1.0 - t), c2(2.0 - t)], -1)


def bicubic_ref(x, sf: int, f16: bool, *, A: float = -0.75, clamp=True, align_corners=False) -> Bound:
    """x [n, h, w, c] stored values -> [n, h sf, w sf, c]: Keys cubic A = -0.75, half-pixel centres, border clamp.
    bicubic_kernel: s = rs (o + 0.5) - 0.5 with rs = 1.0f / sf - exact for sf 1, 2, 4; for sf = 3 rs, the product and the
    subtraction round: the position is off by at most 3 U24 (|s| + 1), the weights (|w'| <= 1.35) by 1.35 times that;
    t = s - floor(s) is exact.  The Horner forms of cubic1 / cubic2 (intermediates <= 6, five operations, later
    multiplications by <= 2) are off by at most 16 U24.  Then rowv += x * wx (4 x 2 roundings), acc += rowv * wy
    (4 x 2): a chain of 20 roundings (with the slack of gamma) on sum |wy||wx||x|.
    Mutation hooks: A, clamp=False (out-of-image taps read as zero), align_corners."""
    n, h, w, c = x.shape
    ho, wo = h * sf, w * sf

    def axis(size, osize):
        o = torch.arange(osize, dtype=torch.float64)
        s = (o * (size - 1) / max(osize - 1, 1)) if align_corners else (o + 0.5) / sf - 0.5
        f = torch.floor(s)
        wts = _cubic_weights(s - f, A)
        idx = f.long()[:, None] + torch.arange(-1, 3)[None, :]
        ok = (idx >= 0) & (idx < size)
        dpos = torch.zeros_like(s) if sf in (1, 2, 4) else 3 * U24 * (s.abs() + 1.0)
        dw = (1.35 * dpos + 16 * U24)[:, None].expand(-1, 4)
        if not clamp:
            wts = wts * ok
        return idx.clamp(0, size - 1), wts, dw

    iy, wy, dwy = axis(h, ho)
    ix, wx, dwx = axis(w, wo)
    g = x[:, iy][:, :, :, ix]                            # [n, ho, 4, wo, 4, c]
    W = wy[:, :, None, None] * wx[None, None, :, :]      # [ho, 4, wo, 4]
    Wa = W.abs()
    dW = (wy.abs()[:, :, None, None] * dwx[None, None] + dwy[:, :, None, None] * wx.abs()[None, None]
          + dwy[:, :, None, None] * dwx[None, None])
    ref = (g * W[None, ..., None]).sum((2, 4))
    e = (g.abs() * (gamma(20) * Wa + dW)[None, ..., None]).sum((2, 4)) + 1e-300
    return Bound(ref, e, e, f16)


# ============================================================================================ exact references
F32 = np.float32


def np_store(v: np.ndarray, f16: bool) -> np.ndarray:
    return v.astype(np.float16) if f16 else v.astype(np.float32)


def vq_ref(z: np.ndarray, codebook: np.ndarray, *, last_wins=False, fused=False):
    """z [P, c] float32 (the stored values), codebook [K, c] float32 -> (idx int32 [P], codebook[idx]).  Distances
    ((dx dx) + dy dy) + dz dz ... in float32, one rounding per operation; the first minimum wins.
    Mutation hooks: last_wins; fused (the adds as fused multiply-adds, evaluated in float64 and rounded once each)."""
    P, c = z.shape
    idx = np.empty(P, np.int32)
    for p0 in range(0, P, 256):
        df = z[p0:p0 + 256, None, :].astype(F32) - codebook[None, :, :].astype(F32)       # [p, K, c] float32
        d = df[..., 0] * df[..., 0]
        for k in range(1, c):
            if fused:
                d = (df[..., k].astype(np.float64) * df[..., k].astype(np.float64) + d.astype(np.float64)).astype(F32)
            else:
                d = d + df[..., k] * df[..., k]
        if last_wins:
            idx[p0:p0 + 256] = d.shape[1] - 1 - np.argmin(d[:, ::-1], 1)
        else:
            idx[p0:p0 + 256] = np.argmin(d, 1)
    return idx, codebook[idx]


def u8_to_float_ref(src: np.ndarray, scale, bias, swap_rb: int, div255: int, f16: bool, pitch: int, *, swap_back=True):
    """src [..., 3] u8 -> [..., pitch]: (div255 ? v / 255 : v) * scale + bias, three float32 operations; zeros on
    [3, pitch).  Mutation hook: swap_back=False ignores swap_rb."""
    v = src.astype(F32)
    if swap_rb and swap_back:
        v = v[..., ::-1]
    t = v / F32(255.0) if div255 else v
    t = t * F32(scale) + F32(bias)
    out = np.zeros(src.shape[:-1] + (pitch,), np.float16 if f16 else np.float32)
    out[..., :3] = np_store(t, f16)
    return out


def float_to_u8_ref(src: np.ndarray, scale, bias, mode: int, swap_rb: int, *, half_up=False):
    """src [..., >= 3] float32 of the stored values -> (u8 [..., 3], t float32 [..., 3]): t = fmin(fmax(src * scale +
    bias, 0), 1) (a NaN becomes 0: fmaxf returns the other operand), q = t * 255; mode 0 rounds half to even, mode 1
    truncates.  Mutation hook: half_up (floor(q + 0.5))."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = src[..., :3].astype(F32) * F32(scale) + F32(bias)
        t = np.fmin(np.fmax(v, F32(0.0)), F32(1.0)).astype(F32)
    if swap_rb:
        t = t[..., ::-1]
    q = t * F32(255.0)
    if half_up:
        u = np.floor(q.astype(np.float64) + 0.5)
    else:
        u = np.rint(q) if mode == 0 else np.trunc(q)
    return np.clip(u, 0, 255).astype(np.uint8), np.ascontiguousarray(t)


def pad_reflect_axpy_ref(x: np.ndarray, hp: int, wp: int, mul, add: Optional[np.ndarray], add_mul, f16: bool, *,
                         symmetric=False):
    """x [n, h, w, c] float32 of the stored values -> [n, hp, wp, c]: reflect (the edge pixel is not repeated) on the
    right / bottom, x * mul (+ add_mul * add, add [n, c, hp, wp] float32): one rounding per operation.
    Mutation hook: symmetric (the edge pixel repeated)."""
    n, h, w, c = x.shape
    refl = lambda i, size: np.where(i < size, i, 2 * (size - 1) - i + (1 if symmetric else 0))
    ry, rx = refl(np.arange(hp), h), refl(np.arange(wp), w)
    v = x[:, ry][:, :, rx].astype(F32) * F32(mul)
    if add is not None:
        v = v + F32(add_mul) * add.transpose(0, 2, 3, 1).astype(F32)
    return np_store(v, f16)


def crop_ref(x: np.ndarray, h: int, w: int, c: int, pitch_out: int):
    out = np.zeros((x.shape[0], h, w, pitch_out), x.dtype)
    out[..., :c] = x[:, :h, :w, :c]
    return out


def convert_ref(x: np.ndarray, to_f16: bool):
    with np.errstate(over="ignore"):
        return x.astype(np.float16) if to_f16 else x.astype(np.float32)


def trunc_f16(x: np.ndarray) -> np.ndarray:
    """float32 -> f16 toward zero (mutation: conversion by truncation)."""
    with np.errstate(over="ignore"):
        r = x.astype(np.float16)
    over = np.abs(r.astype(np.float64)) > np.abs(x.astype(np.float64))
    return np.where(over, np.nextafter(r, np.float16(0)), r)


def f32_to_f16_inputs():
    """Every f16 value, every midpoint between neighbouring finite f16 values (ties to even) and one fp32 ulp either
    side of it, the subnormal range, the overflow threshold and NaN - as float32."""
    h = np.arange(0x10000, dtype=np.uint32).astype(np.uint16).view(np.float16)
    allh = h.astype(np.float32)
    pos = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)
    nxt = np.append(pos[1:], 65536.0)                       # past 65504: the midpoint 65520 rounds to inf
    mid = ((pos + nxt) / 2).astype(np.float32)              # exact in float32
    around = np.concatenate([mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(1e9))])
    extra = np.array([65519.996, 65520.0, 65536.0, 1e9, 2.0 ** -25, 2.0 ** -24, 2.0 ** -26, 1e-30, np.nan, np.inf], np.float32)
    a = np.concatenate([allh, around, -around, extra, -extra]).astype(np.float32)
    return np.concatenate([a, np.zeros((-a.size) % 8, np.float32)])


def bits_equal(a: np.ndarray, b: np.ndarray, nan_as_nan=False) -> bool:
    """Same shape, dtype and bit patterns (with nan_as_nan: any NaN matches any NaN)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize]
    eq = a.view(u) == b.view(u)
    if nan_as_nan and a.dtype.kind == "f":
        eq |= np.isnan(a) & np.isnan(b)
    return bool(eq.all())


def half_ties(k_values, mode_scale=255.0):
    """float32 t in [0, 1] with float32(t * 255) == k + 0.5 exactly, for every k asked for that has one (searched over
    the neighbouring float32 values of (k + 0.5) / 255), with the float32 just below and just above."""
    out = {}
    for k in k_values:
        t0 = F32((k + 0.5) / mode_scale)
        cand = [t0]
        for _ in range(4):
            cand.append(np.nextafter(cand[-1], F32(2.0)))
        lo = t0
        for _ in range(4):
            lo = np.nextafter(lo, F32(-1.0))
            cand.append(lo)
        hits = [t for t in cand if F32(t * F32(mode_scale)) == F32(k + 0.5)]
        if hits:
            t = hits[0]
            out[k] = (np.nextafter(min(hits), F32(-1.0)), t, np.nextafter(max(hits), F32(2.0)))
    return out


# ============================================================================================ kernel names
KERNEL_STEMS = ("gn_channel_sums_kernel", "gn_partials_reduce_kernel", "gn_partials_reduce4_kernel", "gn_affine_kernel",
                "affine_act_kernel", "layernorm_kernel", "u8_to_float_kernel", "float_to_u8_kernel", "bicubic_kernel",
                "vq_nearest_kernel", "pad_reflect_axpy_kernel", "crop_copy_kernel", "convert_act_kernel")


def demangle_norm_misc(sym: str) -> Optional[str]:
    """`_ZN12_GLOBAL__N_117affine_act_kernelIDF16_Lb0EEEv...` -> `affine_act_kernel<half,false>`; None for every symbol
    that is not a kernel of norm.hip / misc.hip."""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", sym)
    if not m:
        return None
    ln, pos = int(m.group(1)), m.end()
    name = sym[pos:pos + ln]
    if name not in KERNEL_STEMS:
        return None
    s = sym[pos + ln:]
    if s.startswith("E"):
        return name
    assert s.startswith("I"), f"cannot decode {sym}"
    s, args = s[1:], []
    while not s.startswith("E"):
        if s.startswith("DF16_"):
            args.append("half"); s = s[5:]
        elif s.startswith("f"):
            args.append("float"); s = s[1:]
        else:
            t = re.match(r"L([ib])(n?)(\d+)E", s)
            assert t, f"cannot decode template arguments of {sym}"
            v = int(t.group(3)) * (-1 if t.group(2) else 1)
            args.append(("true" if v else "false") if t.group(1) == "b" else str(v))
            s = s[t.end():]
    return f"{name}<{','.join(args)}>"


def norm_misc_kernel_symbols(path: str):
    return {nm for nm in (demangle_norm_misc(s) for s in elf_symbols(path)) if nm is not None}


# ============================================================================================ cases
@dataclass
class Case:
    id: str
    op: str            # gn_sums | partials | gn_affine | gn_e2e | affine_act | layernorm | bicubic
    expect: str        # the instantiation elvis_last_launch reports after the call
    dt: str = "f16"
    n: int = 1
    hw: int = 64
    c: int = 8
    pitch_extra: int = 0       # input pitch beyond pitch_for(c) (NaN-filled)
    out_extra: int = 0         # output pitch beyond pitch_for(c) (sentinel: must stay)
    coff: int = 0              # gn_sums / partials: channel slice into a wider sums buffer
    ctot_extra: int = 0
    tiles: int = 1             # partials
    misalign: bool = False     # partials: pointer off 16 bytes (on 4)
    groups: int = 1            # gn_affine / gn_e2e
    eps: float = 1e-5
    scale: bool = False
    shift: bool = False
    affine: bool = True        # gamma / beta non-null
    kind: str = "normal"       # gn_affine: normal | const | negvar ; layernorm: normal | const | offset ; affine_act: normal | sat
    mean: float = 0.0          # gn_e2e / gn_sums: mean / std of the input
    act: int = 2
    c2: int = 0                # gn_e2e: second input of the virtual concat
    inplace: bool = False
    h: int = 1                 # bicubic
    w: int = 1
    sf: int = 2
    seed: int = 0


def _k(name, dt):
    return f"{name}<{'half' if dt == 'f16' else 'float'}>"


def _build_cases():
    C_ = []
    add = lambda **kw: C_.append(Case(**kw))
    SUM = lambda dt: _k("gn_channel_sums_kernel", dt)
    # ---- GN sums.  pl_count = 256 / ceil(c / VEC); a slab is max(ceil(hw / 2048), 16 pl) pixels
    for dt, c in (("f16", 8), ("f32", 8), ("f32", 12), ("f16", 64), ("f32", 64), ("f16", 100), ("f32", 100), ("f16", 160),
                  ("f32", 160), ("f16", 320), ("f32", 320), ("f16", 640), ("f32", 640), ("f32", 1024), ("f16", 2048)):
        _, ppb, pl = gn_blocks(dt == "f16", 10 ** 4, c)      # hw small enough that ppb = 16 pl
        add(id=f"gnsum_{dt}_c{c}_ragged", op="gn_sums", expect=SUM(dt), dt=dt, c=c, hw=3 * ppb + max(pl // 2, 1) + 1,
            n=3 if c <= 100 else 1, mean=1.0)
    for dt in ("f16", "f32"):
        _, ppb, pl = gn_blocks(dt == "f16", 10 ** 4, 64)
        add(id=f"gnsum_{dt}_1px", op="gn_sums", expect=SUM(dt), dt=dt, c=64, hw=1)
        add(id=f"gnsum_{dt}_lt_pl", op="gn_sums", expect=SUM(dt), dt=dt, c=64, hw=pl - 1, n=3)
        add(id=f"gnsum_{dt}_one_slab", op="gn_sums", expect=SUM(dt), dt=dt, c=64, hw=ppb, mean=3.0)
        add(id=f"gnsum_{dt}_slab_plus1", op="gn_sums", expect=SUM(dt), dt=dt, c=64, hw=ppb + 1, n=3)
        add(id=f"gnsum_{dt}_pad_nan_slice", op="gn_sums", expect=SUM(dt), dt=dt, c=100, hw=700, n=3, pitch_extra=16,
            coff=24, ctot_extra=40, mean=30.0)
    # hw > 2048 * 16 * pl: px_per_block from the hw / 2048 branch (f32 c = 1024: cv = 256, pl = 1)
    add(id="gnsum_f32_c1024_hw_branch", op="gn_sums", expect=SUM("f32"), dt="f32", c=1024, hw=2048 * 17 + 5, mean=1.0)
    # ---- partials -> sums
    R4, R1 = "gn_partials_reduce4_kernel", "gn_partials_reduce_kernel"
    for tiles in (1, 255, 256, 257, 1000):
        add(id=f"partials_r4_t{tiles}", op="partials", expect=R4, c=64, tiles=tiles, n=3 if tiles < 1000 else 1,
            coff=8 if tiles == 257 else 0, ctot_extra=16 if tiles == 257 else 0)
        add(id=f"partials_scalar_c6_t{tiles}", op="partials", expect=R1, c=6, tiles=tiles, n=2)
        add(id=f"partials_scalar_off4_t{tiles}", op="partials", expect=R1, c=64, tiles=tiles, misalign=True)
    # ---- GN affine (exact fp64 sums in)
    AF = "gn_affine_kernel"
    combos = [(s, h) for s in (False, True) for h in (False, True)]
    for i, (s, h) in enumerate(combos):
        add(id=f"gnaff_g32_cpg5_scale{int(s)}_shift{int(h)}", op="gn_affine", expect=AF, c=160, groups=32, n=3, hw=400,
            scale=s, shift=h, eps=1e-5 if i % 2 == 0 else 1e-6)
    add(id="gnaff_g1_c20_nogamma", op="gn_affine", expect=AF, c=20, groups=1, n=2, hw=77, affine=False, scale=True, shift=True)
    add(id="gnaff_g_eq_c", op="gn_affine", expect=AF, c=100, groups=100, n=3, hw=333, eps=1e-6)   # cpg 1; n c = 300
    add(id="gnaff_g32_cpg20", op="gn_affine", expect=AF, c=640, groups=32, n=1, hw=1024, scale=True, shift=True)
    add(id="gnaff_const_var0", op="gn_affine", expect=AF, c=64, groups=32, n=2, hw=256, kind="const")
    add(id="gnaff_const_var0_eps1e-6", op="gn_affine", expect=AF, c=64, groups=32, n=2, hw=256, kind="const", eps=1e-6)
    add(id="gnaff_negvar_clamps", op="gn_affine", expect=AF, c=64, groups=32, n=2, hw=256, kind="negvar")
    # ---- GN end to end: dtype x act x mean / std
    for dt in ("f16", "f32"):
        AA = "affine_act_kernel<half,false>" if dt == "f16" else "affine_act_kernel<float,true>"
        for act in (0, 2):
            for mean in (0.0, 3.0, 30.0):
                add(id=f"gn_{dt}_act{act}_mean{int(mean)}", op="gn_e2e", expect=AA, dt=dt, c=64, groups=32, n=2,
                    hw=40 * 37, act=act, mean=mean, scale=mean == 3.0, shift=mean == 3.0)
        add(id=f"gn_{dt}_inplace", op="gn_e2e", expect=AA, dt=dt, c=160, groups=32, n=2, hw=600, inplace=True, mean=1.0)
    add(id="gn_f16_concat_64_32", op="gn_e2e", expect="affine_act_kernel<half,false>", dt="f16", c=64, c2=32, groups=32,
        hw=900, mean=1.0)
    add(id="gn_f32_concat_160_320", op="gn_e2e", expect="affine_act_kernel<float,true>", dt="f32", c=160, c2=320,
        groups=32, hw=500, mean=3.0, eps=1e-6)
    # ---- affine_act alone
    for dt, c in (("f32", 3), ("f32", 12), ("f32", 20), ("f16", 8), ("f16", 100), ("f16", 3)):
        AA = "affine_act_kernel<half,false>" if dt == "f16" else "affine_act_kernel<float,true>"
        for act in (0, 2):
            add(id=f"aa_{dt}_c{c}_act{act}", op="affine_act", expect=AA, dt=dt, c=c, n=2, hw=333, act=act,
                pitch_extra=8 if c == 12 else 0, out_extra=8 if c in (3, 100) else 0)
        add(id=f"aa_{dt}_c{c}_saturation", op="affine_act", expect=AA, dt=dt, c=c, n=1, hw=64, act=2, kind="sat")
    add(id="aa_f16_c8_inplace", op="affine_act", expect="affine_act_kernel<half,false>", dt="f16", c=8, n=2, hw=500, inplace=True)
    add(id="aa_f32_c12_inplace", op="affine_act", expect="affine_act_kernel<float,true>", dt="f32", c=12, n=2, hw=500, inplace=True)
    # total_vec > 256 * 32 * 256: the grid-stride loop iterates
    add(id="aa_f16_c8_grid_stride", op="affine_act", expect="affine_act_kernel<half,false>", dt="f16", c=8, n=1,
        hw=256 * 32 * 256 + 1000)
    # ---- LayerNorm
    for dt, cs in (("f16", (8, 64, 96, 128, 192, 256, 512)), ("f32", (4, 12, 64, 192, 256))):
        LN = _k("layernorm_kernel", dt)
        for c in cs:
            tpw = 64 // ln_lpt(c, dt == "f16")
            for tokens in sorted({1, max(tpw - 1, 1), tpw + 1, 4 * tpw * 3 + 2}):
                add(id=f"ln_{dt}_c{c}_t{tokens}", op="layernorm", expect=LN, dt=dt, c=c, hw=tokens,
                    pitch_extra=8 if c in (96, 12) else 0, out_extra=16 if c in (96, 12, 4) else 0)
        add(id=f"ln_{dt}_const", op="layernorm", expect=LN, dt=dt, c=64, hw=50, kind="const")
        add(id=f"ln_{dt}_mean100", op="layernorm", expect=LN, dt=dt, c=192, hw=70, kind="offset")
        add(id=f"ln_{dt}_inplace", op="layernorm", expect=LN, dt=dt, c=192 if dt == "f16" else 12, hw=333, inplace=True)
    # tokens > 256 * 16 * 4 * tpw: the wave loop iterates (f32 c = 256: lpt = 64, tpw = 1)
    add(id="ln_f32_c256_wave_loop", op="layernorm", expect=_k("layernorm_kernel", "f32"), dt="f32", c=256,
        hw=256 * 16 * 4 + 77)
    add(id="ln_f16_c64_wave_loop", op="layernorm", expect=_k("layernorm_kernel", "f16"), dt="f16", c=64,
        hw=256 * 16 * 4 * 8 + 77)
    # ---- bicubic
    i = 0
    for dt in ("f16", "f32"):
        BC = _k("bicubic_kernel", dt)
        for sf in (1, 2, 3, 4):
            for (h, w) in ((1, 1), (2, 3), (3, 2), (1, 13), (13, 17)):
                c = (1, 3, 4, 8)[i % 4]
                i += 1
                add(id=f"bicubic_{dt}_x{sf}_{h}x{w}_c{c}", op="bicubic", expect=BC, dt=dt, sf=sf, h=h, w=w, c=c,
                    n=2 if (h, w) != (13, 17) else 1, pitch_extra=8 if c == 4 else 0)
    for j, c in enumerate(C_):
        c.seed = j
    return C_


CASES = _build_cases()

# the exact-equality tests of tests/test_gpu_norm_misc_matrix.py reach these (asserted there through elvis_last_launch)
EXACT_KERNELS = {f"{k}<{t}>" for k in ("u8_to_float_kernel", "float_to_u8_kernel", "vq_nearest_kernel",
                                       "pad_reflect_axpy_kernel", "crop_copy_kernel") for t in ("half", "float")} | {
    "convert_act_kernel<half,float>", "convert_act_kernel<float,half>"}
