"""References and the case matrix for the twelve kernels of csrc/glue.hip (importable without a GPU:
tests/test_gpu_glue_matrix.py runs the cases through the C ABI, tests/test_glue_ledger.py checks the ledger, the pins
against oracle.glue_ref and the goldens, and the discrimination of the inputs on the CPU).

The references are plain numpy, written from the contracts in include/elvis_amd.h and the comments of glue.hip:

  exact    recompose (+ the clamped map), area downscale, blend, per-level select, tile accumulate / normalise, SSE:
           integer arithmetic, or numpy float32 with one IEEE operation per step where the contract is "numpy's float32
           evaluation order".  Compared bit for bit.
  bounded  per-block SSIM: float64, with a per-block bound derived below (ssim_ref).

Keyword arguments named `mutant` exist for the discrimination test only: each builds a plausible wrong kernel."""
from __future__ import annotations

import functools
import re
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from _convref import elf_symbols

F32, F64, I64 = np.float32, np.float64, np.int64
U24 = 2.0 ** -24
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
ROUND_CV2, ROUND_HALF_UP = 0, 1

# the grid caps of the launch code, in units of what one lane handles: above them a grid-stride loop iterates
CAP_RECOMPOSE_BYTES = 256 * 16 * 256 * 16      # 4096 workgroups x 256 lanes x 16 bytes = 16 MiB
CAP_BLEND_BYTES = 8192 * 256 * 16              # blend and select: 32 MiB
CAP_AREA_OUTPUTS = 8192 * 256                  # generic: output elements; c3/f4: output pixels
CAP_NORMALIZE_PIXELS = 8192 * 256


# ============================================================================================ recompose
def _block_index(size: int, block: int, cells: int):
    """(index of the block of every coordinate, clipped into the map; whether the coordinate is inside the map)."""
    i = np.arange(size) // block
    return np.minimum(i, cells - 1), i < cells


def recompose_ref(a, b, m, block: int, thr: int, *, mutant: Optional[str] = None):
    """a, b [n, h, w, c] u8, m [n, by, bx] int32 -> block (i, j) of frame f from a where m[f, i, j] <= thr, else from b;
    pixels outside the by*block x bx*block grid take b.  Mutants: `strict` (<), `trailing_a`."""
    n, h, w, _ = a.shape
    yi, yin = _block_index(h, block, m.shape[1])
    xi, xin = _block_index(w, block, m.shape[2])
    pred = (m.astype(I64) < thr) if mutant == "strict" else (m.astype(I64) <= thr)
    inside = yin[:, None] & xin[None, :]
    take = pred[:, yi][:, :, xi] & inside[None]
    if mutant == "trailing_a":
        take = take | ~inside[None]
    return np.where(take[..., None], a, b)


def clamp_map_ref(m, thr: int, clamp_to: int, *, mutant: Optional[str] = None):
    """map_out = (map <= thr) ? map : clamp_to.  Mutant: `no_clamp`."""
    if mutant == "no_clamp":
        return m.copy()
    return np.where(m.astype(I64) <= thr, m, np.int32(clamp_to)).astype(np.int32)


def recompose_path(n, h, w, c, block) -> str:
    """The dispatch of elvis_recompose_u8 restated."""
    if (w * c) % 16 == 0 and block * c >= 16:
        return "recompose_rows_u8_kernel"
    return "recompose_u8_kernel<true>" if block & (block - 1) == 0 else "recompose_u8_kernel<false>"


# ============================================================================================ area downscale
def area_ref(x, f: int, rounding: int, *, mutant: Optional[str] = None):
    """x [n, h, w, c] u8 -> box mean over f x f, in integers.  ROUND_HALF_UP and every f == 2: (s + area/2) // area.
    ROUND_CV2 otherwise: the float32 product s * (1 / area) rounded half to even - for f a power of two the product is
    exact, for odd areas no sum is a tie and the nearest fraction (1 / (2 area) >= 0.01 from .5) is far beyond the
    float32 error of the product, so the exact quotient rounded half to even is the same number.
    Mutants: `half_up` (every f), `half_even` (every f, f == 2 included)."""
    n, h, w, c = x.shape
    s = x.reshape(n, h // f, f, w // f, f, c).astype(I64).sum((2, 4))
    area = f * f
    up = (s + area // 2) // area
    q, r = np.divmod(s, area)
    even = q + (2 * r > area) + ((2 * r == area) & (q & 1 == 1))
    if mutant == "half_up":
        v = up
    elif mutant == "half_even":
        v = even
    else:
        v = up if (rounding == ROUND_HALF_UP or f == 2) else even
    return np.minimum(v, 255).astype(np.uint8)


def area_ref_u16(x, f: int, rounding: int):
    """area_ref for the large frame: the sum as f*f strided uint16 slices (255 f^2 <= 65535 for f <= 16)."""
    s = np.zeros((x.shape[0], x.shape[1] // f, x.shape[2] // f, x.shape[3]), np.uint16)
    for dy in range(f):
        for dx in range(f):
            s += x[:, dy::f, dx::f]
    area = f * f
    s = s.astype(np.uint32)
    if rounding == ROUND_HALF_UP or f == 2:
        return ((s + area // 2) // area).astype(np.uint8)
    q, r = np.divmod(s, area)
    return (q + (2 * r > area) + ((2 * r == area) & (q & 1 == 1))).astype(np.uint8)


def area_path(c, f, w, offset) -> str:
    return "area_downscale4_c3_kernel" if (c == 3 and f == 4 and (w * 3) % 4 == 0 and offset % 4 == 0) \
        else "area_downscale_u8_kernel"


def every_sum_image(f: int, c: int, seed: int = 0):
    """[1, ho f, wo f, c] u8 whose output blocks, in raster order, sum to k = 0 .. 255 f^2 (then wrap), channel ch
    shifted by 97 ch: every remainder of the division - every tie, every saturation point - occurs in every channel.
    The k of a block is spread as base = k // f^2 everywhere and + 1 on k % f^2 positions chosen by a seeded shuffle."""
    K = 255 * f * f + 1
    wo = 53 if f == 4 else 56 if f == 3 else 32
    ho = -(-K // wo)
    rng = np.random.default_rng(seed)
    k = (np.arange(ho * wo)[:, None] + 97 * np.arange(c)[None, :]) % K              # [blocks, c]
    base, rem = k // (f * f), k % (f * f)
    order = rng.permuted(np.tile(np.arange(f * f), (ho * wo, c, 1)), axis=2)        # a shuffle per block and channel
    px = base[..., None] + (order < rem[..., None])                                 # [blocks, c, f*f]
    img = px.reshape(ho, wo, c, f, f).transpose(0, 3, 1, 4, 2).reshape(1, ho * f, wo * f, c)
    assert img.max() <= 255
    return img.astype(np.uint8)


# ============================================================================================ blend
def blend_ref(o, r, m, block: int, alpha: float, *, mutant: Optional[str] = None):
    """o, r [n, h, w, c] u8, m [n, h // block, w // block] int32 -> trunc(clip(o (1 - a mask) + r (a mask), 0, 255)) in
    numpy float32, one rounding per operation; mask = (m > 0) at map row floor(y by / h), column floor(x bx / w) (the
    nearest-neighbour resize of the map to the frame).  Mutants: `y_div_block` (y // block), `round`."""
    n, h, w, _ = o.shape
    by, bx = m.shape[1:]
    if mutant == "y_div_block":
        ys, xs = np.minimum(np.arange(h) // block, by - 1), np.minimum(np.arange(w) // block, bx - 1)
    else:
        ys, xs = np.minimum(np.arange(h) * by // h, by - 1), np.minimum(np.arange(w) * bx // w, bx - 1)
    mask = (m[:, ys][:, :, xs] > 0).astype(F32)[..., None]
    w_rest = mask * F32(alpha)
    w_orig = F32(1.0) - w_rest
    v = o.astype(F32) * w_orig + r.astype(F32) * w_rest
    v = np.clip(v, F32(0.0), F32(255.0))
    if mutant == "round":
        v = np.rint(v)
    return v.astype(np.uint8)


# ============================================================================================ select
def select_ref(versions, slot_of_level, m, block: int):
    """versions: list of [n, h, w, c] u8; slot_of_level int32 [n_levels]; m [n, h // block, w // block] int32 ->
    block (i, j) of frame f from versions[slot_of_level[m[f, i, j]]]; 0 where the level is outside [0, n_levels), where
    its slot is negative, and outside the floored grid."""
    n, h, w, _ = versions[0].shape
    yi, yin = _block_index(h, block, m.shape[1])
    xi, xin = _block_index(w, block, m.shape[2])
    lvl = m.astype(I64)
    ok = (lvl >= 0) & (lvl < len(slot_of_level))
    slot = np.where(ok, np.asarray(slot_of_level, I64)[np.clip(lvl, 0, len(slot_of_level) - 1)], -1)
    slot = np.where((yin[:, None] & xin[None, :])[None], slot[:, yi][:, :, xi], -1)            # [n, h, w]
    out = np.zeros_like(versions[0])
    for s, v in enumerate(versions):
        out[slot == s] = v[slot == s]
    return out


# ============================================================================================ tile accumulate / normalise
def tile_accumulate_ref(acc, wsum, tile, wy, wx, wx2, y0: int, x0: int, temporal_weight: float, *,
                        mutant: Optional[str] = None):
    """In place on acc [h, w, c] / wsum [h, w] float32; tile [th, tw, c] u8, wy [th] float32, wx / wx2 [tw] float64:
    sw = f32(f64(f32(f64(wy) wx)) wx2); wgt = sw * f32(temporal_weight); acc += f32(tile) * wgt; wsum += wgt - numpy's
    own evaluation of a float32 weight image multiplied in place by two float64 ramps.
    Mutant: `single_rounding` (wy wx wx2 in float64, rounded once)."""
    th, tw, _ = tile.shape
    if mutant == "single_rounding":
        sw = (wy.astype(F64)[:, None] * wx[None, :] * wx2[None, :]).astype(F32)
    else:
        sw = (wy.astype(F64)[:, None] * wx[None, :]).astype(F32)
        sw = (sw.astype(F64) * wx2[None, :]).astype(F32)
    wgt = sw * F32(temporal_weight)
    acc[y0:y0 + th, x0:x0 + tw] += tile.astype(F32) * wgt[..., None]
    wsum[y0:y0 + th, x0:x0 + tw] += wgt


def tile_normalize_ref(acc, wsum, *, mutant: Optional[str] = None):
    """acc [h, w, c], wsum [h, w] float32 -> trunc(clip(acc / (wsum > 0 ? wsum : 1), 0, 255)) u8, float32 division.
    No NaN inputs (numpy leaves their cast undefined).  Mutants: `round`, `wsum_ge_0` (a zero weight divides)."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        safe = np.where((wsum >= 0) if mutant == "wsum_ge_0" else (wsum > 0), wsum, F32(1.0)).astype(F32)
        v = acc / safe[..., None]
        v = np.where(np.isnan(v), F32(0.0), np.clip(v, F32(0.0), F32(255.0)))
    if mutant == "round":
        v = np.rint(v)
    return v.astype(np.uint8)


# ============================================================================================ SSE
def sse_ref(a, b, mask=None, *, mutant: Optional[str] = None):
    """a, b [n, h, w, c] u8, mask [n, h, w] u8 or None -> (sum of squared differences, number of compared elements)
    per frame, int64: every channel of the pixels whose mask is non-zero.  Mutant: `mask_by_byte` (the mask indexed by
    the element, not by the pixel; wrapped into the frame's mask)."""
    n, h, w, c = a.shape
    d = a.astype(I64) - b.astype(I64)
    sq = (d * d).reshape(n, h * w * c)
    if mask is None:
        return sq.sum(1), np.full(n, h * w * c, I64)
    use = mask.reshape(n, h * w) != 0
    idx = np.arange(h * w * c)
    use = use[:, idx % (h * w)] if mutant == "mask_by_byte" else use[:, idx // c]
    return (sq * use).sum(1), use.sum(1).astype(I64)


# ============================================================================================ per-block SSIM
def ssim_window(sigma: float = 1.5, normalise: bool = True):
    """The 11-tap Gaussian of pytorch_msssim in float32 (coordinates, exponent and normalisation in float32)."""
    coords = np.arange(11, dtype=F32) - 5
    g = np.exp(-(coords ** 2) / F32(2 * sigma ** 2)).astype(F32)
    return (g / g.sum()).astype(F32) if normalise else g


def _blocks(x, b):
    """[n, h, w, c] -> [n, by, bx, c, b, b] over the floored grid."""
    n, h, w, c = x.shape
    by, bx = h // b, w // b
    return x[:, :by * b, :bx * b].reshape(n, by, b, bx, b, c).transpose(0, 1, 3, 5, 2, 4)


def _hulp(v):
    """Half a float32 ulp at magnitude v >= 0 (float64 array): what one correctly rounded float32 operation whose exact
    result has that magnitude can be off by.  v is inflated by 2^-18 so that a result the kernel's own earlier errors
    moved across a power of two is covered; 0 stays 0 (an exact zero is computed exactly from exact zeros)."""
    v = np.asarray(v, F64)
    e = np.frexp(v * (1 + 2.0 ** -18))[1]
    return np.where(v > 0, np.ldexp(1.0, e - 25), 0.0)


def _chain(terms, dterms):
    """A left-to-right float32 sum of products along the last axis, as the kernel forms it (acc = 0; acc += w * x):
    terms = w x (float64, >= 0 here), dterms = w dx, what the factors x are already off by.  Returns (sum, bound):
    every product rounds once, every add after the first rounds once, each by half an ulp at the magnitude of its own
    result - the reference's partial sums (all terms are >= 0, so they only grow)."""
    s = terms.sum(-1)
    e = dterms.sum(-1) + _hulp(terms + dterms).sum(-1)
    partial = np.cumsum(terms + dterms, -1)[..., 1:]
    return s, e + _hulp(partial).sum(-1)


def _smooth(x, dx, win, m):
    """x, dx [..., b, b] -> the 'valid' separable window sums [..., m, m] and their bound; the kernel's order: for every
    output, rows first (dx inner), then the column of the 11 row sums."""
    k = win.shape[0]
    idx = np.arange(m)[:, None] + np.arange(k)[None, :]                  # [m, k]
    r = x[..., :, idx]                                                   # [..., b, m, k]
    rs, re = _chain(r * win, dx[..., :, idx] * win)                      # [..., b, m]
    c_ = np.swapaxes(rs, -1, -2)[..., :, idx]                            # [..., m(x), m(y), k]
    ce = np.swapaxes(re, -1, -2)[..., :, idx]
    s, e = _chain(c_ * win, ce * win)
    return np.swapaxes(s, -1, -2), np.swapaxes(e, -1, -2)


def ssim_ref(a, b, bs: int, *, win=None, C1: float = 0.01 ** 2, C2: float = 0.03 ** 2, smooth_from: int = 11,
             channel_mean: bool = True):
    """a, b [n, h, w, c] u8 -> (ssim [n, h // bs, w // bs] float64, bound of |kernel - ssim| per block, float64).

    The operation: pytorch_msssim.ssim of every bs x bs block at data_range 1 - local moments by the separable 11-tap
    window ('valid'; skipped when bs < 11: the moments are the pixels' own), s1 = E[xx] - mu1^2 etc.,
    cs = (2 s12 + C2) / (s1 + s2 + C2), l = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1), mean of l cs over the map, then over
    the channels.  The window is the float32 one the kernel is handed (exact in float64).

    The bound follows block_ssim_kernel operation by operation (float32, no fused operations: the library is built
    without contraction), from the reference's values and the inputs only.  Every float32 operation is correctly
    rounded: it is off by at most H(r) = half an ulp at the magnitude of its result r (_hulp; r is the reference's value
    plus the bound gathered so far).  With dx what a quantity x is already off by:
      u = p / 255                      du = H(u)
      uu, vv, uv                       d(uv) = u dv + v du + du dv + H(uv)
      the 11 + 11 term chains          _chain: H of every product w x and of every partial sum after the first (all
                                       terms >= 0, so the reference's partial sums are the magnitudes); rows first,
                                       then the column of the row sums, as the kernel loops
      mu1 mu1, mu1 mu2, mu2 mu2        as the products above
      s = E - mu mu                    ds = dE + d(mu mu) + H(s)
      2 s12 + C2, s1 + s2 + C2         the doubling is exact; C1, C2 are float products of rounded constants (3 U24 C);
                                       H of every add
      cs = N / D                       (dN + |cs| dD) / (D - dD) + H(cs), likewise l
      l cs, the mean over the map      the product as above; m^2 sequential adds (y outer, x inner): H of every partial
                                       sum of |l cs|; H of the division by m^2
      the channel sum and / c          H of every partial sum and of the quotient
    For bs < 11 the kernel's xx and mu1 mu1 are the SAME float32 product of the same operands (likewise xy and mu1 mu2),
    so s1 = s2 = s12 = 0 and cs = C2 / C2 = 1 hold exactly, whatever u rounds to: ds = dcs = 0 there.
    Where s1 + s2 is small against C2 = 9e-4 the bound is large by construction (dE of a few 1e-7 on moments near 1,
    divided by D ~ 1e-3): that is the kernel's own sensitivity on flat blocks, not slack.
    Mutation hooks: win, C2, smooth_from, channel_mean."""
    win = ssim_window() if win is None else win
    win = win.astype(F64)
    n, h, w, c = a.shape
    smooth = bs >= smooth_from
    k = min(win.shape[0], bs)
    m = bs - k + 1 if smooth else bs
    x, y = _blocks(a, bs).astype(F64) / 255.0, _blocks(b, bs).astype(F64) / 255.0
    dx, dy = _hulp(x), _hulp(y)
    prod = lambda p, q, dp, dq: (p * q, p * dq + q * dp + dp * dq + _hulp(np.abs(p * q) + p * dq + q * dp + dp * dq))
    xx, dxx = prod(x, x, dx, dx)
    yy, dyy = prod(y, y, dy, dy)
    xy, dxy = prod(x, y, dx, dy)
    if smooth:
        wk = win[:k]
        mu1, dmu1 = _smooth(x, dx, wk, m)
        mu2, dmu2 = _smooth(y, dy, wk, m)
        xx, dxx = _smooth(xx, dxx, wk, m)
        yy, dyy = _smooth(yy, dyy, wk, m)
        xy, dxy = _smooth(xy, dxy, wk, m)
    else:
        mu1, dmu1, mu2, dmu2 = x, dx, y, dy
    m11, dm11 = prod(mu1, mu1, dmu1, dmu1)
    m22, dm22 = prod(mu2, mu2, dmu2, dmu2)
    m12, dm12 = prod(mu1, mu2, dmu1, dmu2)
    sub = lambda E, dE, M, dM: (E - M, dE + dM + _hulp(np.abs(E - M) + dE + dM))
    if smooth:
        s1, ds1 = sub(xx, dxx, m11, dm11)
        s2, ds2 = sub(yy, dyy, m22, dm22)
        s12, ds12 = sub(xy, dxy, m12, dm12)
    else:
        s1 = s2 = s12 = ds1 = ds2 = ds12 = np.zeros_like(mu1)
    dC1, dC2 = 3 * U24 * C1, 3 * U24 * C2
    add = lambda p, dp, q, dq: (p + q, dp + dq + _hulp(np.abs(p + q) + dp + dq))

    def div(N, dN, D, dD):
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(D - dD > 0, (dN + np.abs(N / D) * dD) / (D - dD), np.inf)      # inf: nothing can be promised
        return N / D, e + _hulp(np.abs(N / D) + e)

    N, dN = add(2 * s12, 2 * ds12, C2, dC2)
    D, dD = add(*add(s1, ds1, s2, ds2), C2, dC2)
    if smooth:
        cs, dcs = div(N, dN, D, dD)
    else:
        cs, dcs = N / D, np.zeros_like(N)            # C2 / C2 == 1 exactly
    Nl, dNl = add(2 * m12, 2 * dm12, C1, dC1)
    Dl, dDl = add(*add(m11, dm11, m22, dm22), C1, dC1)
    l, dl = div(Nl, dNl, Dl, dDl)
    p = l * cs
    dp = np.abs(l) * dcs + np.abs(cs) * dl + dl * dcs
    dp = dp + _hulp(np.abs(p) + dp)
    mm = m * m
    flat = lambda t: t.reshape(t.shape[:-2] + (mm,))                                 # the kernel's order: y outer, x inner
    ch = p.sum((-1, -2)) / mm                                                        # [n, by, bx, c]
    dsum = dp.sum((-1, -2)) + _hulp(np.cumsum(flat(np.abs(p) + dp), -1)[..., 1:]).sum(-1)
    dch = dsum / mm
    dch = dch + _hulp(np.abs(ch) + dch)
    out = ch.sum(-1) / (c if channel_mean else 1)
    dout = dch.sum(-1) + _hulp(np.cumsum(np.abs(ch) + dch, -1)[..., 1:]).sum(-1)
    dout = dout / c
    dout = dout + _hulp(np.abs(ch.sum(-1) / c) + dout)
    return out, dout + 1e-300


def ssim_f32_restatement(a, b, bs: int, win=None):
    """block_ssim_kernel's evaluation order in numpy float32, operation by operation (vectorised over the blocks, the
    channels and the map; the loops are the kernel's sequential ones).  Keeps the bound honest on the CPU: it must stay
    inside ssim_ref's bound on every case, and not far inside on all of them."""
    win = (ssim_window() if win is None else win).astype(F32)
    n, h, w, c = a.shape
    smooth = bs >= 11
    m = bs - 10 if smooth else bs
    u = _blocks(a, bs).astype(F32) / F32(255.0)
    v = _blocks(b, bs).astype(F32) / F32(255.0)
    C1, C2 = F32(0.01) * F32(0.01), F32(0.03) * F32(0.03)
    if not smooth:
        mu1, mu2, xx, yy, xy = u, v, u * u, v * v, u * v
    else:
        z = lambda: np.zeros(u.shape[:-2] + (m, m), F32)
        mu1, mu2, xx, yy, xy = z(), z(), z(), z(), z()
        for dy in range(11):
            r1, r2, rxx, ryy, rxy = z(), z(), z(), z(), z()
            for dx in range(11):
                uu, vv = u[..., dy:dy + m, dx:dx + m], v[..., dy:dy + m, dx:dx + m]
                r1 = r1 + win[dx] * uu
                r2 = r2 + win[dx] * vv
                rxx = rxx + win[dx] * (uu * uu)
                ryy = ryy + win[dx] * (vv * vv)
                rxy = rxy + win[dx] * (uu * vv)
            mu1 = mu1 + win[dy] * r1
            mu2 = mu2 + win[dy] * r2
            xx = xx + win[dy] * rxx
            yy = yy + win[dy] * ryy
            xy = xy + win[dy] * rxy
    s1, s2, s12 = xx - mu1 * mu1, yy - mu2 * mu2, xy - mu1 * mu2
    cs = (F32(2.0) * s12 + C2) / (s1 + s2 + C2)
    t = ((F32(2.0) * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs
    acc = np.zeros(t.shape[:-2], F32)
    for yy_ in range(m):
        for xx_ in range(m):
            acc = acc + t[..., yy_, xx_]
    chv = acc / F32(m * m)
    tot = np.zeros(chv.shape[:-1], F32)
    for ch in range(c):
        tot = tot + chv[..., ch]
    out = tot / F32(c)
    assert out.dtype == F32
    return out


SSIM_CONTENT = ("noise", "noise_near", "identical", "black", "black_white", "inverse", "ramp", "bright_flat")


def ssim_pair(content: str, n, h, w, c, seed: int):
    rng = np.random.default_rng(seed)
    shape = (n, h, w, c)
    if content == "noise":          # two independent uniform-noise images: large variance, SSIM near 0
        return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)
    if content == "noise_near":     # the pair of tests/test_gpu_metrics.py: uniform noise, one image moved by up to 12
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        return a, np.clip(a.astype(int) + rng.integers(-12, 13, shape), 0, 255).astype(np.uint8)
    if content == "identical":
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        return a, a.copy()
    if content == "black":
        return np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    if content == "black_white":
        return np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)
    if content == "inverse":
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        return a, (255 - a).astype(np.uint8)
    if content == "ramp":
        a = np.broadcast_to(((np.arange(w) * 255) // max(w - 1, 1)).astype(np.uint8)[None, None, :, None], shape).copy()
        return a, np.clip(a.astype(int) + 3, 0, 255).astype(np.uint8)
    if content == "bright_flat":    # 250 .. 252, one image one lower on a sparse lattice: s1 + s2 << C2
        a = rng.integers(250, 253, shape, dtype=np.uint8)
        b = a.copy()
        b[:, ::3, ::4] -= 1
        return a, b
    raise ValueError(content)


# ============================================================================================ kernel names
def kernel_stems(source_path: str):
    """The __global__ functions of a .hip source file, from its text."""
    text = open(source_path).read()
    return set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", text))


def demangle_kernel(sym: str, stems) -> Optional[str]:
    """`_Z19recompose_u8_kernelILb1EEvPKh...` -> `recompose_u8_kernel<true>`, `_Z15blend_u8_kernelPKh...` ->
    `blend_u8_kernel`, `_ZN12_GLOBAL__N_120stretch_index_kernelEPKhPiiiiii` (a kernel of an unnamed namespace) ->
    `stretch_index_kernel`; None for everything that is not one of `stems` (the host stubs included)."""
    t = re.match(r"_Z(?:N12_GLOBAL__N_1)?(\d+)", sym)
    if not t:
        return None
    ln, pos = int(t.group(1)), t.end()
    name, rest = sym[pos:pos + ln], sym[pos + ln:]
    if name not in stems:
        return None
    b = re.match(r"ILb([01])EE", rest)
    return f"{name}<{'true' if b.group(1) == '1' else 'false'}>" if b else name


def kernel_symbols(lib_path: str, source_path: str):
    """The kernels of one source file that the built library holds."""
    stems = kernel_stems(source_path)
    return {nm for nm in (demangle_kernel(s, stems) for s in elf_symbols(lib_path)) if nm is not None}


glue_kernel_stems, demangle_glue, glue_kernel_symbols = kernel_stems, demangle_kernel, kernel_symbols


# ============================================================================================ cases
@dataclass
class Case:
    id: str
    op: str                        # recompose | area | blend | select | accumulate | normalize | sse | ssim
    expect: str                    # what elvis_last_launch reports after the call
    shape: Tuple[int, int, int, int] = (1, 1, 1, 1)      # n, h, w, c
    block: int = 1
    grid: Optional[Tuple[int, int]] = None               # recompose: (by, bx) of the map when not the floored grid
    thr: int = 0
    clamp_to: Optional[int] = None                       # recompose: map_out present with this value
    kind: str = ""                                       # the inputs' recipe (see the builders)
    factor: int = 1
    rounding: int = 0
    offset: int = 0                                      # area: byte offset of src into its allocation; select: of version 1
    alpha: float = 1.0
    versions: int = 1
    slots: Tuple[int, ...] = ()
    tiles: Tuple[Tuple[int, int, int, int, float], ...] = ()   # accumulate: (y0, x0, th, tw, temporal_weight) in sequence
    mask: str = ""                                       # sse: "" | zero | full | random
    big: bool = False                                    # over a grid cap: the only large cases
    seed: int = 0


def _recompose_cases(add):
    shapes = [  # (n, h, w, c, block, grid)
        (2, 16, 32, 3, 6, None), (1, 8, 16, 1, 16, (1, 1)), (1, 16, 64, 1, 16, None), (1, 9, 16, 4, 4, None),
        (2, 24, 48, 3, 8, None), (1, 32, 48, 3, 8, (3, 4)), (1, 20, 32, 2, 9, None),
        (1, 17, 13, 1, 4, None), (2, 30, 50, 3, 8, None), (1, 8, 16, 1, 8, None), (1, 6, 10, 2, 2, None),
        (1, 21, 25, 3, 5, None), (2, 14, 10, 1, 3, None), (1, 12, 16, 1, 6, None), (1, 21, 25, 3, 5, (3, 4))]
    for n, h, w, c, blk, grid in shapes:
        path = recompose_path(n, h, w, c, blk)
        tag = f"{n}x{h}x{w}x{c}_b{blk}" + (f"_map{grid[0]}x{grid[1]}" if grid else "")
        for kind, thr, clamp_to in (("some", 1, -7), ("all", INT32_MAX, None), ("none", -4, 9)):
            add(id=f"recompose_{tag}_{kind}", op="recompose", expect=path, shape=(n, h, w, c), block=blk, grid=grid,
                thr=thr, clamp_to=clamp_to, kind=kind)
    for (n, h, w, c, blk) in ((3, 1080, 1920, 3, 8), (3, 1080, 1918, 3, 8), (3, 1080, 1918, 3, 6)):
        add(id=f"recompose_over_cap_{n}x{h}x{w}x{c}_b{blk}", op="recompose", expect=recompose_path(n, h, w, c, blk),
            shape=(n, h, w, c), block=blk, thr=1, clamp_to=-7, kind="some", big=True)


def _area_cases(add):
    for c in (1, 2, 3, 4):
        for f in (1, 2, 3, 4, 5, 7, 8, 16):
            for rounding in (ROUND_CV2, ROUND_HALF_UP):
                for n in (1, 3):
                    ho, wo = (5, 7) if n == 1 else (3, 9)
                    add(id=f"area_c{c}_f{f}_r{rounding}_n{n}", op="area", expect=area_path(c, f, wo * f, 0),
                        shape=(n, ho * f, wo * f, c), factor=f, rounding=rounding, kind="random")
    for f in (2, 3, 4):
        for c in (1, 3):
            for rounding in (ROUND_CV2, ROUND_HALF_UP):
                shp = every_sum_shape(f, c)
                add(id=f"area_every_sum_f{f}_c{c}_r{rounding}", op="area", expect=area_path(c, f, shp[2], 0), shape=shp,
                    factor=f, rounding=rounding, kind="every_sum")
    for off in (0, 1, 2, 3):          # c3 / f4 from an aligned pointer and from the three misaligned ones: same image
        for rounding in (ROUND_CV2, ROUND_HALF_UP):
            add(id=f"area_c3_f4_offset{off}_r{rounding}", op="area", expect=area_path(3, 4, 212, off),
                shape=every_sum_shape(4, 3), factor=4, rounding=rounding, kind="every_sum", offset=off)
    add(id="area_over_cap_generic_2x1080x1920x3_f2", op="area", expect="area_downscale_u8_kernel", shape=(2, 1080, 1920, 3),
        factor=2, rounding=ROUND_CV2, kind="random", big=True)
    add(id="area_over_cap_c3f4_1x5800x5800x3", op="area", expect="area_downscale4_c3_kernel", shape=(1, 5800, 5800, 3),
        factor=4, rounding=ROUND_CV2, kind="random", big=True)


def every_sum_shape(f, c):
    K = 255 * f * f + 1
    wo = 53 if f == 4 else 56 if f == 3 else 32
    return (1, -(-K // wo) * f, wo * f, c)


ALPHAS = (0.0, 1.0 / 3.0, 0.35, 0.5, 0.999, 1.0, 1.5, -0.25)


def _blend_cases(add):
    for i, alpha in enumerate(ALPHAS):
        add(id=f"blend_pairs_a{i}", op="blend", expect="blend_u8_kernel", shape=(1, 256, 256, 1), block=8, alpha=alpha,
            kind="pairs")
        add(id=f"blend_pairs_all_positive_a{i}", op="blend", expect="blend_u8_kernel", shape=(1, 256, 256, 1), block=8,
            alpha=alpha, kind="pairs_positive")
        for shp, blk in (((1, 36, 52, 3), 8), ((2, 9, 7, 3), 2), ((1, 9, 7, 3), 2)):
            add(id=f"blend_{'x'.join(map(str, shp))}_b{blk}_a{i}", op="blend", expect="blend_u8_kernel", shape=shp, block=blk,
                alpha=alpha, kind="random")
    add(id="blend_over_cap_6x1080x1920x3", op="blend", expect="blend_u8_kernel", shape=(6, 1080, 1920, 3), block=8,
        alpha=0.35, kind="random", big=True)


def _select_cases(add):
    S = "select_levels_u8_kernel"
    add(id="select_2x19x29x3_b3_v3", op="select", expect=S, shape=(2, 19, 29, 3), block=3, versions=3, slots=(0, -1, 1, 2, -1))
    add(id="select_1x36x52x3_b8_v4", op="select", expect=S, shape=(1, 36, 52, 3), block=8, versions=4, slots=(3, 2, 1, 0))
    add(id="select_1x17x13x1_b3_v1", op="select", expect=S, shape=(1, 17, 13, 1), block=3, versions=1, slots=(-1, 0, 0))
    add(id="select_2x16x24x1_b8_v2", op="select", expect=S, shape=(2, 16, 24, 1), block=8, versions=2, slots=(1, 0, 1))
    add(id="select_1x44x60x3_b8_v2_offset1", op="select", expect=S, shape=(1, 44, 60, 3), block=8, versions=2,
        slots=(0, 1), offset=1)
    add(id="select_over_cap_6x1080x1920x3", op="select", expect=S, shape=(6, 1080, 1920, 3), block=8, versions=2,
        slots=(1, -1, 0), big=True)


def _tile_cases(add):
    A, N = "tile_accumulate_kernel", "tile_normalize_kernel"
    H, W = 40, 56
    spots = {"top_left": (0, 0, 13, 19), "top_right": (0, W - 19, 13, 19), "bottom_left": (H - 13, 0, 13, 19),
             "bottom_right": (H - 13, W - 19, 13, 19), "interior": (11, 17, 16, 16), "interior_3wg": (5, 9, 23, 29),
             "whole": (0, 0, H, W)}
    for c in (1, 3):
        for i, (name, (y0, x0, th, tw)) in enumerate(spots.items()):
            add(id=f"accumulate_c{c}_{name}", op="accumulate", expect=A, shape=(1, H, W, c),
                tiles=((y0, x0, th, tw, (1.0, 0.5, 0.3)[(i + c) % 3]),))
        add(id=f"accumulate_c{c}_two_overlapping", op="accumulate", expect=A, shape=(1, H, W, c),
            tiles=((3, 5, 20, 30, 0.5), (15, 25, 21, 31, 0.3)))
    for c in (1, 3, 4):
        add(id=f"normalize_c{c}_edges", op="normalize", expect=N, shape=(1, 0, 0, c), kind="edges")
        add(id=f"normalize_c{c}_random", op="normalize", expect=N, shape=(1, 17, 23, c), kind="random")
    add(id="normalize_over_cap_1100x1920x3", op="normalize", expect=N, shape=(1, 1100, 1920, 3), kind="random", big=True)


def _sse_cases(add):
    S = "sse_u8_kernel"
    frames = {1: (1, 1, 1), 63: (3, 7, 3), 64: (4, 4, 4), 65: (5, 13, 1), 4095: (15, 91, 3), 4096: (32, 32, 4),
              4097: (17, 241, 1), 8197: (7, 1171, 1)}
    for per_frame, (h, w, c) in frames.items():
        assert h * w * c == per_frame
        for n in (1, 3):
            for mask in ("", "zero", "full", "random"):
                add(id=f"sse_pf{per_frame}_c{c}_n{n}_{mask or 'nomask'}", op="sse", expect=S, shape=(n, h, w, c), mask=mask)
    for c in (1, 3, 4):
        add(id=f"sse_3x37x53x{c}_random", op="sse", expect=S, shape=(3, 37, 53, c), mask="random")
    add(id="sse_1080p_255_vs_0", op="sse", expect=S, shape=(1, 1080, 1920, 3), kind="extreme")


SSIM_BLOCKS = (1, 2, 4, 8, 10, 11, 12, 16, 32)


def _ssim_cases(add):
    for b in SSIM_BLOCKS:
        gy, gx = (9, 11) if b <= 4 else (3, 5)                # 99 blocks (two workgroups of 64) / 15 blocks
        h, w = gy * b + b // 2, gx * b + (2 * b) // 3         # b does not divide the frame (b > 1)
        for c in (1, 3):
            for content in SSIM_CONTENT:
                add(id=f"ssim_b{b}_c{c}_{content}", op="ssim", expect="block_ssim_kernel",
                    shape=(2 if content in ("noise", "noise_near", "bright_flat") else 1, h, w, c), block=b, kind=content)


def _build_cases():
    C_ = []
    add = lambda **kw: C_.append(Case(**kw))
    for fn in (_recompose_cases, _area_cases, _blend_cases, _select_cases, _tile_cases, _sse_cases, _ssim_cases):
        fn(add)
    for j, c in enumerate(C_):
        c.seed = 100 + j
    return C_


CASES = _build_cases()
OPS = ("recompose", "area", "blend", "select", "accumulate", "normalize", "sse", "ssim")
# launched by elvis_recompose_u8 after the recompose kernel whenever map_out is given; every such case checks its output
ALSO_RUN = {"clamp_map_kernel"}


# ============================================================================================ inputs (shared, read-only)
def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=4)
def _inputs_cached(case_id: str):
    return _make_inputs(BY_ID[case_id])


def inputs(case: Case):
    """The case's input arrays (read-only; built once per case and shared between the GPU test and the CPU checks)."""
    return _inputs_cached(case.id)


def _make_inputs(c: Case):
    rng = np.random.default_rng(c.seed)
    n, h, w, ch = c.shape
    if c.op == "recompose":
        by, bx = c.grid or (h // c.block, w // c.block)
        a = rng.integers(0, 128, c.shape, dtype=np.uint8)               # disjoint ranges: every byte tells its source
        b = rng.integers(128, 256, c.shape, dtype=np.uint8)
        m = rng.integers(-3, 7, (n, by, bx)).astype(np.int32)
        flat = m.reshape(-1)
        if flat.size >= 4:
            where = rng.choice(flat.size, size=max(flat.size // 8, 2), replace=False)
            flat[where[0::2]] = INT32_MAX
            if c.kind != "none":
                flat[where[1::2]] = INT32_MIN
        return _ro(a, b, m)
    if c.op == "area":
        x = every_sum_image(c.factor, ch, c.factor) if c.kind == "every_sum" else rng.integers(0, 256, c.shape, dtype=np.uint8)
        return _ro(x)
    if c.op == "blend":
        by, bx = h // c.block, w // c.block
        if c.kind.startswith("pairs"):
            o = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None, None], c.shape).copy()
            r = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :, None], c.shape).copy()
            m = rng.integers(-2, 4, (n, by, bx)).astype(np.int32) if c.kind == "pairs" else \
                rng.integers(1, 4, (n, by, bx)).astype(np.int32)
        else:
            o, r = rng.integers(0, 256, c.shape, dtype=np.uint8), rng.integers(0, 256, c.shape, dtype=np.uint8)
            m = rng.integers(-2, 4, (n, by, bx)).astype(np.int32)
        return _ro(o, r, m)
    if c.op == "select":
        vs = tuple(rng.integers(1, 256, c.shape, dtype=np.uint8) for _ in range(c.versions))   # never 0: 0 means "none"
        m = rng.integers(-2, len(c.slots) + 2, (n, h // c.block, w // c.block)).astype(np.int32)
        return _ro(*vs, m)
    if c.op == "accumulate":
        out = []
        for (y0, x0, th, tw, _) in c.tiles:
            out += [rng.integers(0, 256, (th, tw, ch), dtype=np.uint8), rng.random(th).astype(F32), rng.random(tw),
                    rng.random(tw)]
        return _ro(*out)
    if c.op == "normalize":
        return _ro(*(normalize_edges(ch) if c.kind == "edges" else normalize_random(rng, h, w, ch)))
    if c.op == "sse":
        if c.kind == "extreme":
            return _ro(np.full(c.shape, 255, np.uint8), np.zeros(c.shape, np.uint8), None)
        a, b = rng.integers(0, 256, c.shape, dtype=np.uint8), rng.integers(0, 256, c.shape, dtype=np.uint8)
        mk = {"": None, "zero": np.zeros((n, h, w), np.uint8), "full": np.full((n, h, w), 255, np.uint8),
              "random": np.array([0, 1, 2, 255], np.uint8)[rng.integers(0, 4, (n, h, w))]}[c.mask]
        return _ro(a, b, mk)
    if c.op == "ssim":
        return _ro(*ssim_pair(c.kind, n, h, w, ch, c.seed))
    raise ValueError(c.op)


NORMALIZE_EXACT_WSUM = (0.75, 1.5, 3.0, 0.3125, 2.0 ** -100)       # few mantissa bits: k * weight is exact in float32
NORMALIZE_WSUM = NORMALIZE_EXACT_WSUM + (0.0, -0.0, 1e-30, -1.0, -1e-30)


def normalize_edges(c: int):
    """(acc [h, w, c], wsum [h, w]) float32: for every weight of NORMALIZE_WSUM (ordinary, tiny, zero, negative) and
    every k in 0 .. 255 (channel ch: k + 85 ch, wrapped) the accumulators whose quotient is exactly k (exactly, for the
    weights of NORMALIZE_EXACT_WSUM and for the non-positive ones, which divide by 1), the float32 just below, k + 0.5,
    a negative one and one beyond 255."""
    rows = []
    for ws in NORMALIZE_WSUM:
        div = F32(ws) if ws > 0 else F32(1.0)
        k = (np.arange(256)[:, None] + 85 * np.arange(c)[None, :]) % 256
        exact = (k.astype(F64) * F64(div)).astype(F32)
        assert ws == 1e-30 or (exact.astype(F64) == k * F64(div)).all()
        below = np.nextafter(exact, F32(-np.inf))
        half = ((k + 0.5) * F64(div)).astype(F32)
        neg = (-(k + 1.0) * F64(div)).astype(F32)
        beyond = ((256.0 + k) * F64(div)).astype(F32)
        for acc in (exact, below, half, neg, beyond):
            rows.append((np.full(256, ws, F32), acc))
    wsum = np.concatenate([r[0] for r in rows])
    acc = np.concatenate([r[1] for r in rows])
    h = len(rows)
    return acc.reshape(h, 256, c).copy(), wsum.reshape(h, 256).copy()


def normalize_random(rng, h, w, c):
    wsum = (rng.random((h, w)) * 3.0).astype(F32)
    wsum[rng.random((h, w)) < 0.1] = 0.0
    wsum[rng.random((h, w)) < 0.05] = -0.5
    acc = ((rng.random((h, w, c)) * 300.0 - 20.0) * np.where(wsum > 0, wsum, 1.0)[..., None]).astype(F32)
    return acc, wsum


BY_ID = {c.id: c for c in CASES}


# ============================================================================================ expected outputs
def expected(c: Case, *, mutant: Optional[str] = None):
    """The reference output(s) of a case as a tuple of arrays (the exact ops); `mutant` is handed to the reference."""
    x = inputs(c)
    kw = {"mutant": mutant} if mutant else {}
    if c.op == "recompose":
        a, b, m = x
        mo = () if c.clamp_to is None else (clamp_map_ref(m, c.thr, c.clamp_to, **({"mutant": mutant} if mutant == "no_clamp" else {})),)
        return (recompose_ref(a, b, m, c.block, c.thr, **({} if mutant == "no_clamp" else kw)),) + mo
    if c.op == "area":
        if c.big and c.factor == 4 and not mutant:
            return (area_ref_u16(x[0], c.factor, c.rounding),)
        return (area_ref(x[0], c.factor, c.rounding, **kw),)
    if c.op == "blend":
        return (blend_ref(x[0], x[1], x[2], c.block, c.alpha, **kw),)
    if c.op == "select":
        return (select_ref(list(x[:-1]), np.asarray(c.slots, np.int32), x[-1], c.block),)
    if c.op == "normalize":
        return (tile_normalize_ref(x[0], x[1], **kw),)
    if c.op == "sse":
        return sse_ref(x[0], x[1], x[2], **kw)
    raise ValueError(c.op)


def accumulate_expected(c: Case, acc, wsum, *, mutant: Optional[str] = None):
    """Applies the case's tiles in sequence to copies of acc [h, w, c] / wsum [h, w]."""
    acc, wsum = acc.copy(), wsum.copy()
    x = inputs(c)
    for i, (y0, x0, th, tw, tweight) in enumerate(c.tiles):
        tile, wy, wx, wx2 = x[4 * i:4 * i + 4]
        tile_accumulate_ref(acc, wsum, tile, wy, wx, wx2, y0, x0, tweight, **({"mutant": mutant} if mutant else {}))
    return acc, wsum


def first_difference(got: np.ndarray, ref: np.ndarray):
    """Index tuple of the first differing element (bitwise for floats), or None."""
    if got.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        ne = got.view(u) != ref.view(u)
    else:
        ne = got != ref
    if not ne.any():
        return None
    return tuple(int(i) for i in np.argwhere(ne)[0])
