"""float64 references with explicit error models for the window attention, fused Swin and DCNv2 kernels, and the
case matrix of tests/test_gpu_model_kernels_matrix.py (importable without a GPU: the dispatch ledger and the mutation
self-test of tests/test_model_kernels_ledger.py use it on the CPU).

Each reference computes what the kernel is SPECIFIED to compute, from exactly the operands it multiplies (the stored
f16 / fp32 inputs, f16(W) for the packed Swin weights, the fp32 bias table, scale, biases as passed), and returns a
`Bound`: `ref` plus two absolute terms of the value the kernel rounds to its output type,

  e1  the tier-1 term:  |y - ref| <= 1/2 ulp_out(|ref| + e1) + e1 on every element;
  e2  the tier-2 term (f16 outputs):  y == RNE16(t) for some t in [ref - e2, ref + e2] on a fraction >= the op's floor.

The terms are sums of named pieces, each derived below from the kernel's code.  U24 = 2^-24 is the fp32 unit roundoff.
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from _convref import EPS_ACT_REL, L_ACT, U24, elf_symbols, rne16, trunc16, ulp16, ulp32  # noqa: F401

LOG2E = 1.4426950408889634
# Tier-2 floors: the fraction of f16 outputs that must be a correct rounding of a value inside [ref - e2, ref + e2].
# Observed minimum over the matrix on one MI355X: 1.00000 for every Swin case and every f16 DCNv2 case (tile and
# generic).  The floor keeps the conv matrix's 0.998: truncated outputs / samples score 0.50 - 0.97 in the mutation
# self-test.
TIER2_FLOOR = {"swin": 0.998, "dcn": 0.998}
# Tier-2 accumulation term, as in the conv matrix: 8 fp32 ulps of sum |a||b| (the rigorous gamma_K is for tier 1).
ETA = 2.0 ** -21


def gamma(n: int) -> float:
    """Worst-case relative error of an fp32 sum of n terms (with two extra roundings of slack)."""
    return (n + 2) * U24


@dataclass
class Bound:
    ref: torch.Tensor
    e1: torch.Tensor
    e2: Optional[torch.Tensor] = None
    out_f16: bool = True

    def bound(self):
        ulp = ulp16 if self.out_f16 else ulp32
        return 0.5 * ulp(self.ref.abs() + self.e1) + self.e1


def tier1(y: torch.Tensor, b: Bound):
    """(every element within the bound, worst |y - ref| / bound, index of the worst element)."""
    ratio = (y - b.ref).abs() / b.bound()
    ratio = torch.where(torch.isnan(y), torch.full_like(ratio, float("inf")), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    return worst <= 1.0, worst, np.unravel_index(int(torch.argmax(ratio)), tuple(ratio.shape))


def tier2(y: torch.Tensor, b: Bound) -> float:
    """Fraction of the elements equal to RNE16(t) for some t in [ref - e2, ref + e2] (rounding is monotone)."""
    ok = (y >= rne16(b.ref - b.e2)) & (y <= rne16(b.ref + b.e2))
    return float(ok.double().mean())


def midpoint_dev(t: torch.Tensor, tol: torch.Tensor):
    """(RNE16(t), how far the kernel's f16 value may sit from it).  The kernel rounds a value within `tol` of t: where t
    lies within tol of an f16 rounding midpoint that value may round the other way - by at most ulp16(|t| + tol) + tol
    in all (one ulp when tol is far below an ulp).  Elsewhere both round to the same f16."""
    th = rne16(t)
    u = ulp16(t)
    mid = torch.minimum((t - (th + 0.5 * u)).abs(), (t - (th - 0.5 * u)).abs())
    near = mid <= tol
    return th, torch.where(near, ulp16(t.abs() + tol) + tol, torch.zeros_like(t))


# ============================================================================================ window attention
def _windows(t: torch.Tensor, ws: int):
    """[n, h, w, c] -> [n * nwy * nwx, ws * ws, c], windows in (n, wy, wx) order, tokens row-major."""
    n, h, w, c = t.shape
    t = t.view(n, h // ws, ws, w // ws, ws, c).permute(0, 1, 3, 2, 4, 5)
    return t.reshape(-1, ws * ws, c)


def _unwindows(t: torch.Tensor, n, h, w, ws):
    c = t.shape[-1]
    t = t.view(n, h // ws, w // ws, ws, ws, c).permute(0, 1, 3, 2, 4, 5)
    return t.reshape(n, h, w, c)


def shift_mask(h, w, ws, shift) -> torch.Tensor:
    """[nwy * nwx, ws^2, ws^2]: 0 within a region, -100 across (the standard Swin mask; zeros without a shift)."""
    nw = (h // ws) * (w // ws)
    if not shift:
        return torch.zeros(nw, ws * ws, ws * ws, dtype=torch.float64)
    ry = torch.zeros(h, dtype=torch.long)
    ry[h - ws:] = 1
    ry[h - shift:] = 2
    rx = torch.zeros(w, dtype=torch.long)
    rx[w - ws:] = 1
    rx[w - shift:] = 2
    reg = (ry[:, None] * 3 + rx[None, :]).double()[None, :, :, None]
    rw = _windows(reg, ws)[..., 0]
    return torch.where(rw[:, :, None] != rw[:, None, :], -100.0, 0.0).double()


def relative_position_index(ws: int) -> torch.Tensor:
    from elvis_amd.weights import relative_position_index as rpi
    return rpi(ws)


def attention_ref(qkv: torch.Tensor, heads: int, shift: int, table: torch.Tensor, scale: float, *, f16: bool = True,
                  ws: int = 8, rpi: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                  roll_sign: int = 1, head_of_bias=None, v_key_perm=None) -> Bound:
    """qkv [n, h, w, 3E] (the stored values, float64), table [(2ws-1)^2, heads] (the fp32 table), scale (the fp32 value
    passed).  Logits L = scale q.k + B[rel] + mask(-100) in float64, softmax, P.V; output [n, h, w, E] in image order.
    The keyword overrides exist for the mutation self-test only (a transposed index, a mask, the roll's sign, the bias
    column each head reads, a key permutation of V)."""
    n, h, w, e3 = qkv.shape
    E, hd, nt = e3 // 3, e3 // 3 // heads, ws * ws
    t = torch.roll(qkv, (-roll_sign * shift, -roll_sign * shift), (1, 2)) if shift else qkv
    win = _windows(t, ws)                                               # [NW, 64, 3E]
    q, k, v = win.view(-1, nt, 3, heads, hd).permute(2, 0, 3, 1, 4)     # [NW, heads, 64, hd]
    if v_key_perm is not None:
        v = v[:, :, v_key_perm]
    S = q @ k.transpose(-1, -2)
    SA = q.abs() @ k.abs().transpose(-1, -2)                            # sum_d |q_d k_d|
    rpi = relative_position_index(ws) if rpi is None else rpi
    cols = torch.arange(heads) if head_of_bias is None else torch.as_tensor(head_of_bias)
    B = table[rpi.reshape(-1)][:, cols].view(nt, nt, heads).permute(2, 0, 1)   # [heads, 64, 64]
    M = shift_mask(h, w, ws, shift) if mask is None else mask              # [nwin, 64, 64]
    M = M.repeat(n, 1, 1)[:, None]
    L = scale * S + B[None] + M
    mx = L.max(-1, keepdim=True).values
    ex = torch.exp(L - mx)
    den = ex.sum(-1, keepdim=True)                                       # >= 1: the row maximum contributes 1
    p = ex / den
    ref = p @ v
    spv = p @ v.abs()                                                   # sum_j p_j |v_j|
    s1v = v.abs().sum(-2, keepdim=True) / den                           # sum_j |v_j| / den
    masked = (M != 0).double()
    if f16:
        # window_attention_tr_kernel, in log2 units a = L log2(e):
        #  * S: 32 exact f16 products summed by v_mfma_f32_16x16x32_f16 into fp32: gamma(32) sum|q k|, times scale log2(e);
        #  * a = fma(S, scale2, B2) with scale2 = fp32(scale * 1.4426950f) and B2 = fp32(B * 1.4426950f) (stored to LDS):
        #    the constant, the two products and the fma are ~3 roundings of |scale S| and of |B| (log2 units) and one of |a|;
        #  * the mask adds fp32(-100 log2 e) = -144.26950f: the constant and the add, 2 roundings of 144.27;
        #  * a - mx: one rounding of |a - mx|;  v_exp_f32: ~1 ulp relative = 2^-23 / ln 2 in log2 units (2^-22 taken).
        #  The largest such logit error D of a row perturbs every normalised p_j by a factor within 2^(+-2D): the
        #  output moves by at most (2^(2D) - 1) sum_j p_j |v_j|.
        a = L * LOG2E
        D = (LOG2E * scale * gamma(32) * SA + 3 * U24 * LOG2E * (scale * S).abs() + 3 * U24 * LOG2E * B.abs()[None]
             + U24 * a.abs() + masked * 2 * U24 * 144.27 + U24 * (a - a.max(-1, keepdim=True).values).abs() + 2.0 ** -22)
        Dr = D.max(-1, keepdim=True).values
        e_logit = (torch.exp2(2 * Dr) - 1) * spv
        # * P is stored to f16 UNNORMALISED (values exp2(a - mx) in (0, 1]) and the row sum is the fp32 sum of the
        #   unrounded values: a relative 2^-11 of sum p_j |v_j| for normal P, and below 2^-14 the subnormal grid's
        #   absolute 2^-25 per key, i.e. 2^-25 sum_j |v_j| / den after the normalisation;
        e_p16 = 2.0 ** -11 * spv + 2.0 ** -25 * s1v
        # * the row sum of 64 values (16 in a lane, then two shuffle adds): gamma(64) relative; rcp: 1 ulp (2^-22 taken);
        #   O * inv: one rounding; P.V over 64 keys on the matrix cores in fp32: gamma(64) of sum P^ |v| (P^ <= p(1 + 2^-10)).
        e_norm = (gamma(64) + 2.0 ** -22 + U24) * spv + gamma(64) * (1 + 2.0 ** -10) * (spv + 2.0 ** -25 * s1v)
        e = e_logit + e_p16 + e_norm
    else:
        # window_attention_kernel<float>, in nats: q * scale (1 rounding of |scale q|, i.e. of |scale q k| per product),
        # 32 fmas: gamma(32) sum |scale q k|; + bias (1 rounding of |a|); the mask adds -100.0f exactly representable (1
        # rounding of |a|); s - mx (1 rounding); expf: ~1 ulp (2^-22 taken).  Then as above with (e^(2D) - 1).
        D = (gamma(33) * scale * SA + 2 * U24 * L.abs() + U24 * (L - mx).abs() + 2.0 ** -22)
        Dr = D.max(-1, keepdim=True).values
        e_logit = torch.expm1(2 * Dr) * spv
        # the sum of 64 expf values: gamma(64); 1.0f / sum: correctly rounded (2^-24), p = s * inv: one rounding; P.V: 64
        # fmas, gamma(64) of sum p |v|
        e = e_logit + (2 * gamma(64) + 3 * U24) * spv
    out = _unwindows(ref.permute(0, 2, 1, 3).reshape(-1, nt, E), n, h, w, ws)
    err = _unwindows(e.permute(0, 2, 1, 3).reshape(-1, nt, E), n, h, w, ws)
    if shift:
        out = torch.roll(out, (roll_sign * shift, roll_sign * shift), (1, 2))
        err = torch.roll(err, (roll_sign * shift, roll_sign * shift), (1, 2))
    return Bound(out, err, None, f16)


# ============================================================================================ fused Swin
# LayerNorm in swin_fused_kernel (LINEAR / MLP: on the f16 tokens; PROJ: on the fp32 accumulators y'):
#  * mean: a lane sums C/4 values sequentially, then two shuffle adds, then / C: gamma(C/4 + 3) sum|x| / C = eps_m;
#  * var: d = x - mean (one rounding of |d|), C/4 fmas + two adds: gamma(C/4 + 3) relative, plus the mean's own error
#    (second order: sum(x - mean) = 0); q / C + eps, sqrtf, 1.0f / : ~4 roundings.  rstd relative: delta_r = gamma/2 + 6u;
#  * t = (x - mean) * rstd * g + h: the error of mean times rstd |g|, delta_r + 3 roundings of |x - mean| rstd |g|, one
#    rounding of |t|.
# PROJ adds y' = y + Wp a + bp (bp as the accumulator's start, C/32 MFMAs of 32 products, + y): gamma(C + 2) of
# sum |Wp^||a| + |bp| + |y| per channel = eps_y, which moves x - mean by eps_y + mean(eps_y) and rstd by max(eps_y) rstd.
def ln_tol(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, eps: float, eps_y: Optional[torch.Tensor] = None):
    """(t = LN(x) g + b in float64, the kernel's possible deviation from t before the f16 rounding).  x [M, C]."""
    C = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    t = d * rstd * g + b
    gm = gamma(C // 4 + 3)
    eps_m = gm * x.abs().mean(-1, keepdim=True) + U24 * mean.abs()
    dr = gm / 2 + 6 * U24
    xm = d.abs() * rstd * g.abs()
    tol = eps_m * rstd * g.abs() + (dr + 3 * U24) * xm + U24 * t.abs()
    if eps_y is not None:
        ey = eps_y + eps_y.mean(-1, keepdim=True)
        tol = tol + ey * rstd * g.abs() + eps_y.max(-1, keepdim=True).values * rstd * xm
    return t, tol


def _gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def swin_ref(mode: int, x: torch.Tensor, gamma_: torch.Tensor, beta: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor,
             w2: Optional[torch.Tensor] = None, b2: Optional[torch.Tensor] = None, *, y: Optional[torch.Tensor] = None,
             wp: Optional[torch.Tensor] = None, bp: Optional[torch.Tensor] = None, eps: float = 1e-5,
             drop_last_chunk: bool = False, w2_cols=None, residual: bool = True) -> Bound:
    """mode 0 LINEAR z = W1^ xn^ + b1; 1 MLP out = x + W2^ H^ + b2, H^ = f16(gelu(W1^ xn^ + b1)); 2 PROJ: y' = y + Wp^ x
    + bp, out = y' + W2^ H^ + b2 with xn^ = f16(LN(y')).  Tokens [M, C] float64 of the stored f16 values; weights as
    f16(W) float64; biases / gamma / beta the fp32 values.  drop_last_chunk, w2_cols, residual: mutation hooks."""
    if mode == 2:
        yp = y + x @ wp.T + bp
        Ay = x.abs() @ wp.abs().T + bp.abs() + y.abs()
        # y' is the fp32 accumulator the output starts from: gamma(C + 2) Ay for tier 1, ETA Ay for tier 2 and for the
        # midpoint indicator of LN(y') (as for S below)
        t, tol = ln_tol(yp, gamma_, beta, eps, ETA * Ay)
        res, res_abs, res_e1, res_e2 = yp, yp.abs(), gamma(x.shape[-1] + 2) * Ay, ETA * Ay
    else:
        t, tol = ln_tol(x, gamma_, beta, eps)
        res, res_abs, res_e1, res_e2 = x, x.abs(), 0.0, 0.0
    xn, dev_x = midpoint_dev(t, tol)
    # first GEMM: b1 is the accumulator's start, C/32 MFMAs of 32 exact f16 products
    S = xn @ w1.T + b1
    AS = xn.abs() @ w1.abs().T + b1.abs()
    PS = dev_x @ w1.abs().T                                 # the xn values that may have rounded the other way
    if mode == 0:
        return Bound(S, gamma(x.shape[-1] + 2) * AS + PS, ETA * AS + PS, True)
    # H^ = f16(gelu_erf_f(S)): S within eta_S = 2^-21 AS + PS of the kernel's accumulator (the tier-2 figure: the worst
    # case gamma(C) AS would flag nearly every hidden value), gelu's Lipschitz 1.129 and EPS_ACT_REL[1] |S| for the A&S
    # erf, __expf and rcp of common.h gelu_erf_f
    G = _gelu(S)
    tolH = L_ACT[1] * (ETA * AS + PS) + EPS_ACT_REL[1] * S.abs()
    H, dev_h = midpoint_dev(G, tolH)
    if drop_last_chunk:
        H = H.clone()
        H[:, -64:] = 0
    w2u = w2 if w2_cols is None else w2[:, w2_cols]
    # second GEMM over all hidden chunks into the same fp32 accumulators, then + b2 + the residual (MLP) or from y' (PROJ)
    z = H @ w2u.T + b2 + (res if residual else 0.0)
    A = H.abs() @ w2u.abs().T + b2.abs() + res_abs
    P = dev_h @ w2u.abs().T
    return Bound(z, gamma(w2.shape[1] + 3) * A + P + res_e1, ETA * A + P + res_e2, True)


# ============================================================================================ DCNv2
def _sigmoid(m):
    return 1.0 / (1.0 + torch.exp(-m))


def dcn_samples(x: torch.Tensor, om: torch.Tensor, dg: int, mask_sigmoid: bool, *, tile: bool, swap_dydx=False,
                clamp_edges=False, mask_group_shift=0):
    """Modulated samples s[n, h, w, K] (k = c * 9 + tap) of x [n, h, w, cin] (stored values) at p + tap + d from om
    [n, h, w, >= 27 dg] (stored offsets / masks), out-of-image corners zero; and the kernel's possible deviation from each
    in fp32.  The mutation hooks: swap_dydx, clamp_edges (edge-clamped corners), mask_group_shift (group g reads g + s)."""
    n, h, w, cin = x.shape
    cpg = cin // dg
    c = torch.arange(cin)[:, None]
    tap = torch.arange(9)[None, :]
    g = c // cpg
    gk = (g * 9 + tap).reshape(-1)                            # [K]
    dy, dx = om[..., 2 * gk], om[..., 2 * gk + 1]
    if swap_dydx:
        dy, dx = dx, dy
    mg = ((g + mask_group_shift) % dg * 9 + tap).reshape(-1)
    m = om[..., 18 * dg + mg]
    if mask_sigmoid:
        sg = _sigmoid(m)
        # generic: 1 / (1 + expf(-m)): expf ~1 ulp, the add and the division: 2^-21 relative.  tile: rcp(1 + exp2(-log2e m)):
        # the product rounds |m log2 e| by 2^-24 (a relative 2^-24 |m| of the exponential after exp2), v_exp_f32 and rcp
        # ~1 ulp each, the add: 2^-20 + 2^-24 |m| relative
        sig_rel = (2.0 ** -20 + U24 * m.abs()) if tile else torch.full_like(m, 2.0 ** -21)
        m = sg
    else:
        sig_rel = torch.zeros_like(m)
    ky = (tap // 3 - 1).expand(cin, 9).reshape(-1).double()
    kx = (tap % 3 - 1).expand(cin, 9).reshape(-1).double()
    yo = torch.arange(h, dtype=torch.float64)[None, :, None, None]
    xo = torch.arange(w, dtype=torch.float64)[None, None, :, None]
    sy, sx = yo + ky + dy, xo + kx + dx
    fy, fx = torch.floor(sy), torch.floor(sx)
    ly, lx = sy - fy, sx - fx
    y0, x0 = fy.long(), fx.long()
    cidx = c.expand(cin, 9).reshape(-1)                       # channel of sample k
    nidx = torch.arange(n)[:, None, None, None]

    def corner(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = x[nidx, yy.clamp(0, h - 1), xx.clamp(0, w - 1), cidx]
        return v if clamp_edges else torch.where(ok, v, torch.zeros_like(v))

    v00, v01, v10, v11 = corner(y0, x0), corner(y0, x0 + 1), corner(y0 + 1, x0), corner(y0 + 1, x0 + 1)
    bil = (1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11)
    s = m * bil
    # the kernel's error of a sample:
    #  * the position: fp32(yo + tap) + dy is one rounding (1/2 ulp32 of |sy|, likewise x), floor and sy - floor are exact;
    #    the interpolant moves by at most Lipschitz x shift, with the cell's corner differences as the constant - or, for a
    #    position within that shift of a cell edge (the neighbouring cell's corners apply), 2 max|x| of the channel;
    #  * the lerps: generic form ~6 roundings, tile form three fmas and two subtractions: 8 roundings of the corners' max;
    #  * the product with m: one rounding; the sigmoid's relative error above.
    py, px = 0.5 * ulp32(sy), 0.5 * ulp32(sx)
    cmax = torch.stack([v00.abs(), v01.abs(), v10.abs(), v11.abs()]).max(0).values
    lip_y = torch.maximum((v10 - v00).abs(), (v11 - v01).abs())
    lip_x = torch.maximum((v01 - v00).abs(), (v11 - v10).abs())
    xmax = x.abs().amax((0, 1, 2))[cidx]
    edge_y = (ly <= py) | (1 - ly <= py)
    edge_x = (lx <= px) | (1 - lx <= px)
    lip_y = torch.where(edge_y, 2 * xmax.expand_as(lip_y), lip_y)
    lip_x = torch.where(edge_x, 2 * xmax.expand_as(lip_x), lip_x)
    tol = m.abs() * (lip_y * py + lip_x * px + 8 * U24 * cmax) + s.abs() * (sig_rel + U24)
    return s, tol


def dcn_ref(x, om, wt, bias, dg, mask_sigmoid, *, tile: bool, f16_out: bool, act: int = 0, trunc_samples=False,
            **hooks) -> Bound:
    """out [n, h, w, cout] = act(b + sum_k W[co][k] s_k).  wt [cout, cin * 9] (stored values), bias fp32 or None."""
    s, tol = dcn_samples(x, om, dg, mask_sigmoid, tile=tile, **hooks)
    b = torch.zeros(wt.shape[0], dtype=torch.float64) if bias is None else bias
    K = wt.shape[1]
    if tile:
        # dcnv2_tile_kernel stores every sample to f16 before the MFMA: the reference multiplies RNE16(s), and a sample
        # within tol of a rounding midpoint may round the other way.  Accumulation: the bias is the accumulator's start,
        # ceil(K / 32) MFMAs of 32 exact products.
        sh, dev = midpoint_dev(s, tol)
        if trunc_samples:
            sh = trunc16(s)
        z = sh @ wt.T + b
        A = sh.abs() @ wt.abs().T + b.abs()
        P = dev @ wt.abs().T
        e1, e2 = gamma(K + 2) * A + P, ETA * A + P
    else:
        # dcnv2_kernel: fp32 samples in LDS, K fmas from the bias
        z = s @ wt.T + b
        A = s.abs() @ wt.abs().T + b.abs()
        P = tol @ wt.abs().T
        e1, e2 = gamma(K + 1) * A + P, ETA * A + P
    if act == 3:
        z = z.clamp(min=0.0)   # 1-Lipschitz and monotone: the terms carry over
    return Bound(z, e1, e2, f16_out)


# ============================================================================================ kernel names
def demangle_model(sym: str) -> Optional[str]:
    """`_ZN12_GLOBAL__N_117swin_fused_kernelILi192ELi2ELi1ELb1EEEvNS_8SwinArgsE` -> `swin_fused_kernel<192,2,1,true>`,
    `_ZN12_GLOBAL__N_126window_attention_tr_kernelEPKDF16_...` -> `window_attention_tr_kernel`; None for every symbol
    that is not a window_attention_*, swin_fused_kernel or dcnv2_* kernel."""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", sym)
    if not m:
        return None
    ln, pos = int(m.group(1)), m.end()
    name = sym[pos:pos + ln]
    if not (re.fullmatch(r"window_attention_\w*kernel", name) or name == "swin_fused_kernel"
            or re.fullmatch(r"dcnv2_\w*kernel", name)):
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


def model_kernel_symbols(path: str):
    return {nm for nm in (demangle_model(s) for s in elf_symbols(path)) if nm is not None}


# ============================================================================================ cases
SWIN_PXT = {64: 2, 128: 2, 192: 2, 256: 1}
SWIN_STAG = {(64, 1): False, (128, 1): False, (192, 1): True, (256, 1): True,
             (64, 2): False, (128, 2): False, (192, 2): False, (256, 2): True}


def swin_name(c, mode):
    st = SWIN_STAG.get((c, mode), False)
    return f"swin_fused_kernel<{c},{SWIN_PXT[c]},{mode},{'true' if st else 'false'}>"


@dataclass
class Case:
    id: str
    op: str                       # attn | swin | dcn
    expect: str
    # attention
    heads: int = 2
    shift: int = 0
    dt: str = "f16"
    n: int = 1
    h: int = 16
    w: int = 16
    pitch_extra: int = 0          # input pitch beyond its channels (qkv / x / attention output of PROJ)
    out_extra: int = 0            # output pitch beyond its channels
    logits: str = "normal"        # normal | onehot | flat
    # swin
    mode: int = 0
    c: int = 64
    n1: int = 64                  # LINEAR: n_out; MLP / PROJ: hidden
    tokens: int = 100
    y_extra: int = 0
    offset: float = 0.0           # common token offset (LayerNorm cancellation)
    spread: float = 1.5
    # dcn
    cin: int = 7
    dg: int = 7
    cout: int = 64
    sigmoid: bool = True
    bias: bool = True
    act: int = 0
    offsets: str = "small"        # small | six | six_seven | far | mixed
    x_pitch: int = 8
    seed: int = 0


def _build_cases():
    C_ = []
    add = lambda **kw: C_.append(Case(**kw))
    TR, AF = "window_attention_tr_kernel", "window_attention_kernel<float>"
    # ---- attention: heads 1..8 (ATT_NW = 2 waves loop over heads), shifts 0 / 2 / 3 / ws/2 / 6, n > 1
    add(id="attn_tr_h1_s0", op="attn", expect=TR, heads=1, shift=0, h=16, w=24)
    add(id="attn_tr_h2_s4_n2", op="attn", expect=TR, heads=2, shift=4, n=2, h=16, w=24)
    add(id="attn_tr_h3_s4", op="attn", expect=TR, heads=3, shift=4, h=24, w=16)
    add(id="attn_tr_h4_s2", op="attn", expect=TR, heads=4, shift=2, h=16, w=32)
    add(id="attn_tr_h6_s6", op="attn", expect=TR, heads=6, shift=6, h=24, w=24)
    add(id="attn_tr_h8_s4_n3", op="attn", expect=TR, heads=8, shift=4, n=3, h=16, w=16)
    # a single window row / column / window with a shift: every window is masked (need_mask on all of them)
    add(id="attn_tr_row_s4", op="attn", expect=TR, heads=2, shift=4, h=8, w=40)
    add(id="attn_tr_col_s4", op="attn", expect=TR, heads=4, shift=4, h=40, w=8)
    add(id="attn_tr_one_window_s3", op="attn", expect=TR, heads=2, shift=3, h=8, w=8)
    # pitches wider than 3E / E
    add(id="attn_tr_pitch", op="attn", expect=TR, heads=4, shift=4, h=16, w=24, pitch_extra=24, out_extra=16)
    # near-one-hot and flat softmax rows
    add(id="attn_tr_onehot", op="attn", expect=TR, heads=2, shift=4, h=16, w=16, logits="onehot")
    add(id="attn_tr_flat", op="attn", expect=TR, heads=2, shift=4, h=16, w=16, logits="flat")
    add(id="attn_f32_h3_s4_n2", op="attn", expect=AF, dt="f32", heads=3, shift=4, n=2, h=16, w=24)
    add(id="attn_f32_row_s2_pitch", op="attn", expect=AF, dt="f32", heads=2, shift=2, h=8, w=32, pitch_extra=8, out_extra=8)
    add(id="attn_f32_onehot", op="attn", expect=AF, dt="f32", heads=2, shift=4, h=16, w=16, logits="onehot")
    # ---- fused Swin: the 12 (C, MODE) pairs on their default STAG, chunk counts 1 / odd / even, n_out != 3C, token
    #      counts 1, 16 PXT - 1, 128 PXT and several workgroups, wide pitches, LayerNorm cancellation
    add(id="swin_lin_64_n64_t1", op="swin", expect=swin_name(64, 0), mode=0, c=64, n1=64, tokens=1)
    add(id="swin_lin_128_qkv_t256", op="swin", expect=swin_name(128, 0), mode=0, c=128, n1=384, tokens=256)
    add(id="swin_lin_192_qkv_pitch", op="swin", expect=swin_name(192, 0), mode=0, c=192, n1=576, tokens=300,
        pitch_extra=8, out_extra=24)
    add(id="swin_lin_256_n192_t128", op="swin", expect=swin_name(256, 0), mode=0, c=256, n1=192, tokens=128)
    add(id="swin_lin_64_cancel", op="swin", expect=swin_name(64, 0), mode=0, c=64, n1=192, tokens=200, offset=48.0,
        spread=0.5)
    add(id="swin_mlp_64_h64_t31", op="swin", expect=swin_name(64, 1), mode=1, c=64, n1=64, tokens=31)
    add(id="swin_mlp_128_h192_t600", op="swin", expect=swin_name(128, 1), mode=1, c=128, n1=192, tokens=600)
    add(id="swin_mlp_192_h320_pitch", op="swin", expect=swin_name(192, 1), mode=1, c=192, n1=320, tokens=256,
        pitch_extra=16, out_extra=8)
    add(id="swin_mlp_192_h768_t1", op="swin", expect=swin_name(192, 1), mode=1, c=192, n1=768, tokens=1)
    add(id="swin_mlp_256_h192_t15", op="swin", expect=swin_name(256, 1), mode=1, c=256, n1=192, tokens=15)
    add(id="swin_mlp_256_h512_cancel", op="swin", expect=swin_name(256, 1), mode=1, c=256, n1=512, tokens=300,
        offset=40.0, spread=0.5)
    add(id="swin_proj_64_h256_pitch", op="swin", expect=swin_name(64, 2), mode=2, c=64, n1=256, tokens=257,
        pitch_extra=8, y_extra=16, out_extra=8)
    add(id="swin_proj_128_h64_t31", op="swin", expect=swin_name(128, 2), mode=2, c=128, n1=64, tokens=31)
    add(id="swin_proj_192_h448_t256", op="swin", expect=swin_name(192, 2), mode=2, c=192, n1=448, tokens=256)
    add(id="swin_proj_256_h320_t128", op="swin", expect=swin_name(256, 2), mode=2, c=256, n1=320, tokens=128, y_extra=8)
    add(id="swin_proj_256_h256_cancel", op="swin", expect=swin_name(256, 2), mode=2, c=256, n1=256, tokens=200,
        offset=40.0, spread=0.5)
    # ---- DCNv2: tile<7> / tile<8> with and without the sigmoid, bias None, ragged cout, the +-6 fast-path threshold,
    #      6..7 px (checked loop, LDS window), far offsets (global reads, inside the image), a mixed launch, an image
    #      smaller than one 8 x 32 tile, 1080 rows; the generic kernel in f16 and f32
    T7, T8, GH, GF = "dcnv2_tile_kernel<7>", "dcnv2_tile_kernel<8>", "dcnv2_kernel<half>", "dcnv2_kernel<float>"
    add(id="dcn_tile7_sig", op="dcn", expect=T7, cin=7, dg=7, cout=64, h=16, w=64)
    add(id="dcn_tile8_sig_relu_n2", op="dcn", expect=T8, cin=8, dg=8, cout=48, n=2, h=19, w=45, act=3)
    add(id="dcn_tile7_nosig_nobias", op="dcn", expect=T7, cin=7, dg=7, cout=32, h=16, w=40, sigmoid=False, bias=False)
    add(id="dcn_tile8_cout37_nosig", op="dcn", expect=T8, cin=8, dg=8, cout=37, h=16, w=33, sigmoid=False, out_extra=8)
    add(id="dcn_tile7_six", op="dcn", expect=T7, cin=7, dg=7, cout=16, h=24, w=64, offsets="six")
    add(id="dcn_tile8_six_seven", op="dcn", expect=T8, cin=8, dg=8, cout=64, h=24, w=64, offsets="six_seven")
    add(id="dcn_tile7_far", op="dcn", expect=T7, cin=7, dg=7, cout=24, h=48, w=96, offsets="far")
    add(id="dcn_tile8_mixed", op="dcn", expect=T8, cin=8, dg=8, cout=64, h=16, w=64, offsets="mixed", sigmoid=False)
    add(id="dcn_tile7_small_image", op="dcn", expect=T7, cin=7, dg=7, cout=20, h=5, w=20)
    add(id="dcn_tile8_1080_rows", op="dcn", expect=T8, cin=8, dg=8, cout=16, h=1080, w=24)
    add(id="dcn_generic_f16_sig", op="dcn", expect=GH, cin=4, dg=2, cout=5, h=13, w=19, x_pitch=8)
    add(id="dcn_generic_f16_nosig_far", op="dcn", expect=GH, cin=6, dg=3, cout=12, h=20, w=40, sigmoid=False,
        bias=False, offsets="far", act=3)
    add(id="dcn_generic_f16_pitch16", op="dcn", expect=GH, cin=7, dg=7, cout=64, h=12, w=40, x_pitch=16, out_extra=8)
    add(id="dcn_generic_f32_sig", op="dcn", expect=GF, dt="f32", cin=8, dg=8, cout=16, h=16, w=40, act=3)
    add(id="dcn_generic_f32_nosig_1080", op="dcn", expect=GF, dt="f32", cin=3, dg=1, cout=4, h=1080, w=16,
        sigmoid=False, bias=False)
    for i, c in enumerate(C_):
        c.seed = i
    return C_


CASES = _build_cases()


# ============================================================================================ inputs
def dcn_offsets(c: Case, g: torch.Generator) -> torch.Tensor:
    """[n, h, w, 18 dg] offsets of the case's kind."""
    n, h, w, k2 = c.n, c.h, c.w, 18 * c.dg
    if c.offsets == "small":
        d = (torch.randn(n, h, w, k2, generator=g) * 1.5).clamp(-5.0, 5.0)
    elif c.offsets == "six":
        d = torch.where(torch.rand(n, h, w, k2, generator=g) < 0.5, -6.0, 6.0)
        d = torch.where(torch.rand(n, h, w, k2, generator=g) < 0.3, torch.randn(n, h, w, k2, generator=g).clamp(-6.0, 6.0), d)
    elif c.offsets == "six_seven":
        d = (6.0 + torch.rand(n, h, w, k2, generator=g) * 0.99) * torch.where(torch.rand(n, h, w, k2, generator=g) < 0.5, -1.0, 1.0)
    elif c.offsets == "far":
        # 10 .. 20 px toward the image's centre: beyond the LDS window (halo 8), still inside the image where it fits
        mag = 10.0 + 10.0 * torch.rand(n, h, w, k2, generator=g)
        yy = torch.arange(h, dtype=torch.float32)[None, :, None, None].expand(n, h, w, k2)
        xx = torch.arange(w, dtype=torch.float32)[None, None, :, None].expand(n, h, w, k2)
        is_y = (torch.arange(k2) % 2 == 0)[None, None, None, :]
        toward = torch.where(is_y, torch.where(yy < h / 2, 1.0, -1.0), torch.where(xx < w / 2, 1.0, -1.0))
        d = mag * toward
    elif c.offsets == "mixed":
        # rows 2 and 3 of every 8-row tile (wave 1's pixels) reach 6.5 px: that wave takes the checked loop, the rest
        # the fast one
        d = (torch.randn(n, h, w, k2, generator=g)).clamp(-3.0, 3.0)
        rows = (torch.arange(h) % 8 >= 2) & (torch.arange(h) % 8 < 4)
        d[:, rows, :, 0] = 6.5
    else:
        raise ValueError(c.offsets)
    return d
