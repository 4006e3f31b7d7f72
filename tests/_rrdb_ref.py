"""float64 statements of what csrc/rrdb.hip and elvis_amd/realesrgan.py are specified to compute, written from the
architecture (RRDBNet as basicsr defines it and RealESRGANer.enhance drives it), importable without a GPU.

1. `rrdbnet_ref`: the network.  float64 throughout, or (`storage_f16=True`) the same statement in fp32 arithmetic with
   every stored activation and every weight rounded to f16 - what f16 storage alone costs, the yardstick of the model
   tests.
2. `conv_ref`: one `elvis_rrdb_conv3x3` call, from exactly the operands the kernel multiplies - x^ (the stored f16
   activation, nearest-repeated with `upsample`) and w^ = f16(w):
       z = sum x^ w^ + b;   v = lrelu ? (z > 0 ? z : 0.2 z) : z;   ref = s0 v + s1 r1 + r2
   with the error model of tests/_convref.py derived for this epilogue:
       A = sum |x^||w^| + |b|
       e = |s0| (K + 2) 2^-24 A  +  3 * 2^-24 (|s0 lrelu(z)| + |s1 r1| + |r2|)
       |y - ref| <= 1/2 ulp16(|ref| + e) + e
   Term by term.  K = 9 cin products are summed in fp32 in the matrix unit in an order the test does not know: any
   order of K - 1 additions of products that are exact in fp32 (f16 x f16) is within (K - 1) 2^-24 A of the exact sum
   to first order; the bias addition is one more rounding of at most 2^-24 A; that leaves two spare units of
   2^-24 |s0| A >= 2^-24 |s0 lrelu(z)|.  The epilogue then rounds: 0.2f * z (and 0.2f itself is 0.2 (1 + 2^-26.4)),
   s0 * v, s1 * r1, the sum of the two, the addition of r2.  A term of the result is touched by at most the roundings
   after it: |s0 lrelu(z)| by four (lrelu, s0, both additions), |s1 r1| by three, |r2| by one.  Three of them per term
   are in the second part of e; the fourth on |s0 lrelu(z)| and the constant's own error are covered by the spare
   units of the first.  The stored f16 is the nearest to the fp32 y: half an ulp of a value within e of ref.
3. `out_u8`: the byte is round_half_even(255 clamp(ref, 0, 1)) computed from the fp32 y (one more rounding, the
   multiplication by 255, inside the same three): it may differ by 1 only where 255 clamp(ref) lies within 255 e of a
   half-integer.
4. `pack_ref`: the packed weight layout.  5. `input_ref`: the input stage.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

import _srmut as M
from _convref import U24, rne16, trunc16, ulp16

# ----------------------------------------------------------------------------------------------- one conv
class ConvRef:
    def __init__(self, ref, e):
        self.ref, self.e = ref, e

    def bound(self):
        return 0.5 * ulp16(self.ref.abs() + self.e) + self.e


# The statement with one clause changed (tests/test_sr_ledger.py: each must move a named case of tests/_srcases.py past
# the bound).  The sum's mutants are those of tests/_srmut.py; the epilogue's:
#   bias_roll_1 / _4 / _16   the bias of the neighbouring channel, lane group (4 channels) or accumulator (16)
#   s0_s1_swapped            s1 v + s0 r1 + r2
#   r1_r2_swapped            s0 v + s1 r2 + r1
#   ups_source_round_up      the upsampled row y reads source row (y + 1) >> 1 (the last row again past the end)
#   store_f16_trunc          the f16 store rounds toward zero: `ref` is then the stored value itself
MUTANTS = M.SUM + M.WEIGHTS + ("bias_roll_1", "bias_roll_4", "bias_roll_16", "s0_s1_swapped", "r1_r2_swapped", "ups_source_round_up",
                               "store_f16_trunc")
U8_MUTANTS = ("u8_half_up", "u8_truncate")


def conv_ref(x_hat, w, b, *, upsample=False, lrelu=False, s0=1.0, s1=0.0, r1=None, r2=None, mutant=None) -> ConvRef:
    """x_hat NCHW float64 (the stored f16 values, before `upsample`), w OIHW fp32 (rounded to f16 here), b fp32 [cout],
    r1 / r2 NCHW float64 at the output size or None.  s0, s1 as the fp32 values the kernel receives.  `mutant`: one of
    MUTANTS - the error model stays the statement's own."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError("unknown mutant")
    s0, s1 = float(np.float32(s0)), float(np.float32(s1))
    w_hat = rne16(w.double())
    b = b.double()
    if upsample:
        x_src = x_hat
        x_hat = F.interpolate(x_hat, scale_factor=2, mode="nearest")
    z = F.conv2d(x_hat, w_hat, None, padding=1) + b[None, :, None, None]
    A = F.conv2d(x_hat.abs(), w_hat.abs(), None, padding=1) + b.abs()[None, :, None, None]
    if mutant in M.SUM:
        z = M.mutated_sum(x_hat, w_hat, mutant) + b[None, :, None, None]
    elif mutant in M.WEIGHTS:
        z = F.conv2d(x_hat, M.weights(w, mutant), None, padding=1) + b[None, :, None, None]
    elif mutant is not None and mutant.startswith("bias_roll_"):
        z = F.conv2d(x_hat, w_hat, None, padding=1) + b.roll(-int(mutant[10:]))[None, :, None, None]
    elif mutant == "ups_source_round_up" and upsample:
        rows = ((torch.arange(2 * x_src.shape[2]) + 1) >> 1).clamp(max=x_src.shape[2] - 1)
        z = F.conv2d(x_src[:, :, rows].repeat_interleave(2, dim=3), w_hat, None, padding=1) + b[None, :, None, None]
    elif mutant == "s0_s1_swapped":
        s0, s1 = s1, s0
    elif mutant == "r1_r2_swapped":
        r1, r2 = r2, r1
    v = torch.where(z > 0, z, 0.2 * z) if lrelu else z
    t1 = torch.zeros_like(z) if r1 is None else s1 * r1
    t2 = torch.zeros_like(z) if r2 is None else r2
    ref = s0 * v + t1 + t2
    K = 9 * x_hat.shape[1]
    e = abs(s0) * (K + 2) * U24 * A + 3 * U24 * ((s0 * v).abs() + t1.abs() + t2.abs())
    if mutant == "store_f16_trunc":
        ref = trunc16(ref)
    return ConvRef(ref, e)


def u8_ref(r: ConvRef, mutant=None):
    """(expected byte, mask of the elements that may differ by one) of the out_u8 epilogue, NCHW over 3 channels.
    `mutant`: "u8_half_up" (floor(q + 0.5)) or "u8_truncate" (floor(q)) in the place of half to even."""
    if mutant is not None and mutant not in U8_MUTANTS:
        raise ValueError("unknown mutant")
    q = 255.0 * r.ref[:, :3].clamp(0.0, 1.0)
    byte = M.round_u8(q, mutant)                                          # numpy rounds half to even
    frac = q - torch.floor(q)
    near = (frac - 0.5).abs() <= 255.0 * r.e[:, :3]
    return byte, near


def u8_inputs(cin, h, w, n, swap, res, seed=None):
    """Inputs of an out_u8 case, chosen so that few values lie within 255 e of a half-integer.  e grows with
    (9 cin + 2) * A, A = sum |x||w| + |b|, so A is kept near the size of the output itself: only `active` input channels
    are non-zero (A / |z| ~ 0.64 sqrt(9 active)), and where there is a residual the picture's level comes in through
    r2, which costs 3 * 2^-24 and not (K + 2) * 2^-24.  The output still spans [-0.2, 1.2], so both clamps are reached."""
    g = torch.Generator().manual_seed(cin + h + swap if seed is None else seed)
    active, z_std = (4, 0.1) if "2" in res else (2, 0.35)
    wt = torch.randn((3, cin, 3, 3), generator=g) * (z_std / math.sqrt(9 * active))
    b = torch.randn(3, generator=g) * 0.02 if "2" in res else torch.full((3,), 0.5) + torch.randn(3, generator=g) * 0.05
    x_h = torch.zeros((n, h, w, cin), dtype=torch.float16)
    x_h[..., :active] = torch.randn((n, h, w, active), generator=g).half()
    r1_h = (torch.randn((n, h, w, 32), generator=g) * 0.1).half() if "1" in res else None
    r2_h = (0.5 + torch.randn((n, h, w, 36), generator=g) * 0.35).half() if "2" in res else None
    return wt, b, x_h, r1_h, r2_h


U8_CASES = [(32, 9, 33, 2, 0, ""), (32, 17, 70, 1, 1, ""), (64, 8, 32, 1, 1, "2"), (64, 7, 31, 1, 0, "12")]


def nchw(t):
    """[n,h,w,c] -> float64 NCHW on the host."""
    return t.detach().cpu().permute(0, 3, 1, 2).double()


# ----------------------------------------------------------------------------------------------- layouts
def pack_ref(w: np.ndarray, cin: int, cout: int) -> np.ndarray:
    """fp32 OIHW [cout_real, cin_real, 3, 3] -> float16 [cin / 32, 9, cout, 32], zero padded:
    packed[kc, ky * 3 + kx, co, k] = f16(w[co, 32 kc + k, ky, kx])."""
    cout_real, cin_real = w.shape[:2]
    full = np.zeros((cout, cin, 3, 3), dtype=np.float32)
    full[:cout_real, :cin_real] = w
    p = full.reshape(cout, cin // 32, 32, 9)            # co, kc, k, tap
    return np.ascontiguousarray(p.transpose(1, 3, 0, 2)).astype(np.float16)


def input_ref(frames_u8: torch.Tensor, s: int, swap_rb: bool) -> torch.Tensor:
    """[n,h,w,3] uint8 -> float16 [n,ceil(h/s),ceil(w/s),32]: v / 255 in fp32, rounded to f16; s = 2: one reflected
    row / column for an odd size, then torch's pixel_unshuffle; channels past 3 s s are zero."""
    x = frames_u8.permute(0, 3, 1, 2).to(torch.float32)
    if swap_rb:
        x = x.flip(1)
    x = (x / np.float32(255.0)).to(torch.float16)
    if s == 2:
        n, c, h, w = x.shape
        x = F.pad(x.float(), (0, w % 2, 0, h % 2), mode="reflect").to(torch.float16)
        x = F.pixel_unshuffle(x.float(), 2).to(torch.float16)
    n, c, h, w = x.shape
    out = torch.zeros((n, h, w, 32), dtype=torch.float16)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out


# ----------------------------------------------------------------------------------------------- the network
def rrdbnet_ref(sd, scale: int, num_block: int, frames_u8: torch.Tensor, *, storage_f16: bool = False) -> torch.Tensor:
    """RRDBNet(3, 3, 64, num_block, 32, scale) on [n,h,w,3] uint8 frames (channel order as given; even sizes):
    [n,3,s h,s w] before `clamp(0, 1) * 255, round`.  float64, or with `storage_f16` fp32 arithmetic on f16-rounded
    weights with every tensor a module hands on rounded to f16."""
    dt = torch.float32 if storage_f16 else torch.float64
    q = (lambda t: t.to(torch.float16).to(dt)) if storage_f16 else (lambda t: t)
    W = lambda k: q(sd[k + ".weight"].to(dt))
    Bv = lambda k: sd[k + ".bias"].to(dt)
    conv = lambda k, t: F.conv2d(t, W(k), Bv(k), padding=1)
    lrelu = lambda t: F.leaky_relu(t, 0.2)
    x = q(frames_u8.permute(0, 3, 1, 2).to(dt) / 255.0)
    if scale == 2:
        x = F.pixel_unshuffle(x, 2)
    feat = q(conv("conv_first", x))
    body = feat
    for i in range(num_block):
        rrdb_in = body
        for r in (1, 2, 3):
            p = f"body.{i}.rdb{r}"
            xin = body
            x1 = q(lrelu(conv(p + ".conv1", xin)))
            x2 = q(lrelu(conv(p + ".conv2", torch.cat((xin, x1), 1))))
            x3 = q(lrelu(conv(p + ".conv3", torch.cat((xin, x1, x2), 1))))
            x4 = q(lrelu(conv(p + ".conv4", torch.cat((xin, x1, x2, x3), 1))))
            x5 = conv(p + ".conv5", torch.cat((xin, x1, x2, x3, x4), 1))
            body = q(x5 * 0.2 + xin)
        body = q(body * 0.2 + rrdb_in)
    feat = q(feat + conv("conv_body", body))
    feat = q(lrelu(conv("conv_up1", F.interpolate(feat, scale_factor=2, mode="nearest"))))
    feat = q(lrelu(conv("conv_up2", F.interpolate(feat, scale_factor=2, mode="nearest"))))
    return q(conv("conv_last", q(lrelu(conv("conv_hr", feat))))).double()


def to_bytes(out: torch.Tensor) -> torch.Tensor:
    """`enhance`'s quantisation: clamp to [0, 1], * 255, numpy's round (half to even) -> [n,h,w,3] int64."""
    return torch.from_numpy(np.round((out.clamp(0.0, 1.0) * 255.0).numpy())).to(torch.int64).permute(0, 2, 3, 1)
