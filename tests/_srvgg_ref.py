"""float64 statements of what csrc/srvgg.hip and elvis_amd/srvgg.py are specified to compute, written from the
architecture (SRVGGNetCompact as Real-ESRGAN defines it and RealESRGANer.enhance drives it), importable without a GPU.

1. `srvgg_ref`: the network.  float64 throughout, or (`storage_f16=True`) the same statement in fp32 arithmetic with
   every stored activation and every conv weight rounded to f16 (the PReLU slopes and the biases stay fp32, as on the
   device) - what f16 storage alone costs, the yardstick of the model tests.
2. `conv_ref`: one `elvis_srvgg_conv3x3` call, from exactly the operands the kernel multiplies - x^ (the stored f16
   activation), w^ = f16(w), and the fp32 bias b and slopes a:
       z = sum x^ w^ + b;   ref = z > 0 ? z : a[c] z
       A = sum |x^||w^| + |b|
       e = max(1, |a[c]|) (K + 2) 2^-24 A  +  2^-24 |ref|
       |y - ref| <= 1/2 ulp16(|ref| + e) + e
   Term by term.  K = 9 cin products, each exact in fp32 (f16 x f16), are summed in fp32 in the matrix unit in an order
   the test does not know: any order of K - 1 additions is within (K - 1) 2^-24 A of the exact sum to first order; the
   bias addition is one more rounding of at most 2^-24 A; two spare units of 2^-24 A cover the second order.  PReLU is
   continuous and piecewise linear with slopes 1 and a[c], so it carries an error of z into at most max(1, |a[c]|)
   times as much, whichever side of zero the computed z falls on; its one multiplication a[c] * z rounds once more,
   2^-24 |ref| (on the positive side there is no multiplication and the term is spare).  The stored f16 is the nearest
   to the fp32 y: half an ulp of a value within e of ref.
3. `tail_ref`: one `elvis_srvgg_tail` call:
       z = sum x^ w^ + b;   ref[c, 4y + dy, 4x + dx] = z[16c + 4dy + dx, y, x] + base^[c, y, x]
       e = (K + 2) 2^-24 A  +  2^-24 (|z| + |base^|)
   the same sum and bias, then one addition of the stored f16 base, whose rounding is at most 2^-24 |ref| <=
   2^-24 (|z| + |base^|).  Float mode stores the nearest f16: |y - ref| <= 1/2 ulp16(|ref| + e) + e.
4. u8 mode (`u8_ref`): the byte is round_half_even(255 clamp(y, 0, 1)) computed from the fp32 y; the multiplication
   by 255 rounds once more, at most 2^-24 of a value in [0, 1].  With e8 = e + 2^-24 the byte may differ from
   round_half_even(255 clamp(ref)) by one, and only where 255 clamp(ref) lies within 255 e8 of a half-integer.
5. `pack_ref`: the packed weight layout - elvis_rrdb_pack_weights' layout, with cout = 48 admitted.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

import _srmut as M
from _convref import U24, rne16, trunc16, ulp16


# ----------------------------------------------------------------------------------------------- one call
class ConvRef:
    def __init__(self, ref, e):
        self.ref, self.e = ref, e

    def bound(self):
        return 0.5 * ulp16(self.ref.abs() + self.e) + self.e


# The statement with one clause changed (tests/test_sr_ledger.py: each must move a named case of tests/_srcases.py past
# the bound).  The sum's mutants are those of tests/_srmut.py; the others:
#   bias_roll_1 / _4 / _16    the bias of the neighbouring channel, lane group (4 channels) or accumulator (16)
#   slope_roll_1 / _4 / _16   the same for the PReLU slope (the layer)
#   shuffle_dy_dx             channel 16c + 4dy + dx goes to (4y + dx, 4x + dy) (the tail)
#   base_left                 the base of the pixel to the left, the first column its own (the tail)
#   base_not_swapped          under swap_rb the base keeps its order while the conv's channels are exchanged: in the RGB
#                             order `tail_ref` speaks, the base's channels reversed (the tail)
#   store_f16_trunc           the f16 store rounds toward zero: `ref` is then the stored value itself
_BIAS = ("bias_roll_1", "bias_roll_4", "bias_roll_16")
CONV_MUTANTS = M.SUM + M.WEIGHTS + _BIAS + ("slope_roll_1", "slope_roll_4", "slope_roll_16", "store_f16_trunc")
TAIL_MUTANTS = M.SUM + M.WEIGHTS + _BIAS + ("shuffle_dy_dx", "base_left", "base_not_swapped", "store_f16_trunc")
U8_MUTANTS = ("u8_half_up", "u8_truncate")


def _sum(x_hat, w, b, mutant=None):
    w_hat = rne16(w.double())
    b = b.double()
    z = F.conv2d(x_hat, w_hat, None, padding=1) + b[None, :, None, None]
    A = F.conv2d(x_hat.abs(), w_hat.abs(), None, padding=1) + b.abs()[None, :, None, None]
    if mutant in M.SUM:
        z = M.mutated_sum(x_hat, w_hat, mutant) + b[None, :, None, None]
    elif mutant in M.WEIGHTS:
        z = F.conv2d(x_hat, M.weights(w, mutant), None, padding=1) + b[None, :, None, None]
    elif mutant in _BIAS:
        z = F.conv2d(x_hat, w_hat, None, padding=1) + b.roll(-int(mutant[10:]))[None, :, None, None]
    return z, A, 9 * x_hat.shape[1]


def conv_ref(x_hat, w, b, slope, mutant=None) -> ConvRef:
    """x_hat NCHW float64 (the stored f16 values), w OIHW fp32 (rounded to f16 here), b and slope fp32 [64].  `mutant`:
    one of CONV_MUTANTS - the error model stays the statement's own."""
    if mutant is not None and mutant not in CONV_MUTANTS:
        raise ValueError("unknown mutant")
    z, A, K = _sum(x_hat, w, b, mutant)
    a = slope.double()[None, :, None, None]
    ref = torch.where(z > 0, z, a * z)
    e = a.abs().clamp(min=1.0) * (K + 2) * U24 * A + U24 * ref.abs()
    if mutant is not None and mutant.startswith("slope_roll_"):
        ref = torch.where(z > 0, z, a.roll(-int(mutant[11:]), 1) * z)
    elif mutant == "store_f16_trunc":
        ref = trunc16(ref)
    return ConvRef(ref, e)


def shuffle4(z):
    """[n,48,h,w] -> [n,3,4h,4w], channel 16c + 4dy + dx to (c, 4y + dy, 4x + dx), written out index by index."""
    n, _, h, w = z.shape
    out = z.new_zeros((n, 3, 4 * h, 4 * w))
    for c in range(3):
        for dy in range(4):
            for dx in range(4):
                out[:, c, dy::4, dx::4] = z[:, 16 * c + 4 * dy + dx]
    return out


def nearest4(t):
    return t.repeat_interleave(4, dim=2).repeat_interleave(4, dim=3)


def tail_ref(x_hat, w, b, base_hat, mutant=None) -> ConvRef:
    """x_hat NCHW float64 [n,64,h,w], w OIHW fp32 [48,64,3,3], b fp32 [48], base_hat NCHW float64 [n,3,h,w] (the stored
    f16 values): [n,3,4h,4w] in RGB order (no swap).  `mutant`: one of TAIL_MUTANTS - the error model stays the
    statement's own."""
    if mutant is not None and mutant not in TAIL_MUTANTS:
        raise ValueError("unknown mutant")
    z, A, K = _sum(x_hat, w, b, mutant)
    zs, As, bs = shuffle4(z), shuffle4(A), nearest4(base_hat)
    e = (K + 2) * U24 * As + U24 * (zs.abs() + bs.abs())
    if mutant == "shuffle_dy_dx":
        zs = shuffle4(z.reshape(z.shape[0], 3, 4, 4, *z.shape[2:]).transpose(2, 3).reshape(z.shape))
    elif mutant == "base_left":
        bs = nearest4(torch.cat((base_hat[..., :1], base_hat[..., :-1]), -1))
    elif mutant == "base_not_swapped":
        bs = nearest4(base_hat.flip(1))
    ref = zs + bs
    if mutant == "store_f16_trunc":
        ref = trunc16(ref)
    return ConvRef(ref, e)


def u8_ref(r: ConvRef, mutant=None):
    """(expected byte, mask of the elements that may differ by one) of the u8 mode, [n,3,4h,4w].  `mutant`: "u8_half_up"
    (floor(q + 0.5)) or "u8_truncate" (floor(q)) in the place of half to even."""
    if mutant is not None and mutant not in U8_MUTANTS:
        raise ValueError("unknown mutant")
    q = 255.0 * r.ref.clamp(0.0, 1.0)
    byte = M.round_u8(q, mutant)                                          # numpy rounds half to even
    frac = q - torch.floor(q)
    near = (frac - 0.5).abs() <= 255.0 * (r.e + U24)
    return byte, near


# (h, w, n, swap_rb, base pitch) of the u8 device cases
U8_CASES = [(9, 33, 2, 0, 3), (17, 70, 1, 1, 5), (8, 32, 1, 1, 32), (7, 31, 1, 0, 4), (1, 1, 2, 1, 8)]


def u8_inputs(h, w, n, swap, base_pitch, seed=None):
    """Inputs of a u8 case, chosen so that few values lie within 255 e8 of a half-integer.  e grows with
    (9 * 64 + 2) * A, A = sum |x||w| + |b|, so A is kept near the size of the conv's own output: only two input channels
    are non-zero (A / |z| ~ 0.64 sqrt(18)), the conv's output is small (std 0.1) and the picture's level comes in
    through the base, which costs 2^-24 and not (K + 2) * 2^-24.  The sum still spans about [-0.3, 1.3], so both clamps
    are reached.  The one-pixel case has too few elements for random values to reach anything: its base is set by hand."""
    g = torch.Generator().manual_seed(1000 * h + 10 * w + swap if seed is None else seed)
    active, z_std = 2, 0.1
    wt = torch.randn((48, 64, 3, 3), generator=g) * (z_std / math.sqrt(9 * active))
    b = torch.randn(48, generator=g) * 0.02
    x_h = torch.zeros((n, h, w, 64), dtype=torch.float16)
    x_h[..., :active] = torch.randn((n, h, w, active), generator=g).half()
    base_h = (0.5 + torch.randn((n, h, w, base_pitch), generator=g) * 0.4).half()
    if h * w == 1:
        base_h[0, 0, 0, :3] = torch.tensor([-2.0, 3.0, 0.5]).half()
        base_h[1, 0, 0, :3] = torch.tensor([2.0, 0.25, -3.0]).half()
    return wt, b, x_h, base_h


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


# ----------------------------------------------------------------------------------------------- the network
def srvgg_ref(sd, num_conv: int, frames_u8: torch.Tensor, *, storage_f16: bool = False) -> torch.Tensor:
    """SRVGGNetCompact(3, 3, 64, num_conv, 4, 'prelu') on [n,h,w,3] uint8 frames (channel order as given):
    [n,3,4h,4w] before `clamp(0, 1) * 255, round`.  float64, or with `storage_f16` fp32 arithmetic on f16-rounded conv
    weights with every tensor a layer hands on rounded to f16."""
    dt = torch.float32 if storage_f16 else torch.float64
    q = (lambda t: t.to(torch.float16).to(dt)) if storage_f16 else (lambda t: t)
    x = q(frames_u8.permute(0, 3, 1, 2).to(dt) / 255.0)
    feat = x
    for i in range(num_conv + 1):
        z = F.conv2d(feat, q(sd[f"body.{2 * i}.weight"].to(dt)), sd[f"body.{2 * i}.bias"].to(dt), padding=1)
        a = sd[f"body.{2 * i + 1}.weight"].to(dt)[None, :, None, None]
        feat = q(torch.where(z > 0, z, a * z))
    k = 2 * num_conv + 2
    z = F.conv2d(feat, q(sd[f"body.{k}.weight"].to(dt)), sd[f"body.{k}.bias"].to(dt), padding=1)
    return q(shuffle4(z) + nearest4(x)).double()


def to_bytes(out: torch.Tensor) -> torch.Tensor:
    """`enhance`'s quantisation: clamp to [0, 1], * 255, numpy's round (half to even) -> [n,h,w,3] int64."""
    return torch.from_numpy(np.round((out.clamp(0.0, 1.0) * 255.0).numpy())).to(torch.int64).permute(0, 2, 3, 1)
