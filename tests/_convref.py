"""float64 reference of the conv kernels with an explicit error model, and the case matrix of
tests/test_gpu_conv_matrix.py (importable without a GPU: the dispatch ledger and the mutation
self-test of tests/test_conv_ledger.py use it on the CPU).

The reference computes what the kernel is SPECIFIED to compute, from exactly the operands it
multiplies: x^ (the stored activation; with the fused prologue f16(silu(x*pa + pb)), nearest-repeated
with `upsample`) and w^ (f16(w); for PackedUpConv f16 of the fp32 tap sums in ops.py's order; fp32
for the fp32 and compensated paths).  z = sum x^*w^ + b in float64, y = act(z) + res.

Tier 1 (every element):  |y - ref| <= 1/2 ulp_out(|ref| + e) + e,  e = L*gamma*A + eps_act + L*P (+ x3)
Tier 2 (f16 outputs, a fraction >= TIER2_FLOOR of each case):  y == RNE16(act(t) + res) for some t in
[z - P - eta, z + P + eta],  eta = 2^-21 * A.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

TIER2_FLOOR = 0.998   # observed minimum 0.99933 over the matrix (f16 1x1 GELU, 512 threads)
U24 = 2.0 ** -24
# Relative error of the kernels' fp32 SiLU in the fused prologue (conv_kernels.inc prologue_dword_f16 /
# prologue_apply*): v_exp_f32 and v_rcp_f32 are ~1 ulp each; the folded -log2(e)*a, -log2(e)*b and the fma that forms
# u = -log2(e)*t add ~3 roundings of |x*a| + |b| (cancellation in t: hence the absolute part below); with the final
# multiply about 6-8 fp32 ulp in all, so 2^-19 leaves a factor ~4.
DELTA_PRO = 2.0 ** -19
# Lipschitz constants of the epilogue activations (0 none, 1 GELU(erf), 2 SiLU, 3 ReLU)
L_ACT = {0: 1.0, 1: 1.129, 2: 1.0999, 3: 1.0}
# common.h gelu_erf_f: A&S 7.1.26 erf (|err| <= 1.5e-7) times 0.5|z|, plus __expf / rcp / fp32 roundings (~2^-20 |z|);
# the epilogue SiLU v / (1 + expf(-v)): ~4 fp32 roundings (2^-20 |z| with margin)
EPS_ACT_REL = {0: 0.0, 1: 0.75e-7 + 2.0 ** -20, 2: 2.0 ** -20, 3: 0.0}


def act_f64(z: torch.Tensor, act: int) -> torch.Tensor:
    if act == 1:
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    if act == 2:
        return z * torch.sigmoid(z)
    if act == 3:
        return torch.clamp(z, min=0.0)
    return z


def _act_min(act):
    """(argmin, min) of the non-monotonic activations (GELU, SiLU), by golden-section search in float64."""
    lo, hi = -3.0, 0.0
    f = lambda v: float(act_f64(torch.tensor([v], dtype=torch.float64), act)[0])
    for _ in range(200):
        m1, m2 = lo + (hi - lo) * 0.382, lo + (hi - lo) * 0.618
        if f(m1) < f(m2):
            hi = m2
        else:
            lo = m1
    t = 0.5 * (lo + hi)
    return t, f(t)


ACT_MIN = {1: _act_min(1), 2: _act_min(2)}


def rne16(v: torch.Tensor) -> torch.Tensor:
    return v.to(torch.float16).to(torch.float64)


def trunc16(v: torch.Tensor) -> torch.Tensor:
    """f16 rounding toward zero (for the mutation self-test)."""
    r = rne16(v)
    over = r.abs() > v.abs()
    step = torch.nextafter(r.to(torch.float16), torch.zeros_like(r, dtype=torch.float16)).to(torch.float64)
    return torch.where(over, step, r)


def ulp16(v: torch.Tensor) -> torch.Tensor:
    a = v.abs().clamp(min=2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def ulp32(v: torch.Tensor) -> torch.Tensor:
    a = v.abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


# ----------------------------------------------------------------------------------------------- reference
@dataclass
class Ref:
    z: torch.Tensor          # sum x^ w^ + b (float64, NCHW)
    res: torch.Tensor        # residual added after the activation (zeros without one)
    A: torch.Tensor          # sum |x^||w^| + |b| + |res|
    P: torch.Tensor          # prologue term (computed from the f16 midpoints)
    X: torch.Tensor          # extra absolute term of the compensated (x3) paths
    kt: int                  # products per output (for gamma)
    act: int
    out_f16: bool

    @property
    def ref(self):
        return act_f64(self.z, self.act) + self.res

    def bound(self):
        L = L_ACT[self.act]
        gamma = (self.kt + 2) * U24
        e = L * gamma * self.A + EPS_ACT_REL[self.act] * self.z.abs() + L * self.P + self.X
        ulp = ulp16 if self.out_f16 else ulp32
        return 0.5 * ulp(self.ref.abs() + e) + e


def prologue_f64(x_stored, pa, pb, f16: bool):
    """x^ and the midpoint indicator of the fused GroupNorm-affine + SiLU prologue."""
    t = x_stored * pa[:, :, None, None] + pb[:, :, None, None]
    s = t * torch.sigmoid(t)
    tol = DELTA_PRO * (s.abs() + (x_stored * pa[:, :, None, None]).abs() + pb[:, :, None, None].abs())
    if not f16:   # fp32 tensors: the stored operand is the kernel's fp32 SiLU itself - every input carries the error
        return s, tol
    xh = rne16(s)
    # distance to the nearest f16 rounding midpoint: |s - (xh +- ulp/2)|
    u = ulp16(s)
    mid = torch.minimum((s - (xh + 0.5 * u)).abs(), (s - (xh - 0.5 * u)).abs())
    # a value this close to a midpoint may round the other way in the kernel: it can be off by one f16 ulp
    near = (mid <= tol).to(torch.float64) * ulp16(xh)
    return xh, near


def conv_ref(x_hat, w_hat, b, res, *, ksize, stride=1, pad=1, upsample=False, act=0, out_f16=True, pro_err=None,
             x3=False, kt=None, down_pad0=False):
    """Generic direct conv reference (PackedConv / PackedDownConv).  x_hat NCHW float64 (pre-upsample), w_hat OIHW."""
    if upsample:
        x_hat = F.interpolate(x_hat, scale_factor=2, mode="nearest")
        if pro_err is not None:
            pro_err = F.interpolate(pro_err, scale_factor=2, mode="nearest")
    if down_pad0:
        x_hat = F.pad(x_hat, (0, 1, 0, 1))
        pro_err = None if pro_err is None else F.pad(pro_err, (0, 1, 0, 1))
        pad = 0
    cv = lambda t, w: F.conv2d(t, w, None, stride=stride, padding=pad)
    z = cv(x_hat, w_hat) + (b[None, :, None, None] if b is not None else 0.0)
    res = torch.zeros_like(z) if res is None else res
    A = cv(x_hat.abs(), w_hat.abs()) + (b.abs()[None, :, None, None] if b is not None else 0.0) + res.abs()
    P = torch.zeros_like(z) if pro_err is None else cv(pro_err, w_hat.abs())
    X = x3_term(A, cv(x_hat.abs(), torch.ones_like(w_hat)), w_hat) if x3 else torch.zeros_like(z)
    kt = kt if kt is not None else w_hat.shape[1] * w_hat.shape[2] * w_hat.shape[3]
    return Ref(z, res, A, P, X, (4 if x3 else 1) * kt, act, out_f16)


def x3_term(A, sum_abs_x, w_hat):
    """Compensated f16 (x = hi + lo): the dropped lo*lo product and the rounding of lo (3 * 2^-22 relative), and lo
    below f16's normal range (absolute 2^-25 per lo, times the other operand)."""
    sum_abs_w = w_hat.abs().sum((1, 2, 3))[None, :, None, None]
    return 3 * 2.0 ** -22 * A + 2.0 ** -25 * (sum_abs_x + sum_abs_w)


def up_weights(w):
    """PackedUpConv's pre-summed 2x2 taps, fp32 sums in ops.py's order: [parity] -> (cout, cin, 2, 2) fp32."""
    rowsets = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}
    w = w.float()
    out = []
    for a in (0, 1):
        for bb in (0, 1):
            w2 = torch.zeros(w.shape[0], w.shape[1], 2, 2)
            for dyi, rows in enumerate(rowsets[a]):
                for dxi, cols in enumerate(rowsets[bb]):
                    w2[:, :, dyi, dxi] = sum(w[:, :, r, c] for r in rows for c in cols)
            out.append(w2)
    return out


def upconv_ref(x_hat, w2_hat, b, *, act=0, out_f16=True, x3=False):
    """The four sub-pixel parities of PackedUpConv, assembled to the 2h x 2w output."""
    n, cin, h, w = x_hat.shape
    cout = w2_hat[0].shape[0]
    parts = []
    for k, wk in enumerate(w2_hat):
        a, bb = k >> 1, k & 1
        r = conv_ref(x_hat, wk, b, None, ksize=2, pad=1, act=act, out_f16=out_f16, x3=x3)
        parts.append([t[..., a:a + h, bb:bb + w] for t in (r.z, r.res, r.A, r.P, r.X)])

    def assemble(i):
        o = torch.empty(n, cout, 2 * h, 2 * w, dtype=torch.float64)
        for k in range(4):
            o[..., k >> 1::2, k & 1::2] = parts[k][i]
        return o
    return Ref(assemble(0), assemble(1), assemble(2), assemble(3), assemble(4), (4 if x3 else 1) * 4 * cin, act, out_f16)


# ----------------------------------------------------------------------------------------------- checks
def tier1(y: torch.Tensor, r: Ref):
    """(all elements within the bound, worst ratio |y - ref| / bound, index of the worst element)."""
    err = (y - r.ref).abs()
    ratio = err / r.bound()
    ratio = torch.where(torch.isnan(y), torch.full_like(ratio, float("inf")), ratio)
    worst = float(ratio.max())
    return worst <= 1.0, worst, np.unravel_index(int(torch.argmax(ratio)), tuple(ratio.shape))


def tier2(y: torch.Tensor, r: Ref):
    """Fraction of the elements equal to RNE16(act(t) + res) for some t in [z - P - eta, z + P + eta]."""
    eta = 2.0 ** -21 * r.A
    lo, hi = r.z - r.P - eta, r.z + r.P + eta
    alo, ahi = act_f64(lo, r.act), act_f64(hi, r.act)
    vlo, vhi = torch.minimum(alo, ahi), torch.maximum(alo, ahi)
    if r.act in ACT_MIN:   # not monotonic below zero: the interval's image includes the minimum it straddles
        tmin, amin = ACT_MIN[r.act]
        vlo = torch.where((lo <= tmin) & (hi >= tmin), torch.full_like(vlo, amin), vlo)
    ok = (y >= rne16(vlo + r.res)) & (y <= rne16(vhi + r.res))
    return float(ok.double().mean())


def tile_stats_ref(y: torch.Tensor, ty: int, tx: int = 32, parity: Optional[int] = None):
    """float64 [tile][c][sum, sumsq, sum|v|, npx] of the stored output y (NCHW), tiles of ty x tx pixels in
    ((img * tiles_y + ty) * tiles_x + tx) order; `parity` (0..3): the sub-pixel grid of that parity."""
    if parity is not None:
        y = y[..., parity >> 1::2, parity & 1::2]
    n, c, h, w = y.shape
    tys, txs = -(-h // ty), -(-w // tx)
    yp = F.pad(y, (0, txs * tx - w, 0, tys * ty - h))
    blk = yp.reshape(n, c, tys, ty, txs, tx).permute(0, 2, 4, 1, 3, 5).reshape(n * tys * txs, c, ty * tx)
    npx = F.pad(torch.ones(1, 1, h, w, dtype=torch.float64), (0, txs * tx - w, 0, tys * ty - h)).reshape(
        tys, ty, txs, tx).sum((1, 3)).reshape(-1).repeat(n)
    return torch.stack([blk.sum(-1), (blk * blk).sum(-1), blk.abs().sum(-1),
                        npx[:, None].expand(-1, c)], -1)


def stats_check(got: torch.Tensor, ref: torch.Tensor):
    """Per-tile partials vs float64 sums of the stored pixels: |got - ref| <= Npx * 2^-24 * sum|v| (sum v^2 for the
    second).  Returns (ok, worst ratio)."""
    npx = ref[..., 3]
    b0 = npx * U24 * ref[..., 2] + 1e-30
    b1 = npx * U24 * ref[..., 1] + 1e-30
    r0 = (got[..., 0].double() - ref[..., 0]).abs() / b0
    r1 = (got[..., 1].double() - ref[..., 1]).abs() / b1
    worst = float(torch.maximum(r0, r1).max()) if got.numel() else 0.0
    return worst <= 1.0 and got.shape[:2] == ref.shape[:2], worst


# ----------------------------------------------------------------------------------------------- kernel names
_TOK = {"DF16_": "half", "f": "float"}


def demangle_conv(sym: str) -> Optional[str]:
    """`_ZN12_GLOBAL__N_119conv3x3_halo_kernelIDF16_Li128ELi256ELi8ELb1ELi3ELb0EEEv...` ->
    `conv3x3_halo_kernel<half,128,256,8,true,3,false>` (the form the name query and rocprofv3 print); None for other
    symbols."""
    import re
    m = re.match(r"_ZN12_GLOBAL__N_1\d+((?:conv3x3_halo|conv3x3_halo_x3|conv3x3_x3p|conv3x3_ws|conv_igemm)_kernel)I(.*?)EEv", sym)
    if not m:
        return None
    args, s = [], m.group(2)
    while s:
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
    return f"{m.group(1)}<{','.join(args)}>"


def elf_symbols(path: str):
    """Names in the ELF64 little-endian .symtab (and .dynsym) of `path` - no external tool."""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:4] == b"\x7fELF" and data[4] == 2 and data[5] == 1, "expected an ELF64 little-endian file"
    e_shoff, = struct.unpack_from("<Q", data, 0x28)
    e_shentsize, e_shnum = struct.unpack_from("<HH", data, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", data, e_shoff + i * e_shentsize) for i in range(e_shnum)]
    names = set()
    for s in secs:
        if s[1] not in (2, 11):   # SHT_SYMTAB, SHT_DYNSYM
            continue
        off, size, link, entsize = s[4], s[5], s[6], s[9]
        stroff = secs[link][4]
        for i in range(size // entsize):
            st_name, = struct.unpack_from("<I", data, off + i * entsize)
            if st_name:
                end = data.index(b"\0", stroff + st_name)
                names.add(data[stroff + st_name:end].decode("ascii", "replace"))
    return names


def normalize_kernel_name(name: str) -> str:
    """rocprofv3 / demangler spellings -> the name query's: drop `(anonymous namespace)::`, the argument list,
    spaces, and spell _Float16 as half.  A name the tool left mangled (it cannot demangle _Float16) is decoded here."""
    if name.startswith("_Z"):
        return demangle_conv(name) or name
    name = name.replace("(anonymous namespace)::", "").replace(" ", "")
    if name.endswith(")"):
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += {")": 1, "(": -1}.get(name[i], 0)
            if depth == 0:
                name = name[:i]
                break
    name = name.replace("_Float16", "half").replace("__fp16", "half")
    if name.startswith("void"):
        name = name[4:]
    return name


# ----------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    id: str
    expect: str                   # kernel instantiation the case must reach (name query)
    kind: str = "conv"            # conv | up | down
    dt: str = "f16"               # f16 | f32 | x3
    cin: int = 64
    cin2: int = 0
    cout: int = 64
    n: int = 1
    h: int = 16
    w: int = 40
    ksize: int = 3
    upsample: bool = False
    prologue: bool = False
    act: int = 0
    residual: bool = False
    res_pitch_extra: int = 0      # residual pitch = pitch_for(cout) + this
    stats: bool = False
    pad1: bool = False            # down: the pad-1 form
    stride: int = 1
    pad: Optional[int] = None
    ho: Optional[int] = None
    wo: Optional[int] = None
    seed: int = 0
    notes: str = ""

    @property
    def pitch_out(self):
        return (self.cout + 7) // 8 * 8


def _pitch(c):
    return (c + 7) // 8 * 8


def descs(c: Case):
    """(elvis_conv_desc fields, has_residual, has_stats) for every elvis_conv2d call the case makes, as ops builds them."""
    from elvis_amd import _lib as L
    dcode = {"f16": L.F16, "f32": L.F32, "x3": 2}[c.dt]
    cout_k = (c.cout + 3) // 4 * 4
    out = []
    if c.kind == "conv":
        d = L.ConvDesc()
        d.dtype = dcode
        d.n, d.h, d.w = c.n, c.h, c.w
        d.cin, d.cin_pitch = c.cin, _pitch(c.cin)
        d.cin2, d.cin2_pitch = c.cin2, (_pitch(c.cin2) if c.cin2 else 0)
        d.ksize, d.stride, d.upsample, d.act = c.ksize, c.stride, int(c.upsample), c.act
        d.pad_before = (c.ksize // 2) if c.pad is None else c.pad
        lh, lw = (2 * c.h, 2 * c.w) if c.upsample else (c.h, c.w)
        d.ho = c.ho if c.ho is not None else (lh + 2 * d.pad_before - c.ksize) // c.stride + 1
        d.wo = c.wo if c.wo is not None else (lw + 2 * d.pad_before - c.ksize) // c.stride + 1
        d.cout, d.cout_pitch = cout_k, c.pitch_out
        d.prologue = int(c.prologue)
        out.append((d, c.residual, c.stats))
    elif c.kind == "up":
        for k in range(4):
            d = L.ConvDesc()
            d.dtype = dcode
            d.n, d.h, d.w = c.n, c.h, c.w
            d.cin, d.cin_pitch = c.cin, _pitch(c.cin)
            d.ksize, d.stride, d.subpixel, d.act = 2, 1, 1 + k, c.act
            d.ho, d.wo = 2 * c.h, 2 * c.w
            d.cout, d.cout_pitch = cout_k, c.pitch_out
            out.append((d, False, c.stats))
    else:
        d = L.ConvDesc()
        d.dtype = dcode
        d.n, d.h, d.w, d.ho, d.wo = c.n, c.h, c.w, c.h // 2, c.w // 2
        d.cin, d.cin_pitch = 4 * c.cin, _pitch(c.cin)
        d.cout, d.cout_pitch = c.cout, c.pitch_out
        d.ksize, d.stride, d.subpixel = 2, 1, 5
        d.pad_before = 1 if c.pad1 else 0
        d.act = c.act
        out.append((d, False, c.stats))
    return out


def resolve(c: Case):
    """Kernel names the case's calls resolve to through the library's name query (no GPU needed)."""
    import ctypes as C
    from elvis_amd._lib import lib, check
    names = []
    for d, res, st in descs(c):
        buf = C.create_string_buffer(128)
        check(lib().elvis_conv_kernel_name_for_call(C.byref(d), int(res), int(st), buf, len(buf)), None)
        names.append(buf.value.decode())
    return names


def kernel_ty(name: str) -> int:
    """Tile rows of a halo-family instantiation, read from its template arguments."""
    args = name[name.index("<") + 1:-1].split(",")
    if name.startswith("conv3x3_halo_kernel"):
        return int(args[3])
    return int(args[1])   # conv3x3_halo_x3_kernel<TCO,TY,..> / conv3x3_x3p_kernel<TCO,TY,..>


def _halo(t, tco, nt, ty, pro, ks, act):
    b = lambda v: "true" if v else "false"
    return f"conv3x3_halo_kernel<{t},{tco},{nt},{ty},{b(pro)},{ks},{b(act)}>"


def _x3(tco, ty, pro, ks, act):
    b = lambda v: "true" if v else "false"
    return f"conv3x3_halo_x3_kernel<{tco},{ty},{b(pro)},{ks},{b(act)}>"


def _x3p(tco, ty, ks, pro, act):
    b = lambda v: "true" if v else "false"
    return f"conv3x3_x3p_kernel<{tco},{ty},{ks},{b(pro)},{b(act)}>"


def _build_cases():
    C_ = []
    add = lambda **kw: C_.append(Case(**kw))
    ACTS = (1, 2, 3)   # GELU, SiLU, ReLU rotate over the ACT=true leaves
    # ---- f16 256-thread halo kernels: 128 / 64 channels, KS 3 / 2 / 1, PRO false / true, ACT false / true
    for tco, cout in ((128, 128), (64, 96)):
        for act in (0, 1):
            a = ACTS[(tco // 64 + act) % 3] if act else 0
            tag = f"f16_{tco}"
            # 3x3, no prologue: interior + ragged edges (LEAN and general epilogue), n = 2, residual with pitch > cout, stats
            add(id=f"{tag}_ks3_a{a}", expect=_halo("half", tco, 256, 8, False, 3, act), cin=40, cout=cout, n=2, h=19, w=70,
                act=a, residual=True, res_pitch_extra=8, stats=True)
            # 3x3 + prologue, virtual concat
            add(id=f"{tag}_ks3_pro_a{a}", expect=_halo("half", tco, 256, 8, True, 3, act), cin=32, cin2=24, cout=cout, n=2,
                h=17, w=40, prologue=True, act=a, stats=True)
            # sub-pixel 2x2: PackedUpConv, n = 3 (statistics reorder)
            add(id=f"{tag}_up_a{a}", expect=_halo("half", tco, 256, 8, False, 2, act), kind="up", cin=48, cout=cout, n=3,
                h=9, w=37, act=a, stats=True)
            # 1x1 (g1 path), ragged edges, cin % 32 == 0
            add(id=f"{tag}_ks1_a{a}", expect=_halo("half", tco, 256, 8, False, 1, act), ksize=1, cin=64, cout=cout, n=2,
                h=13, w=45, act=a, residual=True, stats=True)
    # ragged cout through the sub-pixel kernel with statistics (the PackedUpConv row-stride fix), padded cout 160 -> 192
    add(id="f16_up_ragged_cout", expect=_halo("half", 64, 256, 8, False, 2, False), kind="up", cin=32, cout=70, n=2, h=8,
        w=40, stats=True)
    add(id="f16_160_to_192", expect=_halo("half", 64, 256, 8, False, 3, False), cin=64, cout=160, n=1, h=16, w=33,
        stats=True, residual=True)
    add(id="f16_upsample_fused", expect=_halo("half", 64, 256, 8, True, 3, False), cin=64, cout=64, h=7, w=21,
        upsample=True, prologue=True, stats=True)
    add(id="f16_small_image", expect=_halo("half", 128, 256, 8, False, 3, False), cin=32, cout=128, n=2, h=5, w=11, stats=True)
    # ---- tall 64-channel tile (>= 128 K pixels per image): with the prologue, and a single K chunk without it
    add(id="f16_tall_pro", expect=_halo("half", 64, 256, 16, True, 3, False), cin=32, cout=64, n=1, h=72, w=1920,
        prologue=True, stats=True)
    add(id="f16_tall_pro_act", expect=_halo("half", 64, 256, 16, True, 3, True), cin=32, cout=64, n=1, h=70, w=1900,
        prologue=True, act=2)
    add(id="f16_tall_1chunk", expect=_halo("half", 64, 256, 16, False, 3, False), cin=24, cout=189, n=1, h=69, w=1920,
        residual=True, stats=True)
    add(id="f16_tall_1chunk_act", expect=_halo("half", 64, 256, 16, False, 3, True), cin=32, cout=64, n=1, h=68, w=1930,
        act=1, stats=True)
    # ---- 512-thread f16: 32 / 16 channel tiles (KS 3 / 2 / 1, PRO, ACT)
    for tco, cout in ((32, 32), (16, 3)):
        for act in (0, 3):
            add(id=f"f16_{tco}_ks3_a{act}", expect=_halo("half", tco, 512, 8, False, 3, act), cin=40, cout=cout, n=2, h=17,
                w=70, act=act, residual=True)
            add(id=f"f16_{tco}_ks3_pro_a{act}", expect=_halo("half", tco, 512, 8, True, 3, act), cin=64, cout=cout, h=9,
                w=33, prologue=True, act=act)
            add(id=f"f16_{tco}_ks1_a{act}", expect=_halo("half", tco, 512, 8, False, 1, act), ksize=1, cin=48, cout=cout,
                h=16, w=20, act=act)
        add(id=f"f16_{tco}_up", expect=_halo("half", tco, 512, 8, False, 2, False), kind="up", cin=32, cout=cout, n=2, h=8,
            w=20)
        add(id=f"f16_{tco}_up_act", expect=_halo("half", tco, 512, 8, False, 2, True), kind="up", cin=32, cout=cout, h=8,
            w=20, act=1)
    # ---- 512-thread f16 halo kernels the 256-thread variant cannot hold (prologue table over ~43 / 71 K chunks)
    add(id="f16_128_512_pro", expect=_halo("half", 128, 512, 12, True, 3, False), cin=1408, cout=128, h=13, w=33,
        prologue=True, stats=True)
    add(id="f16_128_512_pro_act", expect=_halo("half", 128, 512, 12, True, 3, True), cin=1408, cout=128, h=12, w=32,
        prologue=True, act=3)
    add(id="f16_1x1_512_cin_ragged", expect=_halo("half", 128, 512, 8, False, 1, False), ksize=1, cin=40, cout=128, n=2,
        h=13, w=40, stats=True)
    add(id="f16_1x1_512_cin_ragged_act", expect=_halo("half", 64, 512, 8, False, 1, True), ksize=1, cin=40, cout=64,
        h=16, w=16, act=1)
    add(id="f16_1x1_512_64", expect=_halo("half", 64, 512, 8, False, 1, False), ksize=1, cin=24, cout=64, n=2, h=9,
        w=35, residual=True, stats=True)
    add(id="f16_1x1_512_128_act", expect=_halo("half", 128, 512, 8, False, 1, True), ksize=1, cin=56, cout=128, h=16,
        w=20, act=2)
    # 64-channel tile + prologue over more than ~139 K chunks: the 256-thread variant's LDS cannot hold the table
    add(id="f16_64_512_pro", expect=_halo("half", 64, 512, 8, True, 3, False), cin=4480, cout=64, h=8, w=32,
        prologue=True, stats=True)
    add(id="f16_64_512_pro_act", expect=_halo("half", 64, 512, 8, True, 3, True), cin=4480, cout=64, h=8, w=20,
        prologue=True, act=1)
    # ---- weight-stationary kernel (>= 128 K pixels per image, narrow f16 3x3)
    for nkc, cin in ((1, 24), (2, 64)):
        for tco, cout in ((16, 16), (32, 32), (64, 64)):
            stag = nkc == 2 and tco == 64
            act = 3 if (tco == 32) else 0
            add(id=f"ws_{nkc}_{tco}", expect=f"conv3x3_ws_kernel<{nkc},{tco},{'true' if stag else 'false'}>", cin=cin,
                cout=cout, h=70, w=1900 if nkc == 1 else 1920, act=act)
    # the same ws-eligible shape with a residual / with statistics: the halo kernel
    add(id="ws_shape_residual", expect=_halo("half", 32, 512, 8, False, 3, False), cin=32, cout=32, h=70, w=1900, residual=True)
    add(id="ws_shape_stats", expect=_halo("half", 64, 256, 16, False, 3, False), cin=32, cout=64, h=72, w=1920, stats=True)
    # ---- generic implicit-GEMM kernel: stride 2 and 1x1 on fewer than 256 pixels, all four tile ids
    for dt in ("f16", "f32"):
        t = "half" if dt == "f16" else "float"
        add(id=f"igemm_{dt}_s2_t0", expect=f"conv_igemm_kernel<{t},4,4,2,2>", dt=dt, cin=40, cout=128, n=2, h=17, w=23,
            stride=2)
        add(id=f"igemm_{dt}_s2_t1", expect=f"conv_igemm_kernel<{t},4,2,1,4>", dt=dt, cin=64, cout=70, h=16, w=18, stride=2,
            pad=0, ho=8, wo=9, residual=True)
        add(id=f"igemm_{dt}_1x1_t2", expect=f"conv_igemm_kernel<{t},2,4,1,4>", dt=dt, ksize=1, cin=48, cout=32, n=3, h=9,
            w=13, act=1)
        add(id=f"igemm_{dt}_1x1_t3", expect=f"conv_igemm_kernel<{t},1,4,1,4>", dt=dt, ksize=1, cin=24, cout=3, h=7, w=11)
    # ---- fp32 (exact MFMA) halo kernels: 128 / 64 / 32 / 16 channels, TY 12 prologue tile
    for tco, cout in ((128, 128), (64, 72), (32, 32), (16, 16)):
        for act in (0, 2):
            ty3 = 16 if tco >= 64 else 8
            add(id=f"f32_{tco}_ks3_a{act}", expect=_halo("float", tco, 512, ty3, False, 3, act), dt="f32", cin=24, cout=cout,
                n=2, h=19, w=40, act=act, residual=True, stats=tco >= 64)
            typ = 12 if tco == 128 else 8
            add(id=f"f32_{tco}_ks3_pro_a{act}", expect=_halo("float", tco, 512, typ, True, 3, act), dt="f32", cin=16,
                cin2=8, cout=cout, h=13, w=35, prologue=True, act=act, stats=tco >= 64)
            add(id=f"f32_{tco}_ks1_a{act}", expect=_halo("float", tco, 512, 8, False, 1, act), dt="f32", ksize=1, cin=20,
                cout=cout, h=16, w=20, act=act)
            add(id=f"f32_{tco}_up_a{act}", expect=_halo("float", tco, 512, 16 if tco >= 64 else 8, False, 2, act), dt="f32",
                kind="up", cin=16, cout=cout, h=8, w=20, act=act)
    # ---- compensated fp32 (x3): planar 3x3 / sub-pixel, interleaved for the rest
    for tco, cout, ty in ((128, 128, 12), (64, 64, 16)):
        for act in (0, 1):
            add(id=f"x3p_{tco}_ks3_a{act}", expect=_x3p(tco, ty, 3, False, act), dt="x3", cin=40, cout=cout, n=2, h=19,
                w=40, act=act, residual=True, stats=True)
            add(id=f"x3p_{tco}_pro_a{act}", expect=_x3p(tco, ty, 3, True, act), dt="x3", cin=32, cout=cout, h=17, w=35,
                prologue=True, act=act, stats=True)
            add(id=f"x3p_{tco}_up_a{act}", expect=_x3p(tco, ty, 2, False, act), dt="x3", kind="up", cin=32, cout=cout, n=3,
                h=9, w=20, act=act, stats=True)
            # interleaved form: a virtual concat with cin % 32 != 0 (no planar packing), 1x1
            add(id=f"x3_{tco}_cat_a{act}", expect=_x3(tco, 16, False, 3, act), dt="x3", cin=16, cin2=8, cout=cout, n=2,
                h=17, w=40, act=act, residual=True, stats=True)
            add(id=f"x3_{tco}_cat_pro_a{act}", expect=_x3(tco, 12 if tco == 128 else 8, True, 3, act), dt="x3", cin=16,
                cin2=24, cout=cout, h=9, w=35, prologue=True, act=act, stats=True)
            add(id=f"x3_{tco}_ks1_a{act}", expect=_x3(tco, 8, False, 1, act), dt="x3", ksize=1, cin=24, cout=cout, h=16,
                w=20, act=act)
    # ---- space to depth (PackedDownConv): pad 0 and pad 1 in f16, and in x3
    add(id="s2d_f16_pad0", expect=_halo("half", 128, 256, 8, False, 2, False), kind="down", cin=32, cout=128, n=2, h=18,
        w=70, stats=True)
    add(id="s2d_f16_pad1", expect=_halo("half", 64, 256, 8, False, 2, False), kind="down", cin=32, cout=96, h=16, w=66,
        pad1=True, stats=True)
    add(id="s2d_f16_pad1_32", expect=_halo("half", 32, 512, 8, False, 2, False), kind="down", cin=32, cout=32, h=16, w=40,
        pad1=True)
    add(id="s2d_x3_pad0", expect=_x3p(128, 12, 2, False, False), kind="down", dt="x3", cin=32, cout=128, h=18, w=40,
        stats=True)
    add(id="s2d_x3_pad0_il", expect=_x3(64, 16, False, 2, False), kind="down", dt="x3", cin=16, cout=64, h=18, w=40)
    for cout, act in ((128, 0), (128, 1), (64, 1)):
        add(id=f"s2d_x3_il_{cout}_a{act}", expect=_x3(cout, 16, False, 2, act), kind="down", dt="x3", cin=16, cout=cout,
            n=2, h=18, w=70, act=act, stats=act == 0)
    return C_


CASES = _build_cases()
