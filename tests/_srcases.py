"""The edge matrix of csrc/rrdb.hip and csrc/srvgg.hip (the 8 x 32 MFMA tile of csrc/sr_conv3x3.h under four epilogues, and
the uint8 input stage), importable without a GPU: the case list, the inputs, the expected values by the float64
statements tests/_rrdb_ref.py and tests/_srvgg_ref.py, and the mutants - a statement with one clause changed, each mapped
to one case that tests/test_gpu_sr_matrix.py runs and that tests/test_sr_ledger.py holds to move past the bound.

Groups:
  shapes   EDGE_SIZES: the image edge on, one before and one after the seam of a tile's two 16-column fragments
           (w % 32 in 15, 16, 17), one tile column under several tile rows and the reverse, one row wider than two tiles.
           Random operands, the statements' own bounds, launched twice.  The u8 forms take the `u8_inputs` recipes.
  exact    small integers: every value exact in fp32 and in f16, compared for equality.
  values   9 x 33: f16 subnormal activations (`sub_x`), f16 subnormal weights (`sub_w`), sums past 65504 (`sat`), -0.0
           activations under a zero bias (`zeros`).  Each condition is asserted from the statement alone (`value_facts`).
  ties     y = float32((m + 0.5) / 255): float32(y * 255) is m + 0.5 exactly for every m in 0..254 (asserted below), so the
           byte says how the epilogue rounds a tie.  Equality, no `near` mask.
  input    rrdb_input_u8_kernel on the same sizes, bit for bit against `input_ref`.

SR_TY, SR_TX and SR_KC are the header's (tests/_srmut.py reads them)."""
import math
import zlib
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional

import numpy as np
import torch

import _rrdb_ref as RR
import _srmut as M
import _srvgg_ref as SR
from _convref import rne16

SR_TY, SR_TX, SR_KC = M.SR_TY, M.SR_TX, M.SR_KC
SOURCES = ("rrdb.hip", "srvgg.hip")
EDGE_SIZES = ((1, 65), (33, 1), (3, 15), (10, 16), (11, 17), (5, 47), (8, 48), (16, 49))
SEAM_FREE_SIZES = ((7, 31), (8, 32))          # one ragged and one exact tile: w % 32 in 31, 0 (what the seam mutants cannot move)
EXACT_SIZES = ((11, 17), (16, 49))
CINS = (32, 64, 96, 128, 160, 192)
RES = ("", "1", "2", "12")
GUARD = 64                                    # elements of each guard region around an output
F16_MAX, F16_OVER = 65504.0, 65520.0          # the largest finite f16, and the least magnitude that rounds to inf

# op -> the kernel of the library it launches, and what elvis_last_launch reports after it
KERNEL = {"rrdb": "rrdb_conv3x3_kernel<{cout}>", "rrdb_u8": "rrdb_conv3x3_kernel<32>", "layer": "srvgg_conv3x3_kernel<64,false>",
          "tail": "srvgg_conv3x3_kernel<48,true>", "tail_u8": "srvgg_conv3x3_kernel<48,true>", "input": "rrdb_input_u8_kernel"}
NOTED = {"rrdb": "rrdb_conv3x3_kernel<{cout}>", "rrdb_u8": "rrdb_conv3x3_kernel<32>", "layer": "srvgg_conv3x3_kernel<64,prelu>",
         "tail": "srvgg_conv3x3_kernel<48,shuffle_f16>", "tail_u8": "srvgg_conv3x3_kernel<48,shuffle_u8>",
         "input": "rrdb_input_u8_kernel<{s}>"}


# ============================================================================================ cases
@dataclass(frozen=True)
class Case:
    id: str
    group: str                                # shapes | exact | values | ties | input
    op: str                                   # rrdb | rrdb_u8 | layer | tail | tail_u8 | input
    h: int
    w: int
    n: int = 1
    cin: int = 64
    cout: int = 64
    cin_real: int = 0                         # layer: the real input channels packed into cin (0: all)
    ups: int = 0
    lrelu: int = 0
    res: str = ""                             # "", "1", "2", "12": the residuals given
    alias: bool = False                       # rrdb: the in-place form, out is x and out_coff = cin
    swap: int = 0
    base_pitch: int = 3
    kind: str = "randn"                       # values: sub_x | sub_w | sat | zeros; ties: bias | r2; input: the s of the call
    k: int = 0                                # ties: the launch number; u8 shapes: the seed of the recipe

    @property
    def kernel(self):
        return KERNEL[self.op].format(cout=self.cout)

    @property
    def noted(self):
        return NOTED[self.op].format(cout=self.cout, s="unshuffle2" if self.kind == "2" else "1")

    @property
    def seed(self):
        return zlib.crc32(self.id.encode())

    @property
    def out_hw(self):
        if self.op in ("tail", "tail_u8"):
            return 4 * self.h, 4 * self.w
        if self.op == "input":
            s = int(self.kind)
            return -(-self.h // s), -(-self.w // s)
        return (self.h << self.ups, self.w << self.ups)

    @property
    def nkc(self):
        return self.cin // SR_KC

    @property
    def tiles(self):
        ho, wo = (self.h << self.ups, self.w << self.ups)
        return -(-ho // SR_TY), -(-wo // SR_TX)


def _build():
    cases = []
    add = lambda *a, **kw: cases.append(Case(*a, **kw))
    k = 0
    for i, (h, w) in enumerate(EDGE_SIZES):
        small = h * w <= 400
        for cout, ups in ((32, 0), (64, 0), ((32, 64)[i % 2], 1)):
            cin = CINS[(k + i) % 6] if not ups or small else CINS[k % 3]
            n = 1 + (k + i) % 2 if not ups or small else 1
            add(f"shape_rrdb_{h}x{w}_cin{cin}_cout{cout}_u{ups}", "shapes", "rrdb", h, w, n, cin, cout, ups=ups, lrelu=k % 2,
                res=RES[(k // 2) % 4], alias=not ups and k % 3 == 0)
            k += 1
        add(f"shape_rrdb_u8_{h}x{w}", "shapes", "rrdb_u8", h, w, 1 + i % 2, (32, 64)[(i // 2) % 2], 32, res=RES[(i + 1) % 4], swap=(i // 2) % 2,
            k=U8_SEEDS.get((h, w), 0))
        add(f"shape_layer_{h}x{w}_cin32", "shapes", "layer", h, w, 1 + i % 2, 32, 64, cin_real=3)
        add(f"shape_layer_{h}x{w}_cin64", "shapes", "layer", h, w, 2 - i % 2, 64, 64)
        add(f"shape_tail_{h}x{w}", "shapes", "tail", h, w, 1 + i % 2, 64, 48, swap=(i // 2) % 2, base_pitch=(3, 5, 32)[i % 3])
        add(f"shape_tail_u8_{h}x{w}", "shapes", "tail_u8", h, w, 2 - i % 2, 64, 48, swap=(i + 1) % 2, base_pitch=(5, 3, 8)[i % 3])
    for i, (h, w) in enumerate(SEAM_FREE_SIZES):
        add(f"shape_rrdb_{h}x{w}_cin{CINS[3 * i]}_cout{(64, 32)[i]}_u0", "shapes", "rrdb", h, w, 2 - i, CINS[3 * i], (64, 32)[i], lrelu=i, res=RES[1 + i])
        add(f"shape_layer_{h}x{w}_cin64", "shapes", "layer", h, w, 1 + i, 64, 64)
        add(f"shape_tail_{h}x{w}", "shapes", "tail", h, w, 2 - i, 64, 48, swap=i, base_pitch=(5, 3)[i])
    j = 0
    for cin in CINS:
        for cout in (32, 64):
            h, w = EXACT_SIZES[j % 2 if cin + cout + 8 <= 200 else 0]          # no tensor above 2 x 16 x 49 x 200
            add(f"exact_rrdb_cin{cin}_cout{cout}", "exact", "rrdb", h, w, 2, cin, cout, res="12", alias=True)
            if cin <= 96:
                add(f"exact_rrdb_cin{cin}_cout{cout}_ups", "exact", "rrdb", 11, 17, 2, cin, cout, ups=1, res="12")
            j += 1
    for j, cin in enumerate((32, 64)):
        for h, w in EXACT_SIZES:
            add(f"exact_layer_cin{cin}_{h}x{w}", "exact", "layer", h, w, 2, cin, 64)
    for swap in (0, 1):
        for j, (h, w) in enumerate(EXACT_SIZES):
            add(f"exact_tail_s{swap}_{h}x{w}", "exact", "tail", h, w, 2, 64, 48, swap=swap, base_pitch=(3, 5)[(swap + j) % 2])
    for kind in ("sub_x", "sub_w", "sat", "zeros"):
        add(f"value_{kind}_rrdb32", "values", "rrdb", 9, 33, 1, 64, 32, kind=kind)
        add(f"value_{kind}_rrdb64", "values", "rrdb", 9, 33, 2, 96, 64, lrelu=int(kind != "sat"), kind=kind)
        add(f"value_{kind}_layer", "values", "layer", 9, 33, 1, 64, 64, kind=kind)
        add(f"value_{kind}_tail", "values", "tail", 9, 33, 1, 64, 48, swap=int(kind in ("sub_w", "zeros")), base_pitch=4, kind=kind)
    for i in range(TIE_TAIL_LAUNCHES):
        h, w = (1, 1) if i < TIE_TAIL_LAUNCHES // 2 else (9, 33)
        add(f"tie_tail_{i}", "ties", "tail_u8", h, w, 1 + (i // 2) % 2, 64, 48, swap=i % 2, base_pitch=3 + i % 3, kind="bias", k=i)
    for i in range(TIE_RRDB_LAUNCHES):
        add(f"tie_rrdb_{i}", "ties", "rrdb_u8", 1, 1, 1, (32, 64)[i % 2], 32, swap=(i // 2) % 2, kind="bias", k=i)
    add("tie_rrdb_r2", "ties", "rrdb_u8", 9, 33, 1, 32, 32, res="2", kind="r2")
    for i, (h, w) in enumerate(EDGE_SIZES):
        add(f"input_{h}x{w}_s1", "input", "input", h, w, 2, swap=i % 2, kind="1")
        if (h % 2 == 0 or h >= 3) and (w % 2 == 0 or w >= 3):
            add(f"input_{h}x{w}_s2", "input", "input", h, w, 2, swap=(i + 1) % 2, kind="2")
    assert len({c.id for c in cases}) == len(cases)
    return tuple(cases)


TIE_TAIL_LAUNCHES, TIE_RRDB_LAUNCHES = 8, 16
# RRDB u8 shape cases whose recipe, on its own seed, puts 2 % or more of the bytes within 255 e of a half-integer: another seed
U8_SEEDS = {(10, 16): 2}
CASES = _build()
BY_ID = {c.id: c for c in CASES}


def of(group, op=None):
    return [c for c in CASES if c.group == group and (op is None or c.op == op)]


def group_kernels():
    """group -> the kernels of the library its cases launch."""
    return {g: tuple(sorted({c.kernel for c in of(g)})) for g in ("shapes", "exact", "values", "ties", "input")}


def _gen(c: Case):
    return torch.Generator().manual_seed(c.seed)


def nchw(t):
    return t.permute(0, 3, 1, 2).double()


# ============================================================================================ ties
def tie_y(m):
    """float32((m + 0.5) / 255) for m an array of integers in 0..254."""
    return ((np.asarray(m, np.float64) + 0.5) / 255.0).astype(np.float32)


_M = np.arange(255)
TIES_EXACT = int((tie_y(_M) * np.float32(255) == (_M + 0.5).astype(np.float32)).sum())
assert TIES_EXACT == 255 and (tie_y(_M) * np.float32(255)).dtype == np.float32, "float32(y * 255) is m + 0.5 exactly, for every m"


def tie_byte(y32, mutant=None):
    """The byte of the fp32 value y: np.rint(float32(y) * float32(255)), or the rule of a u8 mutant on the same product."""
    q = np.asarray(y32, np.float32) * np.float32(255)
    if mutant is None:
        return np.rint(q).astype(np.int64)
    return M.round_u8(torch.from_numpy(q.astype(np.float64)), mutant).numpy()


def tie_m(c: Case):
    """The m of every bias channel of a `bias` tie case: [48] for the tail, [3] for RRDB."""
    if c.op == "tail_u8":
        return (48 * c.k + np.arange(48)) % 255
    return ((3 * c.k + np.arange(3)) * 37) % 255


def _tie_r2_plan():
    """tie_rrdb_r2: pixel p, channel c aims at m = (p + 85 c) % 255 with r2 = f16(y_m) and bias[c] the remainder y_m - f16(y_m)
    that most m share on that channel; `valid` where float32(bias[c] + r2) == y_m, the others are left out."""
    c = BY_ID["tie_rrdb_r2"]
    p = np.arange(c.h * c.w)
    m = (p[:, None] + 85 * np.arange(3)[None, :]) % 255                       # [pixels, 3]
    y = tie_y(m)
    r2 = y.astype(np.float16)
    d = (y.astype(np.float64) - r2.astype(np.float64)).astype(np.float32)
    bias = np.zeros(3, np.float32)
    taken = set()
    for ch in range(3):
        vals, counts = np.unique(d[:, ch], return_counts=True)
        order = [v for v in vals[np.argsort(-counts, kind="stable")] if float(v) not in taken and v != 0]
        bias[ch] = order[0]
        taken.add(float(order[0]))
    valid = (bias[None, :] + r2.astype(np.float32)) == y
    return m, y, r2, bias, valid


# ============================================================================================ inputs
def _int_weights(cout, cin):
    co, ci, ky, kx = torch.meshgrid(torch.arange(cout), torch.arange(cin), torch.arange(3), torch.arange(3), indexing="ij")
    wt = ((co * 7 + ci * 3 + ky * 5 + kx * 7 + (co * ci) % 4) % 3 - 1).float()
    assert not torch.equal(wt, wt.flip(2)) and not torch.equal(wt, wt.flip(3)) and not torch.equal(wt, wt.transpose(2, 3))
    assert not torch.equal(wt[:32, :32], wt[:32, :32].transpose(0, 1))
    return wt


def _int_grid(n, h, w, c, fn):
    yy, xx, cc = torch.meshgrid(torch.arange(h), torch.arange(w), torch.arange(c), indexing="ij")
    return torch.stack([fn(yy, xx, cc, i) for i in range(n)]).half()


def exact_slopes():
    """64 signed powers of two with no period below 64."""
    g = torch.Generator().manual_seed(64)
    a = torch.tensor([0.125, 0.25, 0.5, 1.0, 2.0])[torch.randint(0, 5, (64,), generator=g)] * (1 - 2 * torch.randint(0, 2, (64,), generator=g))
    assert all(not torch.equal(a.roll(r), a) for r in range(1, 64)), "no roll by 1..63 leaves the slopes equal"
    assert bool((a < 0).any()) and bool((a > 0).any()) and bool(((a.abs().log2() % 1) == 0).all())
    return a.float()


def layer_slopes(g):
    """Per-channel slopes with negative ones, zeros and ones above 1 among them (tests/test_gpu_srvgg.py's)."""
    a = 0.2 + 0.3 * torch.randn(64, generator=g)
    a[3::16], a[5::16], a[9::16], a[12::16] = -0.5, 0.0, 1.75, -1.5
    return a


def _sub(shape, g, lo=-24.0, hi=-15.0):
    """Signed magnitudes 2^u, u uniform in [lo, hi], as f16: all non-zero f16 subnormals (or 2^-14 times a bit less)."""
    u = lo + (hi - lo) * torch.rand(shape, generator=g)
    v = (torch.exp2(u.double()) * (1 - 2 * torch.randint(0, 2, shape, generator=g))).half()
    assert bool((v != 0).all()) and float(v.abs().max()) <= 2.0 ** hi and float(v.abs().min()) >= 2.0 ** -24
    return v


def _pad_nan(t, pitch):
    """[..., c] f16 -> [..., pitch] with NaN in the channels the kernel must not read."""
    out = torch.full(t.shape[:-1] + (pitch,), float("nan"), dtype=torch.float16)
    out[..., :t.shape[-1]] = t
    return out


def _value_operands(c: Case, g, cout):
    """(wt, b, x [n,h,w,cin] f16) of a value-edge case."""
    n, h, w, cin = c.n, c.h, c.w, c.cin
    if c.kind == "sub_x":
        wt = torch.randn((cout, cin, 3, 3), generator=g) * 0.5
        b = torch.randn(cout, generator=g) * 2.0 ** -16
        x = _sub((n, h, w, cin), g)
    elif c.kind == "sub_w":
        wt = _sub((cout, cin, 3, 3), g).float()
        b = torch.randn(cout, generator=g) * 2.0 ** -6
        x = (torch.randn((n, h, w, cin), generator=g) * 1024.0).half()
    elif c.kind == "sat":
        wt = torch.randn((cout, cin, 3, 3), generator=g) / math.sqrt(9 * cin)
        wt[[3, 9, 28]] *= 40.0                                               # the few channels whose sums pass 65504
        b = torch.randn(cout, generator=g) * 0.5
        x = (torch.randn((n, h, w, cin), generator=g) * 64.0).half()
        hit = torch.rand((n, h, w, cin), generator=g) < 0.02
        x[hit] = (F16_MAX * (1 - 2 * torch.randint(0, 2, (int(hit.sum()),), generator=g))).half()
    else:                                                                    # zeros: -0.0 left of column 20, values right of it
        wt = torch.randn((cout, cin, 3, 3), generator=g) / math.sqrt(9 * cin)
        b = torch.zeros(cout)
        x = torch.randn((n, h, w, cin), generator=g).half()
        x[:, :, :20] = -0.0
    return wt, b, x


@lru_cache(maxsize=None)
def inputs(cid: str):
    """The host-side operands of a case, the same objects for every caller: dict of wt / b (fp32, unpacked), x (f16
    [n,h,w,pitch], NaN in the channels past cin unless `alias`), and per op r1 / r2 / r1_is_x / s0 / s1 / out_coff /
    out_pitch, slope, base, frames."""
    c = BY_ID[cid]
    g = _gen(c)
    n, h, w, cin, cout = c.n, c.h, c.w, c.cin, c.cout
    ho, wo = c.out_hw
    d = {}
    if c.op == "input":
        frames = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
        frames[0, 0, 0] = torch.tensor([0, 255, 128], dtype=torch.uint8)
        return dict(frames=frames)
    if c.group == "ties":
        d["wt"] = torch.randn((3 if c.op == "rrdb_u8" else 48, cin, 3, 3), generator=g) / math.sqrt(9 * cin)
        d["x"] = torch.zeros((n, h, w, cin), dtype=torch.float16)
        if c.op == "tail_u8":
            d["b"] = torch.from_numpy(tie_y(tie_m(c)))
            d["base"] = torch.zeros((n, h, w, c.base_pitch), dtype=torch.float16)
            if c.base_pitch > 3:
                d["base"][..., 3:] = float("nan")
        elif c.kind == "bias":
            d["b"] = torch.from_numpy(tie_y(tie_m(c)))
            d.update(r1=None, r2=None, s0=1.0, s1=0.0)
        else:
            m, y, r2, bias, valid = _tie_r2_plan()
            d["b"] = torch.from_numpy(bias)
            wide = torch.zeros((1, h, w, 32), dtype=torch.float16)                # r2's pitch is at least cout
            wide[..., :3] = torch.from_numpy(r2).reshape(1, h, w, 3)
            d.update(r1=None, r2=wide, s0=1.0, s1=0.0)
        return d
    if c.op == "rrdb_u8":
        wt, b, x, r1, r2 = RR.u8_inputs(cin, h, w, n, c.swap, c.res, seed=c.k or None)
        return dict(wt=wt, b=b, x=x, r1=r1, r2=r2, s0=1.0, s1=0.5)
    if c.op == "tail_u8":
        wt, b, x, base = SR.u8_inputs(h, w, n, c.swap, c.base_pitch, seed=c.k or None)
        return dict(wt=wt, b=b, x=x, base=base)
    if c.group == "exact":
        d["wt"] = _int_weights(cout, cin)
        x = _int_grid(n, h, w, cin, lambda yy, xx, cc, i: (yy * 3 + xx * 5 + cc * 7 + i) % 3)
        if c.op == "rrdb":
            d["b"] = (torch.arange(cout) % 5 - 2).float()
            d["r1"] = _int_grid(n, ho, wo, cout + 4, lambda yy, xx, cc, i: 4 * ((yy * 5 + xx * 3 + cc + i) % 5 - 2))
            d["r2"] = _int_grid(n, ho, wo, cout + 12, lambda yy, xx, cc, i: (yy + xx * 7 + cc * 3 + 2 * i) % 9 - 4)
            d.update(s0=0.5, s1=0.25, r1_is_x=False)
            if c.alias:
                d["x"] = torch.cat((x, torch.full((n, h, w, cout + 8), 7.0, dtype=torch.float16)), -1)
                d.update(out_coff=cin, out_pitch=cin + cout + 8)
            else:
                d["x"] = _pad_nan(x, cin + 8)
                d.update(out_coff=0, out_pitch=cout)
        elif c.op == "layer":
            d["b"] = (torch.arange(64) % 5 - 2).float()
            d["slope"] = exact_slopes()
            d["x"] = _pad_nan(x, cin + 8)
        else:
            d["b"] = (torch.arange(48) % 7 - 3).float()
            d["x"] = _pad_nan(x, 72)
            d["base"] = _int_grid(n, h, w, c.base_pitch, lambda yy, xx, cc, i: (yy * 5 + xx * 3 + cc * 11 + 2 * i) % 13 - 6)
            if c.base_pitch > 3:
                d["base"][..., 3:] = float("nan")
        return d
    if c.group == "values":
        wt, b, x = _value_operands(c, g, cout)
        d.update(wt=wt, b=b)
        if c.op == "rrdb":
            d["x"] = _pad_nan(x, cin + 8)
            d.update(r1=None, r2=None, r1_is_x=False, s0=1.0, s1=0.0, out_coff=0, out_pitch=cout + 8)
        elif c.op == "layer":
            d["x"] = _pad_nan(x, cin + 8)
            d["slope"] = layer_slopes(g)
        else:
            d["x"] = _pad_nan(x, 72)
            base = {"sub_x": lambda: _sub((n, h, w, 3), g), "sub_w": lambda: torch.randn((n, h, w, 3), generator=g).half(),
                    "sat": lambda: (torch.randn((n, h, w, 3), generator=g) * 64.0).half(),
                    "zeros": lambda: torch.where(torch.rand((n, h, w, 3), generator=g) < 0.5, torch.tensor(-0.0), torch.tensor(0.0)).half()}[c.kind]()
            d["base"] = _pad_nan(base, c.base_pitch)
        return d
    # shapes
    if c.op == "rrdb":
        d["wt"] = torch.randn((cout, cin, 3, 3), generator=g) / math.sqrt(9 * cin)
        d["b"] = torch.randn(cout, generator=g) * 0.5
        if c.alias:                                   # the in-place concat: channels [0, cin) read, [cin, cin + cout) written
            d["x"] = torch.randn((n, h, w, cin + cout + 8), generator=g).half()
            d.update(out_coff=cin, out_pitch=cin + cout + 8)
        else:
            d["x"] = _pad_nan(torch.randn((n, h, w, cin), generator=g).half(), cin + 8)
            d.update(out_coff=0, out_pitch=cout + 8)
        d["r1_is_x"] = "1" in c.res and not c.ups and cin >= cout          # r1 may be x itself
        d["r1"] = _pad_nan(torch.randn((n, ho, wo, cout), generator=g).half(), cout + 4) if "1" in c.res and not d["r1_is_x"] else None
        d["r2"] = _pad_nan(torch.randn((n, ho, wo, cout), generator=g).half(), cout + 12) if "2" in c.res else None
        d["s0"], d["s1"] = (0.2, 0.5) if c.res else (1.0, 0.0)
    elif c.op == "layer":
        real = c.cin_real or cin
        d["wt"] = torch.randn((64, real, 3, 3), generator=g) / math.sqrt(9 * real)
        d["b"] = torch.randn(64, generator=g) * 0.5
        d["slope"] = layer_slopes(g)
        d["x"] = _pad_nan(torch.randn((n, h, w, cin), generator=g).half(), cin + 8)
    else:
        d["wt"] = torch.randn((48, 64, 3, 3), generator=g) / math.sqrt(9 * 64)
        d["b"] = torch.randn(48, generator=g) * 0.5
        d["x"] = _pad_nan(torch.randn((n, h, w, 64), generator=g).half(), 72)
        d["base"] = _pad_nan(torch.randn((n, h, w, 3), generator=g).half(), c.base_pitch)
    return d


# ============================================================================================ expected
@lru_cache(maxsize=None)
def expected(cid: str, mutant: Optional[str] = None):
    """The statement of a case (its mutant): a ConvRef over the written channels in NCHW (RGB order for the tail, whatever
    `swap`), for the u8 shape cases (ConvRef, byte, near), for the ties (byte [n,3,ho,wo] in RGB order, valid mask), for
    the input stage the f16 tensor."""
    c = BY_ID[cid]
    d = inputs(cid)
    if c.op == "input":
        return RR.input_ref(d["frames"], int(c.kind), bool(c.swap))
    if c.group == "ties":
        ho, wo = c.out_hw
        if c.op == "tail_u8":
            per = torch.from_numpy(tie_byte(d["b"].numpy(), mutant))[None, :, None, None].expand(c.n, 48, c.h, c.w)
            return SR.shuffle4(per.double()).to(torch.int64), torch.ones((c.n, 3, ho, wo), dtype=torch.bool)
        if c.kind == "bias":
            per = torch.from_numpy(tie_byte(d["b"].numpy(), mutant))[None, :, None, None].expand(c.n, 3, c.h, c.w)
            return per.contiguous(), torch.ones((c.n, 3, ho, wo), dtype=torch.bool)
        m, y, r2, bias, valid = _tie_r2_plan()
        byte = torch.from_numpy(tie_byte(y, mutant)).reshape(1, c.h, c.w, 3).permute(0, 3, 1, 2).contiguous()
        return byte, torch.from_numpy(valid).reshape(1, c.h, c.w, 3).permute(0, 3, 1, 2).contiguous()
    x = nchw(d["x"])
    u8 = mutant if mutant in RR.U8_MUTANTS else None
    cm = None if u8 else mutant
    if c.op in ("rrdb", "rrdb_u8"):
        cout = 3 if c.op == "rrdb_u8" else c.cout
        r1 = x if d.get("r1_is_x") else (None if d["r1"] is None else nchw(d["r1"]))
        r2 = None if d["r2"] is None else nchw(d["r2"])
        r = RR.conv_ref(x[:, :c.cin], d["wt"], d["b"], upsample=bool(c.ups), lrelu=bool(c.lrelu), s0=d["s0"], s1=d["s1"],
                        r1=None if r1 is None else r1[:, :cout], r2=None if r2 is None else r2[:, :cout], mutant=cm)
        return (r,) + tuple(RR.u8_ref(r, u8)) if c.op == "rrdb_u8" else r
    if c.op == "layer":
        return SR.conv_ref(x[:, :c.cin_real or c.cin], d["wt"], d["b"], d["slope"], mutant=cm)
    r = SR.tail_ref(x[:, :64], d["wt"], d["b"], nchw(d["base"])[:, :3], mutant=cm)
    return (r,) + tuple(SR.u8_ref(r, u8)) if c.op == "tail_u8" else r


def near_share(cid):
    """Share of the bytes of a u8 shape case that may differ by one: from the statement alone."""
    return float(expected(cid)[2].double().mean())


def must_be_inf(r):
    """Where the stored f16 must be +-inf (|ref| passes 65520 by more than the bound), and where it must be finite."""
    b = r.bound()
    return r.ref.abs() - b >= F16_OVER, r.ref.abs() + b < F16_OVER


def value_facts(cid):
    """What a value-edge case reaches, from the statement and the inputs alone."""
    c, d, r = BY_ID[cid], inputs(cid), expected(cid)
    q = rne16(r.ref.clamp(-F16_MAX, F16_MAX))
    x = d["x"][..., :c.cin]
    w16 = d["wt"].half()
    inf, fin = must_be_inf(r)
    return dict(sub_out=float(((q != 0) & (q.abs() < 2.0 ** -14)).double().mean()), normal_out=float((q.abs() >= 2.0 ** -14).double().mean()),
                zero_out=float((q == 0).double().mean()),
                sub_x=float(((x != 0) & (x.abs() < 2.0 ** -14)).double().mean()), sub_w=float(((w16 != 0) & (w16.abs() < 2.0 ** -14)).double().mean()),
                x_max=float(x.abs().max()), x_at_max=int((x.abs() == F16_MAX).sum()), neg_zero_x=int(((x == 0) & torch.signbit(x)).sum()),
                pos_inf=int((inf & (r.ref > 0)).sum()), neg_inf=int((inf & (r.ref < 0)).sum()), undecided=int((~inf & ~fin).sum()),
                inf_channels=sorted(set(torch.nonzero(inf)[:, 1].tolist())), finite=int(fin.sum()))


# ============================================================================================ mutants
def _first(op, **kw):
    for c in of("shapes", op):
        if all((v(getattr(c, k)) if callable(v) else getattr(c, k) == v) for k, v in kw.items()):
            return c.id
    raise LookupError((op, kw))


# label -> (mutant of the statement, the case it must move, structural: at least 10 bounds)
MUTANTS = {
    "tap_corner_00": ("tap_corner_00", _first("rrdb", h=11, w=17, ups=0), True),
    "halo_col_32": ("halo_col_32", _first("layer", h=5, w=47, cin_real=0), True),
    "halo_row_8": ("halo_row_8", _first("tail", h=11, w=17), True),
    "frag_col_16": ("frag_col_16", _first("rrdb", h=10, w=16, ups=0), True),
    "kchunk_last_nkc2": ("kchunk_last", _first("rrdb", cin=64, ups=0), True),
    "kchunk_last_nkc6": ("kchunk_last", _first("rrdb", cin=192, ups=0), True),
    "taps_transposed": ("taps_transposed", _first("tail", h=3, w=15), True),
    "bias_roll_1": ("bias_roll_1", _first("rrdb", h=3, w=15, ups=0), True),
    "bias_roll_4": ("bias_roll_4", _first("layer", h=10, w=16, cin_real=3), True),
    "bias_roll_16": ("bias_roll_16", _first("tail", h=8, w=48), True),
    "slope_roll_1": ("slope_roll_1", _first("layer", h=33, w=1, cin_real=0), True),
    "slope_roll_4": ("slope_roll_4", _first("layer", h=1, w=65, cin_real=3), True),
    "slope_roll_16": ("slope_roll_16", _first("layer", h=16, w=49, cin_real=0), True),
    "s0_s1_swapped": ("s0_s1_swapped", _first("rrdb", res=lambda r: "1" in r), True),
    "r1_r2_swapped": ("r1_r2_swapped", _first("rrdb", res="12"), True),
    "ups_source_round_up": ("ups_source_round_up", _first("rrdb", ups=1, h=lambda h: h > 1), True),
    "shuffle_dy_dx": ("shuffle_dy_dx", _first("tail", h=5, w=47), True),
    "base_left": ("base_left", _first("tail", h=16, w=49), True),
    "base_not_swapped": ("base_not_swapped", _first("tail", swap=1), True),
    "store_f16_trunc": ("store_f16_trunc", _first("tail", h=10, w=16), False),
    "weights_trunc": ("weights_trunc", _first("layer", h=11, w=17, cin_real=0), False),
}
U8_MUTANTS = ("u8_half_up", "u8_truncate")         # on every case of the `ties` group


def mutant_ratio(label):
    """Worst |mutant - statement| / bound over the elements of the mutant's case."""
    name, cid, _ = MUTANTS[label]
    r, m = expected(cid), expected(cid, name)
    return float(((m.ref - r.ref).abs() / r.bound()).max())


def tie_bytes_changed(mutant):
    """Bytes of the tie cases (valid ones) that a u8 rounding mutant changes."""
    return sum(int(((expected(c.id, mutant)[0] != expected(c.id)[0]) & expected(c.id)[1]).sum()) for c in of("ties"))
