"""The edge matrix of csrc/rrdb.hip and csrc/srvgg.hip on the device: every case of tests/_srcases.py through the C ABI.

Every output lies between two guard regions of 64 elements that must come back untouched; the unwritten channels of a
wide output and the inputs are compared with what they held; `elvis_last_launch` is asserted after every call.  Shape and
value cases hold |y - ref| / bound <= 1 with the statements' own bounds (tests/_rrdb_ref.py, tests/_srvgg_ref.py); the
integer, tie and input-stage cases are compared for equality.  A shape case is launched twice into fresh buffers and the
two results must be the same bytes.

Measured on an MI355X, worst |device - statement| / bound: shapes rrdb<32> 0.973, rrdb<64> 0.976, layer 0.995 (K = 27: the
bound is all but the half ulp of the store), tail 0.870; value edges 0.797 (subnormal activations), 0.964 (subnormal
weights), 0.923 (saturation), 0.784 (zeros); no u8 shape byte off; 85 878 tie bytes equal (the tests section)."""
import numpy as np
import pytest
import torch

import _srcases as S
from elvis_amd import _lib, realesrgan, srvgg

pytestmark = pytest.mark.gpu

F16_GUARD, F16_FILL, U8_GUARD, U8_FILL = -1234.0, 7.0, 0xA5, 99


def _ids(cases):
    return [c.id for c in cases]


class Guarded:
    """A tensor of `shape` between two guard regions of S.GUARD elements, in one allocation."""

    def __init__(self, shape, dtype, dev, fill=None, content=None):
        self.numel = int(np.prod(shape))
        self.guard = U8_GUARD if dtype == torch.uint8 else F16_GUARD
        self.flat = torch.full((self.numel + 2 * S.GUARD,), self.guard, dtype=dtype, device=dev)
        self.t = self.flat[S.GUARD:S.GUARD + self.numel].view(shape)
        if content is not None:
            self.t.copy_(content)
        else:
            self.t.fill_(fill)

    def guards_untouched(self):
        flat = self.flat.cpu()
        return bool((flat[:S.GUARD] == self.guard).all()) and bool((flat[S.GUARD + self.numel:] == self.guard).all())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.uint8)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _packed(c, d, dev):
    packed, bias, cin, cout = (realesrgan if c.op in ("rrdb", "rrdb_u8") else srvgg).pack_conv(d["wt"], d["b"])
    assert (cin, cout) == (c.cin, c.cout)
    return torch.from_numpy(packed.view(np.int16)).to(dev), torch.from_numpy(bias).to(dev)


def launch(c, dev):
    """One call of the case into fresh buffers: (the Guarded output, the values written as NCHW float64 or int64 in the
    statement's channel order).  Asserts the launch note, the guards, the unwritten channels and the inputs."""
    d = S.inputs(c.id)
    L = _lib.lib()
    stream = _lib.stream_handle(dev)
    n, h, w = c.n, c.h, c.w
    ho, wo = c.out_hw
    if c.op == "input":
        src = d["frames"].to(dev)
        out = Guarded((n, ho, wo, 32), torch.float16, dev, fill=F16_FILL)
        _lib.check(L.elvis_rrdb_input_u8(src.data_ptr(), out.t.data_ptr(), n, h, w, int(c.kind), c.swap, stream), dev)
        torch.cuda.synchronize()
        assert L.elvis_last_launch() == c.noted.encode()
        assert out.guards_untouched() and torch.equal(src.cpu(), d["frames"])
        return out, out.t.cpu()
    wp, bias = _packed(c, d, dev)
    u8 = c.op in ("rrdb_u8", "tail_u8")
    if c.op in ("rrdb", "rrdb_u8"):
        alias = c.alias
        if alias:                                     # x is the output buffer: guarded, and its other channels must stay
            out = Guarded(tuple(d["x"].shape), torch.float16, dev, content=d["x"])
            x_d, out_coff = out.t, d["out_coff"]
        elif u8:
            out = Guarded((n, ho, wo, 3), torch.uint8, dev, fill=U8_FILL)
            x_d, out_coff = d["x"].to(dev), 0
        else:
            out = Guarded((n, ho, wo, d["out_pitch"]), torch.float16, dev, fill=F16_FILL)
            x_d, out_coff = d["x"].to(dev), 0
        r1_d = x_d if d.get("r1_is_x") else (None if d["r1"] is None else d["r1"].to(dev))
        r2_d = None if d["r2"] is None else d["r2"].to(dev)
        before = out.t.clone()
        rc = L.elvis_rrdb_conv3x3(x_d.data_ptr(), x_d.shape[-1], wp.data_ptr(), bias.data_ptr(), out.t.data_ptr(), out.t.shape[-1], out_coff,
                                  _lib.ptr(r1_d), 0 if r1_d is None else r1_d.shape[-1], _lib.ptr(r2_d), 0 if r2_d is None else r2_d.shape[-1],
                                  n, h, w, c.cin, c.cout, c.ups, c.lrelu, d["s0"], d["s1"], int(u8), c.swap, stream)
        _lib.check(rc, dev)
        torch.cuda.synchronize()
        assert L.elvis_last_launch() == c.noted.encode()
        assert out.guards_untouched(), "a store outside the output"
        for t, host in ((r1_d, d["r1"]), (r2_d, d["r2"])) + (() if alias else ((x_d, d["x"]),)):
            assert t is None or host is None or _same(t, host), "an input was written"
        if u8:
            got = out.t.cpu().to(torch.int64).permute(0, 3, 1, 2)
            return out, (got.flip(1) if c.swap else got)
        assert _same(out.t[..., :out_coff], before[..., :out_coff]) and _same(out.t[..., out_coff + c.cout:], before[..., out_coff + c.cout:]), \
            "channels outside [out_coff, out_coff + cout) were written"
        return out, S.nchw(out.t.cpu())[:, out_coff:out_coff + c.cout]
    x_d = d["x"].to(dev)
    if c.op == "layer":
        slope = d["slope"].to(dev)
        out = Guarded((n, h, w, 72), torch.float16, dev, fill=F16_FILL)
        _lib.check(L.elvis_srvgg_conv3x3(x_d.data_ptr(), x_d.shape[-1], wp.data_ptr(), bias.data_ptr(), slope.data_ptr(), out.t.data_ptr(),
                                         72, n, h, w, c.cin, stream), dev)
        torch.cuda.synchronize()
        assert L.elvis_last_launch() == c.noted.encode()
        assert out.guards_untouched(), "a store outside the output"
        assert bool((out.t[..., 64:] == F16_FILL).all()), "channels past 64 were written"
        assert _same(x_d, d["x"]) and torch.equal(slope.cpu(), d["slope"])
        return out, S.nchw(out.t.cpu())[:, :64]
    base_d = d["base"].to(dev)
    out = Guarded((n, ho, wo, 3), torch.uint8 if u8 else torch.float16, dev, fill=U8_FILL if u8 else F16_FILL)
    _lib.check(L.elvis_srvgg_tail(x_d.data_ptr(), x_d.shape[-1], wp.data_ptr(), bias.data_ptr(), base_d.data_ptr(), base_d.shape[-1],
                                  out.t.data_ptr(), n, h, w, int(u8), c.swap, stream), dev)
    torch.cuda.synchronize()
    assert L.elvis_last_launch() == c.noted.encode()
    assert out.guards_untouched(), "a store outside the output"
    assert _same(x_d, d["x"]) and _same(base_d, d["base"])
    got = out.t.cpu().to(torch.int64).permute(0, 3, 1, 2) if u8 else S.nchw(out.t.cpu())
    return out, (got.flip(1) if c.swap else got)


def _ratio(y, r):
    """Worst |y - ref| / bound; a NaN or an infinity of the device counts as infinite."""
    ratio = (y - r.ref).abs() / r.bound()
    return float(torch.where(torch.isfinite(y), ratio, torch.full_like(ratio, float("inf"))).max())


# ------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("cid", _ids([c for c in S.of("shapes") if c.op in ("rrdb", "layer", "tail")]))
def test_shapes_within_the_statements_bound(gpu_device, cid):
    c = S.BY_ID[cid]
    r = S.expected(cid)
    out1, y = launch(c, gpu_device)
    worst = _ratio(y, r)
    print(f"{cid}: worst |y - ref| / bound = {worst:.3f}")
    assert worst <= 1.0
    out2, _ = launch(c, gpu_device)
    assert _same(out1.t, out2.t), "the same call into a fresh buffer gave other bytes"


@pytest.mark.parametrize("cid", _ids([c for c in S.of("shapes") if c.op in ("rrdb_u8", "tail_u8")]))
def test_shapes_u8(gpu_device, cid):
    c = S.BY_ID[cid]
    r, byte, near = S.expected(cid)
    share = S.near_share(cid)
    assert share < 0.02, f"{share:.4f} of the elements lie within 255 e of a half-integer"       # from the reference alone
    assert bool((r.ref < 0).any()) and bool((r.ref > 1).any())                                    # both clamps are reached
    out1, got = launch(c, gpu_device)
    diff = (got - byte).abs()
    print(f"{cid}: near-half share {share:.4f}, bytes off by one {int((diff == 1).sum())}")
    assert int(diff.max()) <= 1 and not (diff[~near] != 0).any()
    out2, _ = launch(c, gpu_device)
    assert _same(out1.t, out2.t), "the same call into a fresh buffer gave other bytes"


# ------------------------------------------------------------------------------------------------------- exact integers
@pytest.mark.parametrize("cid", _ids(S.of("exact")))
def test_exact_integers(gpu_device, cid):
    c = S.BY_ID[cid]
    r = S.expected(cid)
    assert torch.equal(r.ref, r.ref.half().double()) and float(r.ref.abs().max()) < 2048, "the expected values are exact in f16"
    assert float((r.ref < 0).double().mean()) > 0.05
    _, y = launch(c, gpu_device)
    assert torch.equal(y, r.ref), f"{int((y != r.ref).sum())} of {y.numel()} values differ"


# ------------------------------------------------------------------------------------------------------- value edges
@pytest.mark.parametrize("cid", _ids(S.of("values")))
def test_value_edges(gpu_device, cid):
    """Subnormal operands and results, sums past 65504, -0.0 under a zero bias: the statement's own bound (ulp16 is 2^-24
    below 2^-14 there); where |ref| passes 65520 by more than the bound the device holds the infinity of that sign, where
    it stays below by more than the bound a finite value within the bound."""
    c = S.BY_ID[cid]
    r = S.expected(cid)
    _, y = launch(c, gpu_device)
    assert not torch.isnan(y).any()
    inf, fin = S.must_be_inf(r)
    assert bool((y[inf] == torch.sign(r.ref[inf]) * float("inf")).all()), "a sum past 65504 by more than the bound is stored as that infinity"
    assert bool(torch.isfinite(y[fin]).all())
    free = ~inf & ~fin                                # within the bound of 65520: either, with the sign of the statement
    assert bool((torch.isfinite(y[free]) | (y[free] == torch.sign(r.ref[free]) * float("inf"))).all())
    ok = torch.isfinite(y)
    worst = float(((y - r.ref).abs() / r.bound())[ok].max())
    print(f"{cid}: worst |y - ref| / bound = {worst:.3f} over {int(ok.sum())} finite values, {int((~ok).sum())} infinities")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("cid", _ids(S.of("ties")))
def test_ties_round_half_to_even(gpu_device, cid):
    c = S.BY_ID[cid]
    byte, valid = S.expected(cid)
    _, got = launch(c, gpu_device)
    wrong = (got != byte) & valid
    print(f"{cid}: {int(valid.sum())} tie bytes compared")
    assert not wrong.any(), f"{int(wrong.sum())} of {int(valid.sum())} tie bytes differ: got {got[wrong][:8].tolist()}, want {byte[wrong][:8].tolist()}"


# ------------------------------------------------------------------------------------------------------- the input stage
@pytest.mark.parametrize("cid", _ids(S.of("input")))
def test_input_stage(gpu_device, cid):
    c = S.BY_ID[cid]
    _, got = launch(c, gpu_device)
    assert _same(got, S.expected(cid))
