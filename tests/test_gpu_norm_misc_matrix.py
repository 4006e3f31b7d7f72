"""The kernels of csrc/norm.hip and csrc/misc.hip against the references of tests/_normref.py, through the C ABI.

Error-bounded ops (GroupNorm sums, partials -> sums, GroupNorm affine, GroupNorm end to end, affine_act, LayerNorm,
bicubic): tier 1 on every element, and for f16 outputs tier 2 in two forms - the interval form of the earlier matrices
(>= 0.998 everywhere) and the share of outputs that EQUAL the correctly rounded reference, whose floor is computed per
case from the float64 reference alone (_normref.exact_share_floor).  Exact ops (VQ, u8 <-> float, reflect pad, crop,
dtype conversion): bit for bit.  Every output buffer starts NaN on its logical elements and a sentinel on a guard row
and on the pitch padding; what each op does to the padding is part of its contract (include/elvis_amd.h) and asserted:
affine_act and LayerNorm zero [c, pitch_for(c)) and leave the rest, bicubic / crop / VQ / u8_to_float zero [c, pitch),
pad_reflect_axpy writes [coff, coff + c) only."""
import numpy as np
import pytest
import torch

import _normref as R
from test_gpu_model_kernels_matrix import SENTINEL, _last_launch, _out_buffer, _pitched

pytestmark = pytest.mark.gpu


def _dt(dt):
    from elvis_amd._lib import F16, F32
    return (torch.float16, F16) if dt == "f16" else (torch.float32, F32)


def _gen(c):
    return torch.Generator().manual_seed(7000 + c.seed)


def _take(buf, rows, c, zero_to, cid):
    """The logical [rows, c] values (float64, CPU) of a [rows + 1, pitch] buffer; [c, zero_to) must be zero, everything
    else (further padding, the guard row) must still hold the sentinel."""
    b = buf.double().cpu()
    assert bool((b[:rows, c:zero_to] == 0).all()), f"{cid}: pad channels [{c}, {zero_to}) are not zero"
    assert bool((b[:rows, zero_to:] == SENTINEL).all()), f"{cid}: written beyond channel {zero_to} of the pitch"
    assert bool((b[rows] == SENTINEL).all()), f"{cid}: written past the last row"
    return b[:rows, :c]


def _inplace_buffer(x2d, c, pitch, dtype, dev):
    """[rows + 1, pitch] input that is also the output: values, NaN on [c, pitch_for(c)), the sentinel beyond."""
    rows = x2d.shape[0]
    t = torch.full((rows + 1, pitch), SENTINEL, dtype=dtype)
    t[:rows, :R.pitch_for(c)] = float("nan")
    t[:rows, :c] = x2d.to(dtype)
    return t.to(dev)


def _guarded(numel, dtype, dev, fill=float("nan"), guard=8):
    t = torch.full((numel + guard,), SENTINEL, dtype=dtype)
    t[:numel] = fill
    return t.to(dev)


def _guard_ok(t, numel, cid):
    assert bool((t[numel:].cpu() == SENTINEL).all()), f"{cid}: written past the end of a buffer"


# ------------------------------------------------------------------------------------------------------- runners
def _sums_call(x, c, case_dt, pitch_extra, sums, ctot, coff, dev, cid):
    """elvis_groupnorm_sums of x [n, hw, c] into the slice of `sums`; checks the workspace size and its guard."""
    from elvis_amd._lib import lib, check, ptr, stream_handle
    dtype, code = _dt(case_dt)
    n, hw, _ = x.shape
    nws = lib().elvis_groupnorm_workspace_floats(code, n, hw, c)
    assert nws == R.gn_workspace_floats(case_dt == "f16", n, hw, c), f"{cid}: gn_blocks restatement is off"
    ws = _guarded(nws, torch.float32, dev)
    pin = R.pitch_for(c) + pitch_extra
    xd = _pitched(x, pin, dtype, dev)                     # NaN in every pad channel: loaded, must be ignored
    check(lib().elvis_groupnorm_sums(ptr(xd), code, n, hw, c, pin, ptr(sums), ctot, coff, ptr(ws), stream_handle(dev)), dev)
    torch.cuda.synchronize()
    _guard_ok(ws, nws, cid)
    assert not bool(torch.isnan(ws[:nws]).any()), f"{cid}: a partial row was not written"
    return xd


def _run_gn_sums(c, dev):
    dtype, _ = _dt(c.dt)
    x = c.mean + torch.randn(c.n, c.hw, c.c, generator=_gen(c))
    ctot = c.coff + c.c + c.ctot_extra
    sums = torch.full((c.n, ctot, 2), SENTINEL, dtype=torch.float64, device=dev)
    _sums_call(x, c.c, c.dt, c.pitch_extra, sums, ctot, c.coff, dev, c.id)
    name = "gn_channel_sums_kernel<half>" if c.dt == "f16" else "gn_channel_sums_kernel<float>"
    assert _last_launch() == "gn_partials_reduce_kernel" or _last_launch() == name
    s = sums.cpu()
    keep = torch.ones(ctot, dtype=torch.bool)
    keep[c.coff:c.coff + c.c] = False
    assert bool((s[:, keep] == SENTINEL).all()), f"{c.id}: sums outside the channel slice changed"
    return name, s[:, c.coff:c.coff + c.c], R.gn_sums_ref(x.to(dtype).double(), c.dt == "f16")


def _partials(c, dev, misalign):
    p = (torch.randn(c.n, c.tiles, c.c, 2, generator=torch.Generator().manual_seed(7000 + c.seed)) * 50.0 + 20.0).float()
    flat = torch.empty(p.numel() + 4, dtype=torch.float32, device=dev)
    off = 1 if misalign else 0
    assert flat.data_ptr() % 16 == 0
    view = flat[off:off + p.numel()]
    view.copy_(p.reshape(-1).to(dev))
    return p, view


def _partials_call(c, view, dev):
    from elvis_amd._lib import lib, check, ptr, stream_handle
    ctot = c.coff + c.c + c.ctot_extra
    sums = torch.full((c.n, ctot, 2), SENTINEL, dtype=torch.float64, device=dev)
    check(lib().elvis_gn_partials_to_sums(ptr(view), c.tiles, c.n, c.c, ptr(sums), ctot, c.coff, stream_handle(dev)), dev)
    name = _last_launch()
    torch.cuda.synchronize()
    s = sums.cpu()
    keep = torch.ones(ctot, dtype=torch.bool)
    keep[c.coff:c.coff + c.c] = False
    assert bool((s[:, keep] == SENTINEL).all()), f"{c.id}: sums outside the channel slice changed"
    return name, s[:, c.coff:c.coff + c.c]


def _run_partials(c, dev):
    p, view = _partials(c, dev, c.misalign)
    name, y = _partials_call(c, view, dev)
    return name, y, R.partials_ref(p.double())


def affine_inputs(c, g):
    """(sums [n, c, 2] float64, gamma, beta, scale, shift as fp32 tensors or None)."""
    n, C, hw = c.n, c.c, c.hw
    if c.kind == "const":
        v = torch.tensor([0.75, -3.0])[torch.arange(C) % 2].double().expand(n, C) if c.groups == C else torch.full((n, C), 0.75).double()
        sums = torch.stack([v * hw, v * v * hw], -1)
    elif c.kind == "negvar":
        # a constant 1000.0 image whose sum of squares came out 2^-40 low: E[x^2] - mean^2 < 0, clamped to 0
        sums = torch.stack([torch.full((n, C), 1000.0 * hw), torch.full((n, C), 1.0e6 * hw * (1 - 2.0 ** -40))], -1).double()
    else:
        x = (torch.randn(n, 1, C, generator=g) * 2.0 + torch.randn(n, hw, C, generator=g) * (0.2 + torch.rand(1, 1, C, generator=g))).double()
        sums = torch.stack([x.sum(1), (x * x).sum(1)], -1)
    f = lambda on, t: t.float() if on else None
    gam = f(c.affine, torch.rand(C, generator=g) + 0.5)
    bet = f(c.affine, torch.randn(C, generator=g) * 0.3)
    sc = f(c.scale, torch.randn(C, generator=g) * 0.3)
    sh = f(c.shift, torch.randn(C, generator=g) * 0.3)
    return sums.contiguous(), gam, bet, sc, sh


def _affine_call(sums_d, gam, bet, sc, sh, n, hw, C, groups, eps, dev, cid):
    from elvis_amd._lib import lib, check, ptr, stream_handle
    d = lambda t: None if t is None else t.to(dev)
    keep = [d(gam), d(bet), d(sc), d(sh)]
    pa, pb = _guarded(n * C, torch.float32, dev), _guarded(n * C, torch.float32, dev)
    check(lib().elvis_groupnorm_affine(ptr(sums_d), ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(pa), ptr(pb),
                                       n, hw, C, groups, eps, stream_handle(dev)), dev)
    torch.cuda.synchronize()
    _guard_ok(pa, n * C, cid)
    _guard_ok(pb, n * C, cid)
    return pa, pb


def _run_gn_affine(c, dev):
    sums, gam, bet, sc, sh = affine_inputs(c, _gen(c))
    eps = float(np.float32(c.eps))
    pa, pb = _affine_call(sums.to(dev), gam, bet, sc, sh, c.n, c.hw, c.c, c.groups, eps, dev, c.id)
    name = "gn_affine_kernel"
    y = torch.stack([pa[:c.n * c.c].view(c.n, c.c), pb[:c.n * c.c].view(c.n, c.c)]).double().cpu()
    f64 = lambda t: None if t is None else t.double()
    return name, y, R.gn_affine_ref(sums, f64(gam), f64(bet), f64(sc), f64(sh), c.hw, c.groups, eps)


def _apply(xbuf_or_x, c_, n, hw, case, pa_ptr, pb_ptr, dev, *, pitch_in, inplace_buf=None):
    """elvis_affine_act of one tensor; returns the logical output [n, hw, c_] float64."""
    from elvis_amd._lib import lib, check, ptr, stream_handle
    dtype, code = _dt(case.dt)
    rows = n * hw
    if inplace_buf is not None:
        out, pout, src = inplace_buf, pitch_in, inplace_buf
    else:
        pout = R.pitch_for(c_) + case.out_extra
        out, src = _out_buffer(rows, c_, pout, dtype, dev), xbuf_or_x
    check(lib().elvis_affine_act(ptr(src), ptr(out), code, n, hw, c_, pitch_in, pout, pa_ptr, pb_ptr, case.act,
                                 stream_handle(dev)), dev)
    name = _last_launch()
    torch.cuda.synchronize()
    return name, _take(out, rows, c_, R.pitch_for(c_), case.id).view(n, hw, c_)


def _run_gn_e2e(c, dev):
    dtype, _ = _dt(c.dt)
    g = _gen(c)
    cs = [c.c] + ([c.c2] if c.c2 else [])
    assert len(cs) == 1 or c.n == 1, "the virtual concat applies pa / pb slices: one image"
    ctot = sum(cs)
    xs = [c.mean + torch.randn(c.n, c.hw, ci, generator=g) + 0.3 * torch.randn(1, 1, ci, generator=g) for ci in cs]
    sums = torch.full((c.n, ctot, 2), float("nan"), dtype=torch.float64, device=dev)
    bufs, off = [], 0
    for x, ci in zip(xs, cs):
        if c.inplace:
            pin = R.pitch_for(ci) + 8
            xd = _inplace_buffer(x.reshape(-1, ci), ci, pin, dtype, dev)
            from elvis_amd._lib import lib, check, ptr, stream_handle
            _, code = _dt(c.dt)
            ws = _guarded(lib().elvis_groupnorm_workspace_floats(code, c.n, c.hw, ci), torch.float32, dev)
            check(lib().elvis_groupnorm_sums(ptr(xd), code, c.n, c.hw, ci, pin, ptr(sums), ctot, off, ptr(ws),
                                             stream_handle(dev)), dev)
        else:
            pin = R.pitch_for(ci) + c.pitch_extra
            xd = _sums_call(x, ci, c.dt, c.pitch_extra, sums, ctot, off, dev, c.id)
        bufs.append((xd, pin))
        off += ci
    gam, bet = (torch.rand(ctot, generator=g) + 0.5).float(), (torch.randn(ctot, generator=g) * 0.3).float()
    sc = (torch.randn(ctot, generator=g) * 0.3).float() if c.scale else None
    sh = (torch.randn(ctot, generator=g) * 0.3).float() if c.shift else None
    eps = float(np.float32(c.eps))
    pa, pb = _affine_call(sums, gam, bet, sc, sh, c.n, c.hw, ctot, c.groups, eps, dev, c.id)
    outs, off = [], 0
    for (xd, pin), ci in zip(bufs, cs):
        name, y = _apply(xd, ci, c.n, c.hw, c, pa.data_ptr() + 4 * off, pb.data_ptr() + 4 * off, dev, pitch_in=pin,
                         inplace_buf=xd if c.inplace else None)
        outs.append(y)
        off += ci
    f64 = lambda t: None if t is None else t.double()
    b = R.groupnorm_ref([x.to(dtype).double() for x in xs], c.dt == "f16", f64(gam), f64(bet), f64(sc), f64(sh), c.groups,
                        eps, c.act)
    return name, torch.cat(outs, -1), b


def _run_affine_act(c, dev):
    dtype, _ = _dt(c.dt)
    g = _gen(c)
    if c.kind == "sat":
        x = torch.tensor([-100.0, -20.0, 0.0, 20.0, 100.0])[torch.randint(0, 5, (c.n, c.hw, c.c), generator=g)]
        pa, pb = torch.ones(c.n, c.c), torch.zeros(c.n, c.c)
    else:
        x = torch.randn(c.n, c.hw, c.c, generator=g) * 2.0
        pa, pb = (torch.randn(c.n, c.c, generator=g) * 1.5).float(), torch.randn(c.n, c.c, generator=g).float()
    pin = R.pitch_for(c.c) + c.pitch_extra + (8 if c.inplace else 0)
    pad, pbd = pa.float().to(dev), pb.float().to(dev)
    if c.inplace:
        xd = _inplace_buffer(x.reshape(-1, c.c), c.c, pin, dtype, dev)
        name, y = _apply(xd, c.c, c.n, c.hw, c, pad.data_ptr(), pbd.data_ptr(), dev, pitch_in=pin, inplace_buf=xd)
    else:
        xd = _pitched(x, pin, dtype, dev)
        name, y = _apply(xd, c.c, c.n, c.hw, c, pad.data_ptr(), pbd.data_ptr(), dev, pitch_in=pin)
    b = R.affine_act_ref(x.to(dtype).double(), pa.float().double(), pb.float().double(), c.act, c.dt == "f16")
    if c.kind == "sat":
        assert not bool(torch.isnan(y).any()), f"{c.id}: NaN from a saturated SiLU"
        assert bool((y[x.to(dtype).double() == -100.0] == 0).all()), f"{c.id}: silu(-100) must be (-)0"
    return name, y, b


def _run_layernorm(c, dev):
    from elvis_amd._lib import lib, check, ptr, stream_handle
    dtype, code = _dt(c.dt)
    g = _gen(c)
    T, C = c.hw, c.c
    if c.kind == "const":
        x = (torch.randn(T, 1, generator=g) * 3.0).expand(T, C).clone()
    elif c.kind == "offset":
        x = 100.0 + 0.1 * torch.randn(T, C, generator=g)
    else:
        x = torch.randn(T, C, generator=g) * 1.5 + 0.5 * torch.randn(T, 1, generator=g)
    gam, bet = (torch.rand(C, generator=g) + 0.5).float(), (torch.randn(C, generator=g) * 0.2).float()
    eps = float(np.float32(c.eps))
    pin = R.pitch_for(C) + c.pitch_extra + (8 if c.inplace else 0)
    if c.inplace:
        xd = _inplace_buffer(x, C, pin, dtype, dev)
        out, pout = xd, pin
    else:
        xd = _pitched(x, pin, dtype, dev)
        pout = R.pitch_for(C) + c.out_extra
        out = _out_buffer(T, C, pout, dtype, dev)
    gd, bd = gam.to(dev), bet.to(dev)
    check(lib().elvis_layernorm(ptr(xd), ptr(out), code, T, C, pin, pout, ptr(gd), ptr(bd), eps, stream_handle(dev)), dev)
    name = _last_launch()
    torch.cuda.synchronize()
    y = _take(out, T, C, R.pitch_for(C), c.id)
    return name, y, R.layernorm_ref(x.to(dtype).double(), gam.double(), bet.double(), eps, c.dt == "f16")


def _run_bicubic(c, dev):
    from elvis_amd._lib import lib, check, ptr, stream_handle
    dtype, code = _dt(c.dt)
    x = torch.randn(c.n, c.h, c.w, c.c, generator=_gen(c))
    pin = R.pitch_for(c.c) + c.pitch_extra
    pout = R.pitch_for(c.c) + c.pitch_extra
    xd = _pitched(x, pin, dtype, dev)
    rows = c.n * c.h * c.sf * c.w * c.sf
    out = _out_buffer(rows, c.c, pout, dtype, dev)
    check(lib().elvis_bicubic_upsample(ptr(xd), ptr(out), code, c.n, c.h, c.w, c.c, pin, pout, c.sf, stream_handle(dev)), dev)
    name = _last_launch()
    torch.cuda.synchronize()
    y = _take(out, rows, c.c, pout, c.id).view(c.n, c.h * c.sf, c.w * c.sf, c.c)
    return name, y, R.bicubic_ref(x.to(dtype).double(), c.sf, c.dt == "f16")


RUN = {"gn_sums": _run_gn_sums, "partials": _run_partials, "gn_affine": _run_gn_affine, "gn_e2e": _run_gn_e2e,
       "affine_act": _run_affine_act, "layernorm": _run_layernorm, "bicubic": _run_bicubic}


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_norm_misc_matrix(gpu_device, case):
    name, y, b = RUN[case.op](case, gpu_device)
    assert name == case.expect, f"{case.id}: launched {name!r}, the case exists for {case.expect!r}"
    assert y.shape == b.ref.shape
    ok1, worst, at = R.tier1(y, b)
    line = f"{case.id}: {name} tier1 worst {worst:.3f}"
    frac = None
    if b.e2 is not None and b.out_f16:
        frac, share = R.tier2(y, b), R.exact_share(y, b)
        floor, near = R.exact_share_floor(b)
        line += f" tier2 {frac:.5f} exact {share:.5f} (floor {floor:.3f}, near a midpoint {near:.5f})"
    print(line)
    assert ok1, (f"{line}: tier 1 fails at {tuple(int(i) for i in at)}: y {float(y[at]):.9g} ref {float(b.ref[at]):.9g} "
                 f"bound {float(b.bound()[at]):.3g}")
    if frac is not None:
        assert frac >= R.TIER2_FLOOR, f"{line} below the floor {R.TIER2_FLOOR}"
        assert share >= floor, f"{line}: fewer correctly rounded outputs than the reference allows"


@pytest.mark.parametrize("tiles", [1, 255, 256, 257, 1000])
def test_partials_reduce4_equals_scalar_bit_for_bit(gpu_device, tiles):
    """gn_partials_reduce4_kernel adds every channel's partials in the order of gn_partials_reduce_kernel: the same
    partials through the aligned pointer (reduce4) and through a copy shifted by 4 bytes (scalar) give the same bits."""
    c = R.Case(id=f"bits_t{tiles}", op="partials", expect="", c=64, tiles=tiles, n=2, seed=900 + tiles)
    p, aligned = _partials(c, gpu_device, False)
    _, shifted = _partials(c, gpu_device, True)
    n4, y4 = _partials_call(c, aligned, gpu_device)
    n1, y1 = _partials_call(c, shifted, gpu_device)
    assert (n4, n1) == ("gn_partials_reduce4_kernel", "gn_partials_reduce_kernel")
    assert R.bits_equal(y4.numpy(), y1.numpy()), f"tiles {tiles}: reduce4 and the scalar reduction differ"
    assert R.tier1(y4, R.partials_ref(p.double()))[0]


# ------------------------------------------------------------------------------------------------------- exact ops
def _np_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


VQ_CASES = [(3, 3000, "f32", 1025, ""), (3, 3000, "f16", 63, ""), (1, 1, "f32", 1, ""), (2, 2, "f16", 3, ""),
            (4, 3, "f32", 4, ""), (1, 5, "f16", 63, ""), (2, 255, "f32", 1025, ""), (4, 1024, "f16", 1025, ""),
            (3, 1025, "f32", 63, ""), (4, 8192, "f32", 1025, ""), (3, 8192, "f16", 4, "noidx"),
            (3, 1024, "f32", 63, "dup_same"), (3, 1024, "f16", 63, "dup_other"), (2, 255, "f32", 63, "equidistant"),
            (1, 3000, "f32", 3, "equidistant")]


@pytest.mark.parametrize("c,n_embed,dt,pixels,kind", VQ_CASES, ids=[f"vq_c{a}_k{b}_{d}_p{e}{'_' + k if k else ''}" for a, b, d, e, k in VQ_CASES])
def test_vq_nearest_exact(gpu_device, c, n_embed, dt, pixels, kind):
    from elvis_amd._lib import lib, check, ptr, stream_handle
    dev = gpu_device
    dtype, code = _dt(dt)
    g = torch.Generator().manual_seed(8000 + c * 10007 + n_embed + pixels)
    cb = torch.randn(n_embed, c, generator=g).float()
    z = torch.randn(pixels, c, generator=g)
    if kind in ("dup_same", "dup_other"):
        # every pixel sits on a code that exists twice: in one quarter (Q = 256) or in two - the lower index must win
        Q = (n_embed + 3) // 4
        lo = torch.randint(0, Q // 2, (pixels,), generator=g)
        hi = lo + (Q // 2 if kind == "dup_same" else 2 * Q + 7)
        cb[hi] = cb[lo]
        z = cb[lo].clone()
        if dt == "f16":
            cb = cb.half().float()
            z = cb[lo].clone()
    if kind == "equidistant":
        # integer codes, pixels exactly half way between two neighbouring ones
        cb = torch.arange(n_embed).float()[:, None].repeat(1, c)
        cb = cb[torch.randperm(n_embed, generator=g)]
        z = (torch.randint(0, n_embed - 1, (pixels, 1), generator=g).float() + 0.5).repeat(1, c)
    pin, pout = R.pitch_for(c) + 8, R.pitch_for(c) + 8
    zd = _pitched(z, pin, dtype, dev)
    out = _out_buffer(pixels, c, pout, dtype, dev)
    idx = _guarded(pixels, torch.int32, dev, fill=-7) if kind != "noidx" else None
    cbd = cb.contiguous().to(dev)
    check(lib().elvis_vq_nearest(ptr(zd), ptr(out), ptr(idx), code, pixels, c, pin, pout, ptr(cbd), n_embed,
                                 stream_handle(dev)), dev)
    assert _last_launch() == f"vq_nearest_kernel<{'half' if dt == 'f16' else 'float'}>"
    torch.cuda.synchronize()
    ridx, rzq = R.vq_ref(z.to(dtype).float().numpy(), cb.numpy())
    if kind.startswith("dup"):
        assert bool((torch.from_numpy(ridx).long() == lo).all())
    got = out.cpu()
    assert bool((got[:pixels, c:] == 0).all()) and bool((got[pixels] == SENTINEL).all())
    if idx is not None:
        _guard_ok(idx, pixels, "vq")
        bad = np.nonzero(idx[:pixels].cpu().numpy() != ridx)[0]
        assert bad.size == 0, f"pixel {bad[0]}: index {int(idx[bad[0]])}, reference {ridx[bad[0]]}"
    assert R.bits_equal(got[:pixels, :c].numpy(), R.np_store(rzq, dt == "f16")), "zq differs from from_f(codebook[idx])"


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("pitch", [8, 16])
def test_u8_to_float_exact(gpu_device, dt, pitch):
    """All 256 values in every channel position x div255 x swap x the scale / bias of both call sites."""
    from elvis_amd._lib import lib, check, ptr, stream_handle
    dev = gpu_device
    dtype, code = _dt(dt)
    v = np.arange(256, dtype=np.uint8)
    src = np.stack([v, np.roll(v, 85), np.roll(v, 170)], -1).reshape(1, 16, 16, 3)
    for div255 in (0, 1):
        for swap in (0, 1):
            for scale, bias in ((2.0, -1.0), (1.0, 0.0)):
                out = _out_buffer(256, 0, pitch, dtype, dev)
                out[:256] = float("nan")
                sd = _np_dev(src, dev)
                check(lib().elvis_u8_to_float(ptr(sd), ptr(out), code, 1, 16, 16, pitch, scale, bias, swap, div255,
                                              stream_handle(dev)), dev)
                assert _last_launch() == f"u8_to_float_kernel<{'half' if dt == 'f16' else 'float'}>"
                torch.cuda.synchronize()
                ref = R.u8_to_float_ref(src.reshape(256, 3), scale, bias, swap, div255, dt == "f16", pitch)
                got = out.cpu().numpy()
                assert (got[256] == SENTINEL).all()
                assert R.bits_equal(got[:256], ref), f"div255 {div255} swap {swap} scale {scale}"


def f2u8_inputs(dt):
    """[P, 3] float32 of values storable in `dt`: the t with t * 255 exactly on k + 0.5 (even and odd k), their
    neighbours, values outside [0, 1], infinities, NaN, and a random tail."""
    ties = R.half_ties(range(0, 255))
    assert any(k % 2 == 0 for k in ties) and any(k % 2 == 1 for k in ties)
    vals = [t for k in sorted(ties) for t in ties[k]]
    vals += [-0.25, -1e-8, 0.0, 1.0, 1.0000001, 1.5, 300.0, float("inf"), float("-inf"), float("nan"), 0.5, 1 / 255.0]
    vals = np.array(vals, np.float32)
    rnd = np.random.default_rng(5).random(3000).astype(np.float32) * 1.2 - 0.1
    a = np.concatenate([vals, rnd])
    if dt == "f16":
        # f16 sources: every f16 in [0, 1] whose float32 product with 255 is a tie, plus the list above rounded
        h = np.arange(0, 0x3C01, dtype=np.uint16).view(np.float16).astype(np.float32)
        q = h * np.float32(255.0)
        tie = h[(q - np.floor(q)) == 0.5]
        with np.errstate(over="ignore"):
            a = np.concatenate([tie, a.astype(np.float16).astype(np.float32)])
    a = a[: a.size // 3 * 3]
    return a.reshape(-1, 3)


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("mode", [0, 1])
def test_float_to_u8_exact(gpu_device, dt, mode):
    from elvis_amd._lib import lib, check, ptr, stream_handle
    dev = gpu_device
    dtype, code = _dt(dt)
    a = f2u8_inputs(dt)
    P = a.shape[0]
    for swap in (0, 1):
        for scale, bias, side in ((1.0, 0.0, True), (0.5, 0.5, False)):
            xd = _pitched(torch.from_numpy(a), 8, dtype, dev)
            dst = torch.full((P * 3 + 16,), 99, dtype=torch.uint8)
            dst[:P * 3] = 77
            dst = dst.to(dev)
            f32 = _guarded(P * 3, torch.float32, dev) if side else None
            check(lib().elvis_float_to_u8(ptr(xd), code, ptr(dst), ptr(f32), 1, 1, P, 8, scale, bias, mode, swap,
                                          stream_handle(dev)), dev)
            assert _last_launch() == f"float_to_u8_kernel<{'half' if dt == 'f16' else 'float'}>"
            torch.cuda.synchronize()
            ru8, rt = R.float_to_u8_ref(a, scale, bias, mode, swap)
            got = dst.cpu().numpy()
            assert (got[P * 3:] == 99).all()
            bad = np.nonzero(got[:P * 3].reshape(P, 3) != ru8)
            assert bad[0].size == 0, (f"mode {mode} swap {swap}: src {a[bad[0][0]]} -> {got[:P * 3].reshape(P, 3)[bad[0][0]]}, "
                                      f"reference {ru8[bad[0][0]]}")
            if side:
                _guard_ok(f32, P * 3, "float_to_u8")
                assert R.bits_equal(f32[:P * 3].cpu().numpy().reshape(P, 3), rt), "the f32 side output is not the clamped value"
    # NaN -> 0 (fmaxf returns the other operand): pinned
    nan_rows = np.isnan(a).any(1)
    assert nan_rows.any() and (R.float_to_u8_ref(a, 1.0, 0.0, mode, 0)[0][np.isnan(a)] == 0).all()


PAD_CASES = [(5, 7, 0, 0, False, 0, 0), (5, 7, 1, 1, True, 0, 0), (5, 7, 4, 6, True, 0, 0), (6, 4, 5, 3, False, 8, 16),
             (3, 9, 2, 8, True, 4, 8), (1, 1, 0, 0, True, 0, 0)]


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("h,w,ph,pw,with_add,coff,extra", PAD_CASES)
def test_pad_reflect_axpy_exact(gpu_device, dt, h, w, ph, pw, with_add, coff, extra):
    """Padding 0, 1 and the largest allowed (h - 1, w - 1); into a channel slice of a sentinel-filled wider tensor only
    [coff, coff + c) may change."""
    from elvis_amd._lib import lib, check, ptr, stream_handle
    dev = gpu_device
    dtype, code = _dt(dt)
    n, c = 2, 3
    g = torch.Generator().manual_seed(h * 100 + w * 10 + ph + pw)
    x = torch.randn(n, h, w, c, generator=g)
    hp, wp = h + ph, w + pw
    add = torch.randn(n, c, hp, wp, generator=g).float() if with_add else None
    mul, add_mul = float(np.float32(0.7071)), float(np.float32(1.3))
    pout = R.pitch_for(coff + c) + extra
    xd = _pitched(x, 8, dtype, dev)
    out = torch.full((n * hp * wp + 1, pout), SENTINEL, dtype=dtype)
    out[:-1, coff:coff + c] = float("nan")
    out = out.to(dev)
    ad = add.to(dev) if with_add else None
    check(lib().elvis_pad_reflect_axpy(ptr(xd), ptr(out), code, n, h, w, c, 8, hp, wp, pout, coff, mul, ptr(ad), add_mul,
                                       stream_handle(dev)), dev)
    assert _last_launch() == f"pad_reflect_axpy_kernel<{'half' if dt == 'f16' else 'float'}>"
    torch.cuda.synchronize()
    got = out.cpu()
    keep = torch.ones(pout, dtype=torch.bool)
    keep[coff:coff + c] = False
    assert bool((got[:, keep] == SENTINEL).all()) and bool((got[-1] == SENTINEL).all()), "written outside [coff, coff + c)"
    ref = R.pad_reflect_axpy_ref(x.to(dtype).float().numpy(), hp, wp, mul, add.numpy() if with_add else None, add_mul, dt == "f16")
    assert R.bits_equal(got[:-1, coff:coff + c].numpy().reshape(n, hp, wp, c), ref)


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("h_in,w_in,h,w,c,pin,pout", [(6, 7, 6, 7, 3, 8, 8), (6, 7, 1, 1, 5, 8, 16), (9, 5, 4, 3, 12, 24, 16)])
def test_crop_copy_exact(gpu_device, dt, h_in, w_in, h, w, c, pin, pout):
    from elvis_amd._lib import lib, check, ptr, stream_handle
    dev = gpu_device
    dtype, code = _dt(dt)
    n = 2
    x = torch.randn(n, h_in, w_in, c, generator=torch.Generator().manual_seed(h * w))
    xd = _pitched(x, pin, dtype, dev)
    out = _out_buffer(n * h * w, c, pout, dtype, dev)
    check(lib().elvis_crop_copy(ptr(xd), ptr(out), code, n, h_in, w_in, pin, h, w, c, pout, stream_handle(dev)), dev)
    assert _last_launch() == f"crop_copy_kernel<{'half' if dt == 'f16' else 'float'}>"
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[-1] == SENTINEL).all()
    ref = R.crop_ref(x.to(dtype).numpy(), h, w, c, pout)
    assert R.bits_equal(got[:-1].reshape(n, h, w, pout), ref)


def test_convert_act_exact(gpu_device):
    """f16 -> f32 over all 65536 bit patterns; f32 -> f16 over every f16 value, every rounding midpoint and its fp32
    neighbours, the subnormal range, overflow to inf, NaN.  Bit for bit against numpy astype (NaN as NaN)."""
    from elvis_amd._lib import lib, check, ptr, stream_handle, F16, F32
    dev = gpu_device
    h = np.arange(0x10000, dtype=np.uint32).astype(np.uint16).view(np.float16)
    xd = _np_dev(h, dev)
    out = _guarded(h.size, torch.float32, dev)
    check(lib().elvis_convert_act(ptr(xd), F16, ptr(out), F32, h.size // 8, 8, stream_handle(dev)), dev)
    assert _last_launch() == "convert_act_kernel<half,float>"
    torch.cuda.synchronize()
    _guard_ok(out, h.size, "convert f16 -> f32")
    assert R.bits_equal(out[:h.size].cpu().numpy(), R.convert_ref(h, False), nan_as_nan=True)
    a = R.f32_to_f16_inputs()
    xd = _np_dev(a, dev)
    out = _guarded(a.size, torch.float16, dev)
    check(lib().elvis_convert_act(ptr(xd), F32, ptr(out), F16, a.size // 8, 8, stream_handle(dev)), dev)
    assert _last_launch() == "convert_act_kernel<float,half>"
    torch.cuda.synchronize()
    _guard_ok(out, a.size, "convert f32 -> f16")
    got, ref = out[:a.size].cpu().numpy(), R.convert_ref(a, True)
    bad = np.nonzero(~((got.view(np.uint16) == ref.view(np.uint16)) | (np.isnan(got) & np.isnan(ref))))[0]
    assert bad.size == 0, f"{a[bad[0]]!r} -> {got[bad[0]]!r}, reference {ref[bad[0]]!r} ({bad.size} differ)"


# ------------------------------------------------------------------------------------------------------- validation
def test_norm_entry_points_reject_misaligned_pointers(gpu_device):
    """elvis_groupnorm_sums, elvis_affine_act and elvis_layernorm move 16-byte vectors: a data pointer off 16 bytes is
    a ValueError before anything launches.  Misaligned pointers go to these validated entry points only."""
    from elvis_amd._lib import lib, check, ptr, stream_handle, F16, F32
    dev = gpu_device
    s = stream_handle(dev)
    n, hw, c = 1, 64, 64
    x = torch.zeros(n * hw * c + 64, dtype=torch.float16, device=dev)
    y = torch.zeros(n * hw * c + 64, dtype=torch.float16, device=dev)
    xf = torch.zeros(n * hw * c + 64, dtype=torch.float32, device=dev)
    yf = torch.zeros(n * hw * c + 64, dtype=torch.float32, device=dev)
    sums = torch.zeros(n, c, 2, dtype=torch.float64, device=dev)
    ws = torch.zeros(lib().elvis_groupnorm_workspace_floats(F16, n, hw, c) + 64, device=dev)
    pa, pb = torch.ones(n, c, device=dev), torch.zeros(n, c, device=dev)
    calls = {
        "sums": lambda xp, yp, code: lib().elvis_groupnorm_sums(xp, code, n, hw, c, c, ptr(sums), c, 0, ptr(ws), s),
        "affine_act": lambda xp, yp, code: lib().elvis_affine_act(xp, yp, code, n, hw, c, c, c, ptr(pa), ptr(pb), 2, s),
        "layernorm": lambda xp, yp, code: lib().elvis_layernorm(xp, yp, code, n * hw, c, c, c, ptr(pa), ptr(pb), 1e-5, s),
    }
    for name, call in calls.items():
        for code, xi, yi in ((F16, x, y), (F32, xf, yf)):
            check(call(ptr(xi), ptr(yi), code), dev)          # aligned: accepted
            torch.cuda.synchronize()
            before = _last_launch()
            offs = ((2, 0), (8, 0)) if name == "sums" else ((2 if code == F16 else 4, 0), (8, 0), (0, 8), (0, 4))
            for dx, dy in offs:
                with pytest.raises(ValueError):
                    check(call(ptr(xi) + dx, ptr(yi) + dy, code), dev)
                assert _last_launch() == before, f"{name}: a launch was recorded for offsets {dx}, {dy}"
    torch.cuda.synchronize()
