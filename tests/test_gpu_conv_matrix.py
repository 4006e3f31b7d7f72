"""Every production-reachable conv kernel instantiation against the float64 error-bounded reference of
tests/_convref.py: tier 1 on every element, tier 2 on >= 99.8 % of each f16 case, the per-tile fused
GroupNorm partials, and the [cout, pitch) pad channels of an output pre-filled with NaN.  Each case
asserts, before it runs, the instantiation it must reach (the library's name query for the call's real
residual / statistics flags) and, after, that ops reported the same name for the launch and that the leaf launcher
which really ran recorded it too (elvis_last_launch: the name query walks the launch tree without launching, this is
the launch itself)."""
import math

import pytest
import torch

import _convref as R

pytestmark = pytest.mark.gpu


def _to_act(x_nchw, dtype, dev, pitch=None):
    from elvis_amd import ops
    n, c, h, w = x_nchw.shape
    p = pitch or ops.pitch_for(c)
    t = torch.zeros((n, h, w, p), dtype=dtype, device=dev)
    t[..., :c] = x_nchw.permute(0, 2, 3, 1).to(dev, dtype)
    return ops.Act(t, c)


def _nan_new_act(orig):
    def new_act(n, h, w, c, dtype, device, zero=None):
        a = orig(n, h, w, c, dtype, device, zero=zero)
        a.t.fill_(float("nan"))   # every element, pads included, must be written by the conv
        return a
    return new_act


def _run(case, dev):
    """Runs the case on the GPU; returns (y_stored NCHW float64, pads, stats or None, Ref, kernel names ops reported,
    the kernel the last conv call launched)."""
    from elvis_amd import ops
    from elvis_amd._lib import lib
    c = case
    g = torch.Generator().manual_seed(1000 + c.seed)
    dtype = torch.float16 if c.dt == "f16" else torch.float32
    f16 = c.dt == "f16"
    cin_tot = c.cin + c.cin2
    kk = c.ksize if c.kind == "conv" else 3
    x = torch.randn(c.n, c.cin, c.h, c.w, generator=g).to(dtype)
    x2 = torch.randn(c.n, c.cin2, c.h, c.w, generator=g).to(dtype) if c.cin2 else None
    wt = torch.randn(c.cout, cin_tot, kk, kk, generator=g) / math.sqrt(kk * kk * cin_tot)
    b = torch.randn(c.cout, generator=g) * 0.1
    pa = torch.rand(c.n, cin_tot, generator=g) + 0.5 if c.prologue else None
    pb = torch.randn(c.n, cin_tot, generator=g) * 0.2 if c.prologue else None
    x64 = torch.cat([x, x2], 1).double() if x2 is not None else x.double()
    cast_w = (lambda w: w.half().double()) if f16 else (lambda w: w.double())
    ops.CONV_PROFILER = names_ev = []
    try:
        if c.kind == "conv":
            with ops.x3_default(c.dt == "x3"):
                conv = ops.PackedConv(wt, b, dtype, dev, c.cin, c.cin2)
            xa = _to_act(x, dtype, dev)
            xb = _to_act(x2, dtype, dev) if x2 is not None else None
            ra = None
            pro = (pa.to(dev), pb.to(dev)) if c.prologue else None
            # reference operands
            if c.prologue:
                x_hat, perr = R.prologue_f64(x64, pa.double(), pb.double(), f16)
            else:
                x_hat, perr = x64, None
            pad = (c.ksize // 2) if c.pad is None else c.pad
            down_pad0 = c.stride == 2 and pad == 0 and c.ho is not None
            r = R.conv_ref(x_hat, cast_w(wt), b.double(), None, ksize=c.ksize, stride=c.stride, pad=pad,
                           upsample=c.upsample, act=c.act, out_f16=f16, pro_err=perr, x3=c.dt == "x3", down_pad0=down_pad0)
            if c.residual:
                res = torch.randn(r.z.shape, generator=g).to(dtype)
                ra = _to_act(res, dtype, dev, pitch=c.pitch_out + c.res_pitch_extra)
                r.res = res.double()
                r.A = r.A + r.res.abs()
            orig = ops.new_act
            ops.new_act = _nan_new_act(orig)
            try:
                y = conv(xa, xb, stride=c.stride, pad=c.pad, upsample=c.upsample, act=c.act, residual=ra, prologue=pro,
                         ho=c.ho, wo=c.wo, want_stats=c.stats)
            finally:
                ops.new_act = orig
        elif c.kind == "up":
            with ops.x3_default(c.dt == "x3"):
                up = ops.PackedUpConv(wt, b, dtype, dev, c.cin)
            xa = _to_act(x, dtype, dev)
            w2 = [cast_w(w) for w in R.up_weights(wt)]
            r = R.upconv_ref(x64, w2, b.double(), act=c.act, out_f16=f16, x3=c.dt == "x3")
            orig = ops.new_act
            ops.new_act = _nan_new_act(orig)
            try:
                y = up(xa, want_stats=c.stats, act=c.act)
            finally:
                ops.new_act = orig
        else:
            down = ops.PackedDownConv(wt, b, dtype, dev, c.cin, pad1=c.pad1)
            xa = _to_act(x, dtype, dev)
            r = R.conv_ref(x64, cast_w(wt), b.double(), None, ksize=3, stride=2, pad=1 if c.pad1 else 0, act=c.act,
                           out_f16=f16, x3=c.dt == "x3", kt=16 * c.cin, down_pad0=not c.pad1)
            orig = ops.new_act
            ops.new_act = _nan_new_act(orig)
            try:
                y = down(xa, want_stats=c.stats, act=c.act)
            finally:
                ops.new_act = orig
        last = lib().elvis_last_launch().decode()   # read once after the op: an up-conv's four calls reach one instantiation
        torch.cuda.synchronize()
        names = [e[0] for e in names_ev]
    finally:
        ops.CONV_PROFILER = None
    t = y.t.double().cpu()
    yn = t[..., :c.cout].permute(0, 3, 1, 2).contiguous()
    pads = t[..., c.cout:]
    st = y.stats.cpu() if y.stats is not None else None
    return yn, pads, st, r, names, last


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_conv_matrix(gpu_device, case):
    # the instantiation the case exists for, asserted before anything runs
    got_names = R.resolve(case)
    assert set(got_names) == {case.expect}, f"{case.id}: resolves to {got_names}, expected {case.expect}"
    y, pads, st, r, launched, last = _run(case, gpu_device)
    assert launched and set(launched) == {case.expect}, f"ops reported {launched}"
    assert last == case.expect, f"{case.id}: launched {last}"
    assert y.shape == r.z.shape
    ok1, worst, at = R.tier1(y, r)
    line = f"{case.id}: {case.expect} tier1 worst {worst:.3f}"
    if case.dt == "f16":
        frac = R.tier2(y, r)
        line += f" tier2 {frac:.5f}"
    print(line)
    assert ok1, f"{line}: tier 1 fails at {at}: y {float(y[at]):.7g} ref {float(r.ref[at]):.7g} bound {float(r.bound()[at]):.3g}"
    if case.dt == "f16":
        assert frac >= R.TIER2_FLOOR, line
    # pad channels [cout, pitch) are written as zeros (the output started as NaN)
    assert pads.numel() == 0 or bool((pads == 0).all()), f"{case.id}: pad channels not zeroed"
    if case.stats:
        assert st is not None, "no fused statistics"
        ty = R.kernel_ty(case.expect)
        if case.kind == "up":
            # PackedUpConv: [n][parity][tile] rows, each parity on the low-res grid
            parts = [R.tile_stats_ref(y, ty, parity=k) for k in range(4)]
            tpi = parts[0].shape[0] // case.n
            ref = torch.cat([p[i * tpi:(i + 1) * tpi] for i in range(case.n) for p in parts], 0)
        else:
            ref = R.tile_stats_ref(y, ty)
        assert st.shape == (ref.shape[0], case.cout, 2), f"stats shape {tuple(st.shape)} vs {tuple(ref.shape[:2])}"
        ok, sw = R.stats_check(st, ref)
        print(f"{case.id}: stats worst {sw:.3f}")
        assert ok, f"{case.id}: per-tile statistics off (worst ratio {sw:.3f})"
