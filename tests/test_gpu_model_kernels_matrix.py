"""Window attention, fused Swin and DCNv2 against the float64 error-bounded references of tests/_modelref.py: tier 1 on
every element, tier 2 on the f16 outputs of Swin and of the DCNv2 tile kernel.  Every case calls the C ABI on the
default dispatch, asserts through elvis_last_launch the one instantiation it reached, and hands the kernel an output
buffer that is NaN on its logical elements and a sentinel on the pitch padding and on one guard row past the end: every
logical element must be written and nothing else."""
import math

import numpy as np
import pytest
import torch

import _modelref as R

pytestmark = pytest.mark.gpu

SENTINEL = 1234.0


def _last_launch():
    from elvis_amd._lib import lib
    return lib().elvis_last_launch().decode()


def _pitched(rows_nhwc: torch.Tensor, pitch: int, dtype, dev, pad=float("nan")):
    """[..., c] -> a device tensor [..., pitch] holding the values, `pad` beyond c."""
    c = rows_nhwc.shape[-1]
    t = torch.full(rows_nhwc.shape[:-1] + (pitch,), pad, dtype=dtype)
    t[..., :c] = rows_nhwc.to(dtype)
    return t.to(dev)


def _out_buffer(rows: int, c: int, pitch: int, dtype, dev):
    """[rows + 1, pitch]: NaN on [0, c) of the first `rows` rows, the sentinel elsewhere (pads and the guard row)."""
    t = torch.full((rows + 1, pitch), SENTINEL, dtype=dtype)
    t[:rows, :c] = float("nan")
    return t.to(dev)


def _split_out(buf: torch.Tensor, rows: int, c: int, case_id: str):
    """The logical [rows, c] values (float64, CPU); asserts that nothing outside them was touched."""
    b = buf.double().cpu()
    assert bool((b[:rows, c:] == SENTINEL).all()), f"{case_id}: written into the pitch padding [c, pitch)"
    assert bool((b[rows] == SENTINEL).all()), f"{case_id}: written past the last row"
    return b[:rows, :c]


# ------------------------------------------------------------------------------------------------------- runners
def _run_attn(c, dev):
    from elvis_amd._lib import lib, check, ptr, stream_handle, F16, F32
    g = torch.Generator().manual_seed(2000 + c.seed)
    E = c.heads * 32
    dtype = torch.float16 if c.dt == "f16" else torch.float32
    qkv = torch.randn(c.n, c.h, c.w, 3 * E, generator=g)
    table = torch.randn(225, c.heads, generator=g) * 0.5
    if c.logits == "onehot":
        qkv[..., :2 * E] *= 3.0          # logits of std ~9: rows close to one-hot
    elif c.logits == "flat":
        qkv[..., :2 * E] *= 0.01         # logits ~0: flat rows (within each shift region)
        table *= 1e-3
    scale = float(np.float32(32 ** -0.5))
    qp, op = 3 * E + c.pitch_extra, E + c.out_extra
    qd = _pitched(qkv, qp, dtype, dev)
    td = table.float().to(dev)
    rows = c.n * c.h * c.w
    out = _out_buffer(rows, E, op, dtype, dev)
    check(lib().elvis_window_attention(ptr(qd), ptr(out), F16 if c.dt == "f16" else F32, c.n, c.h, c.w, c.heads, 32, 8,
                                       c.shift, qp, op, ptr(td), scale, stream_handle(dev)), dev)
    name = _last_launch()
    torch.cuda.synchronize()
    y = _split_out(out, rows, E, c.id).view(c.n, c.h, c.w, E)
    b = R.attention_ref(qkv.to(dtype).double(), c.heads, c.shift, table.float().double(), scale, f16=c.dt == "f16")
    return name, y, b


def _run_swin(c, dev):
    from elvis_amd import ops
    from elvis_amd._lib import lib, check, ptr, stream_handle
    g = torch.Generator().manual_seed(3000 + c.seed)
    C, M, n1 = c.c, c.tokens, c.n1
    rn = lambda *s: torch.randn(*s, generator=g)
    tok = lambda: c.offset + c.spread * rn(M, C) + 0.5 * rn(M, 1)
    x = tok() if c.mode != 2 else rn(M, C)            # PROJ: x is the attention output, y the residual stream
    y = tok() if c.mode == 2 else None
    gam, bet = torch.rand(C, generator=g) + 0.5, rn(C) * 0.2
    w1, b1 = rn(n1, C) / math.sqrt(C), rn(n1) * 0.1
    w2 = rn(C, n1) / math.sqrt(n1) if c.mode else None
    b2 = rn(C) * 0.1 if c.mode else None
    wp = rn(C, C) / math.sqrt(C) if c.mode == 2 else None
    bp = rn(C) * 0.1 if c.mode == 2 else None
    sf = ops.SwinFused(gam, bet, w1, b1, w2, b2, proj_w=wp, proj_b=bp, device=dev)
    xp, outc = C + c.pitch_extra, (n1 if c.mode == 0 else C)
    op = outc + c.out_extra
    xd = _pitched(x, xp, torch.float16, dev)
    out = _out_buffer(M, outc, op, torch.float16, dev)
    eps = float(np.float32(1e-5))
    s = stream_handle(dev)
    if c.mode == 0:
        check(lib().elvis_swin_ln_linear(ptr(xd), ptr(out), ptr(sf.packed), ptr(sf.b1), ptr(sf.gamma), ptr(sf.beta), M, C,
                                         n1, xp, op, eps, s), dev)
    elif c.mode == 1:
        check(lib().elvis_swin_mlp(ptr(xd), ptr(out), ptr(sf.packed), ptr(sf.b1), ptr(sf.b2), ptr(sf.gamma), ptr(sf.beta),
                                   M, C, n1, xp, op, eps, s), dev)
    else:
        yp = C + c.y_extra
        yd = _pitched(y, yp, torch.float16, dev)
        check(lib().elvis_swin_proj_mlp(ptr(xd), ptr(yd), ptr(out), ptr(sf.packed), ptr(sf.bp), ptr(sf.b1), ptr(sf.b2),
                                        ptr(sf.gamma), ptr(sf.beta), M, C, n1, xp, yp, op, eps, s), dev)
    name = _last_launch()
    torch.cuda.synchronize()
    got = _split_out(out, M, outc, c.id)
    h16 = lambda t: None if t is None else t.half().double()
    f64 = lambda t: None if t is None else t.float().double()
    b = R.swin_ref(c.mode, h16(x), f64(gam), f64(bet), h16(w1), f64(b1), h16(w2), f64(b2), y=h16(y), wp=h16(wp),
                   bp=f64(bp), eps=eps)
    return name, got, b


def _run_dcn(c, dev):
    from elvis_amd._lib import lib, check, ptr, stream_handle, F16, F32
    g = torch.Generator().manual_seed(4000 + c.seed)
    dtype = torch.float16 if c.dt == "f16" else torch.float32
    n, h, w, cin, dg = c.n, c.h, c.w, c.cin, c.dg
    x = torch.randn(n, h, w, cin, generator=g)
    off = R.dcn_offsets(c, g)
    mk = torch.randn(n, h, w, 9 * dg, generator=g) * 2.0 if c.sigmoid else torch.rand(n, h, w, 9 * dg, generator=g) * 2 - 0.5
    om = torch.cat([off, mk], -1)
    om_pitch = (27 * dg + 7) // 8 * 8
    wt = torch.randn(c.cout, cin * 9, generator=g) / math.sqrt(cin * 9)
    bias = torch.randn(c.cout, generator=g) * 0.1 if c.bias else None
    xd = _pitched(x, c.x_pitch, dtype, dev)
    omd = _pitched(om, om_pitch, dtype, dev)
    wd = wt.to(dtype).contiguous().to(dev)
    bd = bias.float().to(dev) if bias is not None else None
    rows = n * h * w
    op = (c.cout + 7) // 8 * 8 + c.out_extra
    out = _out_buffer(rows, c.cout, op, dtype, dev)
    check(lib().elvis_dcnv2(ptr(xd), ptr(omd), ptr(wd), ptr(bd), ptr(out), F16 if c.dt == "f16" else F32, n, h, w, cin,
                            c.x_pitch, dg, om_pitch, int(c.sigmoid), c.cout, op, c.act, stream_handle(dev)), dev)
    name = _last_launch()
    torch.cuda.synchronize()
    got = _split_out(out, rows, c.cout, c.id).view(n, h, w, c.cout)
    st = lambda t: t.to(dtype).double()
    b = R.dcn_ref(st(x), st(om), st(wt), bias.float().double() if bias is not None else None, dg, c.sigmoid,
                  tile=c.expect.startswith("dcnv2_tile"), f16_out=c.dt == "f16", act=c.act)
    return name, got, b


RUN = {"attn": _run_attn, "swin": _run_swin, "dcn": _run_dcn}


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_model_kernel_matrix(gpu_device, case):
    name, y, b = RUN[case.op](case, gpu_device)
    assert name == case.expect, f"{case.id}: launched {name!r}, the case exists for {case.expect!r}"
    assert y.shape == b.ref.shape
    ok1, worst, at = R.tier1(y, b)
    line = f"{case.id}: {name} tier1 worst {worst:.3f}"
    frac = None
    if b.e2 is not None and b.out_f16:
        frac = R.tier2(y, b)
        line += f" tier2 {frac:.5f}"
    print(line)
    assert ok1, (f"{line}: tier 1 fails at {tuple(int(i) for i in at)}: y {float(y[at]):.7g} ref {float(b.ref[at]):.7g} "
                 f"bound {float(b.bound()[at]):.3g}")
    if frac is not None:
        assert frac >= R.TIER2_FLOOR[case.op], f"{line} below the floor {R.TIER2_FLOOR[case.op]}"


def test_window_attention_rejects_bad_pitch_and_alignment(gpu_device):
    """The f16 kernels move 16-byte vectors: a pitch that is not a multiple of 8 or a pointer off 16 bytes is a
    ValueError before anything launches."""
    from elvis_amd._lib import lib, check, ptr, stream_handle, F16
    heads, E, h, w = 2, 64, 8, 8
    qkv = torch.zeros(h * w * (3 * E + 8) + 64, dtype=torch.float16, device=gpu_device)
    out = torch.zeros(h * w * (E + 8) + 64, dtype=torch.float16, device=gpu_device)
    table = torch.zeros(225, heads, device=gpu_device)
    call = lambda q, o, qp, op: check(lib().elvis_window_attention(q, o, F16, 1, h, w, heads, 32, 8, 4, qp, op, ptr(table),
                                                                   0.17, stream_handle(gpu_device)), gpu_device)
    call(ptr(qkv), ptr(out), 3 * E, E)
    torch.cuda.synchronize()
    assert _last_launch() == "window_attention_tr_kernel"
    before = _last_launch()
    for args in ((ptr(qkv), ptr(out), 3 * E + 4, E),        # qkv pitch not a multiple of 8
                 (ptr(qkv), ptr(out), 3 * E, E + 4),        # out pitch not a multiple of 8
                 (ptr(qkv) + 2, ptr(out), 3 * E, E),        # qkv off 16 bytes
                 (ptr(qkv), ptr(out) + 8, 3 * E, E)):       # out off 16 bytes
        with pytest.raises(ValueError):
            call(*args)
        assert _last_launch() == before, f"{args}: a launch was recorded"
