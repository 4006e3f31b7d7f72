"""The twelve kernels of csrc/glue.hip against the references of tests/_glueref.py, through the C ABI.

Every case asserts through elvis_last_launch the kernel it reached.  Every output is a view into a larger allocation:
16 sentinel bytes before it (the view itself starts on a 16-byte boundary), 64 after the last logical byte and, for
float outputs, one more row of them.  The exact ops run twice, on an output pre-filled with 0xA5 and with 0x5A: both
must equal the reference, so a byte the kernel does not write cannot pass, and the sentinels must survive.  The
accumulate kernel reads what it writes: its two runs start from two random float32 images, and every element outside
the tile must keep its bits.  Per-block SSIM is compared with its float64 reference under the per-block bound derived
in _glueref.ssim_ref, on an output that starts as NaN.  Nothing here places an input so that a wrong kernel would read
or write outside an allocation it was given: the inputs are exactly as large as the contract says."""
import time

import numpy as np
import pytest
import torch

import _glueref as R
from test_gpu_model_kernels_matrix import _last_launch

pytestmark = pytest.mark.gpu

LEAD, GUARD, SENT = 16, 64, 0xC3
FILLS = (0xA5, 0x5A)


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)          # a copy: the shared inputs are read-only


class Out:
    """`nbytes` logical bytes inside LEAD + nbytes + GUARD + extra allocated ones; .view(dtype) is the logical part."""

    def __init__(self, nbytes, fill, dev, extra=0):
        self.nbytes = nbytes
        self.raw = torch.full((LEAD + nbytes + GUARD + extra,), SENT, dtype=torch.uint8, device=dev)
        self.raw[LEAD:LEAD + nbytes] = fill
        assert (self.raw.data_ptr() + LEAD) % 16 == 0

    def view(self, dtype=torch.uint8):
        return self.raw[LEAD:LEAD + self.nbytes].view(dtype)

    @property
    def ptr(self):
        return self.raw.data_ptr() + LEAD

    def load(self, array):
        self.view(torch.uint8).copy_(torch.from_numpy(np.ascontiguousarray(array)).view(torch.uint8).reshape(-1).to(self.raw.device))

    def numpy(self, dtype, shape, cid):
        raw = self.raw.cpu().numpy()
        assert (raw[:LEAD] == SENT).all(), f"{cid}: written before the start of an output"
        assert (raw[LEAD + self.nbytes:] == SENT).all(), f"{cid}: written past the end of an output"
        return raw[LEAD:LEAD + self.nbytes].view(dtype).reshape(shape)


def _same(got, ref, cid, what="out"):
    at = R.first_difference(got, ref)
    assert at is None, f"{cid}: {what} differs first at {at}: got {got[at]!r}, reference {ref[at]!r}"


def _call(fn, *args):
    from elvis_amd._lib import check
    check(fn(*args))
    name = _last_launch()
    torch.cuda.synchronize()
    return name


# ------------------------------------------------------------------------------------------------------- runners
def _run_recompose(c, dev, s):
    from elvis_amd._lib import lib, ptr
    a, b, m = R.inputs(c)
    ref = R.expected(c)
    n, h, w, ch = c.shape
    by, bx = m.shape[1:]
    ad, bd, md = _dev(a, dev), _dev(b, dev), _dev(m, dev)
    assert ad.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0
    for fill in FILLS:
        out = Out(a.size, fill, dev)
        mo = Out(m.size * 4, fill, dev) if c.clamp_to is not None else None
        name = _call(lib().elvis_recompose_u8, ptr(ad), ptr(bd), ptr(md), out.ptr, mo.ptr if mo else None, n, h, w, ch,
                     c.block, by, bx, c.thr, c.clamp_to or 0, s)
        assert name == c.expect, f"{c.id}: launched {name!r}, the case exists for {c.expect!r}"
        _same(out.numpy(np.uint8, c.shape, c.id), ref[0], c.id)
        if mo:
            _same(mo.numpy(np.int32, m.shape, c.id), ref[1], c.id, "map_out")


def _run_area(c, dev, s):
    from elvis_amd._lib import lib
    x, = R.inputs(c)
    ref, = R.expected(c)
    n, h, w, ch = c.shape
    src = torch.empty(x.size + 16, dtype=torch.uint8, device=dev)
    assert src.data_ptr() % 16 == 0
    view = src[c.offset:c.offset + x.size]
    view.copy_(_dev(x.reshape(-1), dev))
    for fill in FILLS:
        out = Out(ref.size, fill, dev)
        name = _call(lib().elvis_area_downscale_u8, view.data_ptr(), out.ptr, n, h, w, ch, c.factor, c.rounding, s)
        assert name == c.expect, f"{c.id}: launched {name!r}, the case exists for {c.expect!r}"
        _same(out.numpy(np.uint8, ref.shape, c.id), ref, c.id)


def _run_blend(c, dev, s):
    from elvis_amd._lib import lib, ptr
    o, r, m = R.inputs(c)
    ref, = R.expected(c)
    n, h, w, ch = c.shape
    od, rd, md = _dev(o, dev), _dev(r, dev), _dev(m, dev)
    for fill in FILLS:
        out = Out(o.size, fill, dev)
        name = _call(lib().elvis_blend_u8, ptr(od), ptr(rd), ptr(md), out.ptr, n, h, w, ch, c.block, m.shape[1], m.shape[2],
                     c.alpha, s)
        assert name == c.expect
        _same(out.numpy(np.uint8, c.shape, c.id), ref, c.id)


def _run_select(c, dev, s):
    from elvis_amd._lib import lib, ptr
    *vs, m = R.inputs(c)
    ref, = R.expected(c)
    n, h, w, ch = c.shape
    keep, ptrs = [], []
    for i, v in enumerate(vs):
        off = c.offset if i == 1 else 0
        t = torch.empty(v.size + 16, dtype=torch.uint8, device=dev)
        t[off:off + v.size].copy_(_dev(v.reshape(-1), dev))
        keep.append(t)
        ptrs.append(t.data_ptr() + off)
    table = torch.tensor(ptrs, dtype=torch.int64, device=dev)
    slots, md = _dev(np.asarray(c.slots, np.int32), dev), _dev(m, dev)
    for fill in FILLS:
        out = Out(ref.size, fill, dev)
        name = _call(lib().elvis_select_levels_u8, ptr(table), ptr(slots), len(c.slots), ptr(md), out.ptr, n, h, w, ch,
                     c.block, m.shape[1], m.shape[2], s)
        assert name == c.expect
        _same(out.numpy(np.uint8, c.shape, c.id), ref, c.id)


def _run_accumulate(c, dev, s):
    from elvis_amd._lib import lib, ptr
    x = R.inputs(c)
    _, h, w, ch = c.shape
    dx = [_dev(a, dev) for a in x]
    for seed in (1, 2):
        rng = np.random.default_rng(c.seed * 10 + seed)
        acc0 = (rng.standard_normal((h, w, ch)) * 100.0).astype(np.float32)
        wsum0 = (rng.random((h, w)) * 4.0 - 0.5).astype(np.float32)
        acc, wsum = Out(acc0.nbytes, 0, dev, extra=w * ch * 4), Out(wsum0.nbytes, 0, dev, extra=w * 4)
        acc.load(acc0)
        wsum.load(wsum0)
        for i, (y0, x0, th, tw, tweight) in enumerate(c.tiles):
            tile, wy, wx, wx2 = dx[4 * i:4 * i + 4]
            name = _call(lib().elvis_tile_accumulate_f32, acc.ptr, wsum.ptr, ptr(tile), ptr(wy), ptr(wx), ptr(wx2), h, w, y0, x0,
                         th, tw, ch, tweight, s)
            assert name == c.expect
        racc, rwsum = R.accumulate_expected(c, acc0, wsum0)
        _same(acc.numpy(np.float32, acc0.shape, c.id), racc, c.id, "acc")
        _same(wsum.numpy(np.float32, wsum0.shape, c.id), rwsum, c.id, "wsum")


def _run_normalize(c, dev, s):
    from elvis_amd._lib import lib, ptr
    acc, wsum = R.inputs(c)
    ref, = R.expected(c)
    h, w, ch = acc.shape
    ad, wd = _dev(acc, dev), _dev(wsum, dev)
    for fill in FILLS:
        out = Out(ref.size, fill, dev)
        name = _call(lib().elvis_tile_normalize_u8, ptr(ad), ptr(wd), out.ptr, h, w, ch, s)
        assert name == c.expect
        _same(out.numpy(np.uint8, ref.shape, c.id), ref, c.id)


def _run_sse(c, dev, s):
    """include/elvis_amd.h: "both must be zeroed by the caller" - the entry point ADDS to what sse_out / cnt_out hold
    (one atomic add per wave).  Asserted: from zero the outputs are the sums; from other values they are those plus
    the sums."""
    from elvis_amd._lib import lib, ptr
    a, b, mk = R.inputs(c)
    rs, rc = R.expected(c)
    n, h, w, ch = c.shape
    ad, bd, md = _dev(a, dev), _dev(b, dev), _dev(mk, dev)
    for init_s, init_c in ((np.zeros(n, np.int64), np.zeros(n, np.int64)),
                           (np.arange(n, dtype=np.int64) * 1000 + 12345, np.full(n, 2 ** 33 + 7, np.int64))):
        so, co = Out(8 * n, 0, dev), Out(8 * n, 0, dev)
        so.load(init_s)
        co.load(init_c)
        name = _call(lib().elvis_sse_u8, ptr(ad), ptr(bd), ptr(md), so.ptr, co.ptr, n, h, w, ch, s)
        assert name == c.expect
        _same(so.numpy(np.int64, (n,), c.id), init_s + rs, c.id, "sse")
        _same(co.numpy(np.int64, (n,), c.id), init_c + rc, c.id, "count")


def _run_ssim(c, dev, s):
    from elvis_amd._lib import lib, ptr
    a, b = R.inputs(c)
    ref, bound = R.ssim_ref(a, b, c.block)
    n, h, w, ch = c.shape
    ad, bd, wd = _dev(a, dev), _dev(b, dev), _dev(R.ssim_window(), dev)
    out = Out(ref.size * 4, 0xFF, dev, extra=ref.shape[2] * 4)           # 0xFFFFFFFF: a NaN
    name = _call(lib().elvis_block_ssim_u8, ptr(ad), ptr(bd), out.ptr, ptr(wd), n, h, w, ch, c.block, s)
    assert name == c.expect
    y = out.numpy(np.float32, ref.shape, c.id).astype(np.float64)
    ratio = np.abs(y - ref) / bound
    worst = float(np.nanmax(ratio)) if not np.isnan(ratio).all() else float("nan")
    print(f"{c.id}: worst |y - ref| / bound {worst:.4f} (|y - ref| {float(np.nanmax(np.abs(y - ref))):.3g}, bound {float(bound.max()):.3g})")
    bad = np.argwhere(~(ratio <= 1.0))
    assert bad.size == 0, (f"{c.id}: block (n, by, bx) = {tuple(int(i) for i in bad[0])}: y {y[tuple(bad[0])]!r}, reference "
                           f"{ref[tuple(bad[0])]!r}, bound {bound[tuple(bad[0])]:.3g}")
    if c.kind == "black":
        assert (y == 1.0).all(), f"{c.id}: two black blocks must give exactly 1.0f"


RUN = {"recompose": _run_recompose, "area": _run_area, "blend": _run_blend, "select": _run_select,
       "accumulate": _run_accumulate, "normalize": _run_normalize, "sse": _run_sse, "ssim": _run_ssim}


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_glue_matrix(gpu_device, case):
    from elvis_amd._lib import stream_handle
    t0 = time.perf_counter()
    with torch.cuda.device(gpu_device):
        RUN[case.op](case, gpu_device, stream_handle(gpu_device))
    print(f"{case.id}: {time.perf_counter() - t0:.2f} s")


def test_area_c3_f4_is_the_same_from_every_byte_offset(gpu_device):
    """The c3 / f4 kernel (aligned source) and the generic kernel (the same image 1, 2 and 3 bytes further) agree."""
    from elvis_amd._lib import lib, stream_handle
    s = stream_handle(gpu_device)
    x = R.every_sum_image(4, 3, 4)
    n, h, w, ch = x.shape
    for rounding in (R.ROUND_CV2, R.ROUND_HALF_UP):
        outs, names = [], []
        for off in (0, 1, 2, 3):
            src = torch.empty(x.size + 16, dtype=torch.uint8, device=gpu_device)
            src[off:off + x.size].copy_(_dev(x.reshape(-1), gpu_device))
            out = Out(x.size // 16, 0xA5, gpu_device)
            names.append(_call(lib().elvis_area_downscale_u8, src.data_ptr() + off, out.ptr, n, h, w, ch, 4, rounding, s))
            outs.append(out.numpy(np.uint8, (n, h // 4, w // 4, ch), f"offset {off}"))
        assert names == ["area_downscale4_c3_kernel"] + ["area_downscale_u8_kernel"] * 3
        for off in (1, 2, 3):
            _same(outs[off], outs[0], f"rounding {rounding}, offset {off} against offset 0")


def test_glue_entry_points_reject_bad_arguments(gpu_device):
    """Each of these is the invalid-argument code (a ValueError through check) and launches nothing."""
    from elvis_amd._lib import lib, check, ptr, stream_handle
    dev = gpu_device
    s = stream_handle(dev)
    n, h, w, c, blk = 1, 16, 32, 3, 8
    tot = n * h * w * c
    a = torch.zeros(tot + 64, dtype=torch.uint8, device=dev)
    b = torch.zeros(tot + 64, dtype=torch.uint8, device=dev)
    o = torch.zeros(tot + 64, dtype=torch.uint8, device=dev)
    m = torch.zeros(n, h // blk, w // blk, dtype=torch.int32, device=dev)
    check(lib().elvis_recompose_u8(ptr(a), ptr(b), ptr(m), ptr(o), None, n, h, w, c, blk, 2, 4, 0, 0, s))       # accepted
    check(lib().elvis_blend_u8(ptr(a), ptr(b), ptr(m), ptr(o), n, h, w, c, blk, 2, 4, 0.5, s))
    torch.cuda.synchronize()
    marker = _last_launch()
    assert marker == "blend_u8_kernel"

    def refused(rc, what):
        assert rc == -1, f"{what}: returned {rc}"
        with pytest.raises(ValueError):
            check(rc)
        assert _last_launch() == marker, f"{what}: a launch was recorded"

    for da, db, do in ((4, 0, 0), (0, 8, 0), (0, 0, 1), (0, 0, 8)):
        refused(lib().elvis_recompose_u8(ptr(a) + da, ptr(b) + db, ptr(m), ptr(o) + do, None, n, h, w, c, blk, 2, 4, 0, 0, s),
                f"recompose, pointers off by {da}, {db}, {do}")
        refused(lib().elvis_blend_u8(ptr(a) + da, ptr(b) + db, ptr(m), ptr(o) + do, n, h, w, c, blk, 2, 4, 0.5, s),
                f"blend, pointers off by {da}, {db}, {do}")
    refused(lib().elvis_blend_u8(ptr(a), ptr(b), ptr(m), ptr(o), n, h, w, c, blk, 1, 4, 0.5, s), "blend, by != h / block")
    refused(lib().elvis_blend_u8(ptr(a), ptr(b), ptr(m), ptr(o), n, h, w, c, blk, 2, 3, 0.5, s), "blend, bx != w / block")
    acc = torch.zeros(h, w, c, device=dev)
    ws = torch.zeros(h, w, device=dev)
    tile = torch.zeros(8, 8, c, dtype=torch.uint8, device=dev)
    wy = torch.ones(8, device=dev)
    wx = torch.ones(8, dtype=torch.float64, device=dev)
    for y0, x0 in ((h - 7, 0), (0, w - 7), (-1, 0), (0, -1)):
        refused(lib().elvis_tile_accumulate_f32(ptr(acc), ptr(ws), ptr(tile), ptr(wy), ptr(wx), ptr(wx), h, w, y0, x0, 8, 8, c,
                                                1.0, s), f"tile at ({y0}, {x0}) outside the frame")
    for f in (3, 5):
        refused(lib().elvis_area_downscale_u8(ptr(a), ptr(o), n, h, w, c, f, 0, s), f"area factor {f} of {h} x {w}")
    for code in (2, -1):
        refused(lib().elvis_area_downscale_u8(ptr(a), ptr(o), n, h, w, c, 4, code, s), f"rounding code {code}")
    torch.cuda.synchronize()
    assert not bool(o.any()) and not bool(acc.any())
