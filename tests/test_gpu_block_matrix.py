"""The ten kernels of csrc/classical.hip, csrc/degrade.hip and csrc/shrink.hip against the cases of tests/_blockref.py.

The classical and degrade kernels run through their public `*_device` functions with `out=` a view into a larger
allocation; the four shrink kernels run through the C ABI, the only way to hand them a NULL src_of / removal_idx, a
misaligned base or an output this test owns.  Every output is pre-filled with a sentinel byte (twice, with two
different bytes) and framed by guard bytes that must survive, so an element a kernel skips cannot pass and a write
outside the output is seen.  Every comparison is exact (dtype, shape and contents); inputs must be unchanged
afterwards.  Nothing here places an input so that a wrong kernel would read or write outside an allocation."""
import time

import numpy as np
import pytest
import torch

import _blockref as R
from test_gpu_glue_matrix import FILLS, Out, _dev, _same
from test_gpu_model_kernels_matrix import _last_launch

pytestmark = pytest.mark.gpu

MODES = {"rows": 0, "rows_cols": 1}
RANKS = {"flat": 0, "rows": 1}


def _unchanged(dev_tensor, host, cid):
    assert np.array_equal(dev_tensor.cpu().numpy().reshape(host.shape), host), f"{cid}: an input was modified"


def _check(rc, dev):
    from elvis_amd._lib import check
    check(rc, dev)
    torch.cuda.synchronize()


def _shifted(a, off, dev):
    """A device copy of `a` whose first byte sits `off` bytes past a 16-byte boundary (and the tensor that owns it)."""
    raw = torch.zeros(a.nbytes + 32, dtype=torch.uint8, device=dev)
    assert raw.data_ptr() % 16 == 0
    view = raw[off:off + a.nbytes]
    if a.nbytes:
        view.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev))
    return raw, view


class OutAt(Out):
    """An Out whose logical part starts `off` bytes past the 16-byte boundary."""

    def __init__(self, nbytes, fill, dev, off):
        super().__init__(nbytes + off, fill, dev)
        self.off = off
        self.raw[16:16 + off] = 0xC3
        self.nbytes = nbytes + off

    @property
    def ptr(self):
        return self.raw.data_ptr() + 16 + self.off

    def numpy(self, dtype, shape, cid):
        raw = super().numpy(np.uint8, (self.nbytes,), cid)
        assert (raw[:self.off] == 0xC3).all(), f"{cid}: written before the start of an output"
        return raw[self.off:].view(dtype).reshape(shape)


# ------------------------------------------------------------------------------------------------------- shrink
def _run_topk(c, dev, s):
    from elvis_amd._lib import lib, ptr
    scores, = R.inputs(c)
    mask_ref, src_ref = R.expected(c)
    n, by, bx = c.grid
    sd = _dev(scores, dev)
    for fill in FILLS:
        mask, src_of = Out(mask_ref.size, fill, dev), Out(src_ref.size * 4, fill, dev)
        _check(lib().elvis_shrink_select_topk(ptr(sd), mask.ptr, src_of.ptr if c.k < bx else None, n, by, bx, c.k, s), dev)
        _same(mask.numpy(np.int8, mask_ref.shape, c.id), mask_ref, c.id, "mask")
        _same(src_of.numpy(np.int32, src_ref.shape, c.id), src_ref, c.id, "src_of")
    _unchanged(sd, scores, c.id)


def _run_passes(c, dev, s):
    import ctypes as C
    from elvis_amd._lib import lib, ptr
    scores, = R.inputs(c)
    mask_ref, src_ref, ridx_ref = R.expected(c)
    n, by, bx = c.grid
    sby, sbx = src_ref.shape[1:]
    counts = R.passes_counts(c)
    got_by, got_bx, got_counts = C.c_int(0), C.c_int(0), (C.c_int * (by + bx + 2))()
    np_ = lib().elvis_shrink_passes_plan(by, bx, c.target, MODES[c.mode], C.addressof(got_by), C.addressof(got_bx),
                                         C.addressof(got_counts), by + bx + 2)
    assert (got_by.value, got_bx.value, list(got_counts[:np_])) == (sby, sbx, counts), f"{c.id}: the plan"
    made = sum(counts)
    assert ridx_ref.shape == (n, made)
    sd = _dev(scores, dev)
    for fill in FILLS:
        mask, src_of = Out(n * by * bx, fill, dev), Out(src_ref.size * 4, fill, dev)
        ridx = Out(n * c.target * 4, fill, dev) if c.ridx else None
        ws_s, ws_p = Out(n * by * bx * 8, fill, dev), Out(n * by * bx * 4, fill, dev)
        _check(lib().elvis_shrink_select_passes(ptr(sd), mask.ptr, src_of.ptr if sby * sbx else None, ridx.ptr if ridx else None,
                                                ws_s.ptr, ws_p.ptr, n, by, bx, c.target, MODES[c.mode], sby, sbx, s), dev)
        _same(mask.numpy(np.uint8, mask_ref.shape, c.id), mask_ref, c.id, "mask")
        _same(src_of.numpy(np.int32, src_ref.shape, c.id), src_ref, c.id, "src_of")
        ws_s.numpy(np.float64, (n, by, bx), c.id)
        ws_p.numpy(np.int32, (n, by, bx), c.id)
        if ridx:
            got = ridx.numpy(np.int32, (n, c.target), c.id)
            _same(np.ascontiguousarray(got[:, :made]), ridx_ref, c.id, "removal_idx")
            word = np.frombuffer(bytes([fill] * 4), np.int32)[0]
            assert (got[:, made:] == word).all(), f"{c.id}: removal_idx written beyond the removals made"
    _unchanged(sd, scores, c.id)


def _run_stretch(c, dev, s):
    from elvis_amd._lib import lib, ptr
    m, = R.inputs(c)
    ref, = R.expected(c)
    n, by, bx = c.grid
    md = _dev(m, dev)
    for fill in FILLS:
        out = Out(ref.size * 4, fill, dev)
        _check(lib().elvis_stretch_index(ptr(md), out.ptr, n, by, bx, c.sgrid[0], c.sgrid[1], RANKS[c.mode], s), dev)
        _same(out.numpy(np.int32, ref.shape, c.id), ref, c.id, "src_of")
    _unchanged(md, m, c.id)


def _run_gather(c, dev, s):
    from elvis_amd._lib import lib, ptr
    frames, src_of = R.inputs(c)
    dst_ref, mask_ref = R.expected(c)
    n, hs, ws, ch = c.shape
    keep, fview = _shifted(frames, c.offs[0], dev)
    sd = _dev(src_of, dev)
    for fill in FILLS[:1] if c.big else FILLS:
        dst, mask = OutAt(dst_ref.size, fill, dev, c.offs[1]), OutAt(mask_ref.size, fill, dev, c.offs[2])
        _check(lib().elvis_block_gather_u8(fview.data_ptr() if frames.size else None, ptr(sd), dst.ptr, mask.ptr, n, hs, ws, ch,
                                           c.block, c.sgrid[0], c.sgrid[1], c.dgrid[0], c.dgrid[1], s), dev)
        name = _last_launch()
        assert name == c.launch, f"{c.id}: launched {name!r}, the case exists for {c.launch!r}"
        _same(dst.numpy(np.uint8, dst_ref.shape, c.id), dst_ref, c.id, "dst")
        _same(mask.numpy(np.uint8, mask_ref.shape, c.id), mask_ref, c.id, "mask")
    _unchanged(fview, frames, c.id)
    _unchanged(sd, src_of, c.id)


# ------------------------------------------------------------------------------------------------------- classical, degrade
def _run_blocks(c, dev, s):
    from elvis_amd import classical, degrade
    frames, m = R.inputs(c)
    ref, = R.expected(c)
    fd, md = _dev(frames, dev), _dev(m, dev)
    call = {"lanczos": lambda o: classical.lanczos_restore_device(fd, md, c.block, out=o),
            "unsharp": lambda o: classical.unsharp_restore_device(fd, md, c.block, c.halo, out=o),
            "downsample": lambda o: degrade.degrade_downsample_device(fd, md, c.block, out=o),
            "gaussian": lambda o: degrade.degrade_gaussian_device(fd, md, c.block, out=o),
            "dct": lambda o: degrade.degrade_dct_device(fd, md, out=o)}[c.op]
    n, h, w, ch = c.shape
    inside = np.zeros((h, w), bool)
    inside[:h // c.block * c.block, :w // c.block * c.block] = True
    for fill in FILLS:
        out = Out(frames.size, fill, dev)
        view = out.view().reshape(c.shape)
        assert call(view) is view
        torch.cuda.synchronize()
        got = out.numpy(np.uint8, c.shape, c.id)
        # include/elvis_amd.h: the classical kernels write the whole blocks only - the caller's bytes stay outside them
        want = np.where(inside[None, :, :, None], ref, np.uint8(fill))
        _same(got, want, c.id)
    if not inside.all():            # without `out` the wrapper starts from a copy: the pixels outside the grid are the source's
        got = call(None).cpu().numpy()
        _same(got, ref, c.id, "out (allocated by the wrapper)")
    _unchanged(fd, frames, c.id)
    _unchanged(md, m, c.id)


def _run_blend(c, dev, s):
    from elvis_amd import classical
    frames, = R.inputs(c)
    ref, = R.expected(c)
    fd = _dev(frames, dev)
    if c.alias:
        out = Out(frames.size, 0, dev)
        out.load(frames)
        view = out.view().reshape(c.shape)
        assert classical.temporal_blend_device(view, c.tb, out=view) is view
        torch.cuda.synchronize()
        _same(out.numpy(np.uint8, c.shape, c.id), ref, c.id)
        return
    for fill in FILLS:
        out = Out(frames.size, fill, dev)
        view = out.view().reshape(c.shape)
        assert classical.temporal_blend_device(fd, c.tb, out=view) is view
        torch.cuda.synchronize()
        _same(out.numpy(np.uint8, c.shape, c.id), ref, c.id)
    _unchanged(fd, frames, c.id)


RUN = {"topk": _run_topk, "passes": _run_passes, "stretch": _run_stretch, "gather": _run_gather, "blend": _run_blend,
       "lanczos": _run_blocks, "unsharp": _run_blocks, "downsample": _run_blocks, "gaussian": _run_blocks, "dct": _run_blocks}


def _matrix(op):
    cases = [c for c in R.CASES if c.op == op]
    return pytest.mark.parametrize("case", cases, ids=[c.id for c in cases])


def _go(case, gpu_device):
    from elvis_amd._lib import stream_handle
    t0 = time.perf_counter()
    with torch.cuda.device(gpu_device):
        RUN[case.op](case, gpu_device, stream_handle(gpu_device))
    print(f"{case.id}: {time.perf_counter() - t0:.2f} s")


@_matrix("topk")
def test_shrink_select_topk(gpu_device, case):
    _go(case, gpu_device)


@_matrix("passes")
def test_shrink_select_passes(gpu_device, case):
    _go(case, gpu_device)


@_matrix("stretch")
def test_stretch_index(gpu_device, case):
    _go(case, gpu_device)


@_matrix("gather")
def test_block_gather(gpu_device, case):
    _go(case, gpu_device)


@_matrix("lanczos")
def test_classical_lanczos(gpu_device, case):
    _go(case, gpu_device)


@_matrix("unsharp")
def test_classical_unsharp(gpu_device, case):
    _go(case, gpu_device)


@_matrix("blend")
def test_temporal_blend(gpu_device, case):
    _go(case, gpu_device)


@_matrix("downsample")
def test_degrade_downsample(gpu_device, case):
    _go(case, gpu_device)


@_matrix("gaussian")
def test_degrade_gaussian(gpu_device, case):
    _go(case, gpu_device)


@_matrix("dct")
def test_degrade_dct(gpu_device, case):
    _go(case, gpu_device)


def test_degrade_out_must_match_the_frames(gpu_device):
    """`out=` goes to the kernel as a bare pointer: anything but a contiguous uint8 tensor of the frames' shape on the
    frames' device is a ValueError, and nothing is launched."""
    from elvis_amd import degrade
    dev = gpu_device
    f = torch.zeros((2, 16, 24, 3), dtype=torch.uint8, device=dev)
    m = torch.ones((2, 2, 3), dtype=torch.int32, device=dev)
    calls = (lambda o: degrade.degrade_downsample_device(f, m, 8, out=o), lambda o: degrade.degrade_gaussian_device(f, m, 8, out=o),
             lambda o: degrade.degrade_dct_device(f, m, out=o))
    bad = {"shape": torch.zeros((2, 16, 24, 4), dtype=torch.uint8, device=dev),
           "smaller": torch.zeros((1, 16, 24, 3), dtype=torch.uint8, device=dev),
           "dtype": torch.zeros((2, 16, 24, 3), dtype=torch.int8, device=dev),
           "strided": torch.zeros((2, 16, 24, 6), dtype=torch.uint8, device=dev)[..., ::2],
           "host": torch.zeros((2, 16, 24, 3), dtype=torch.uint8)}
    for call in calls:
        for what, o in bad.items():
            with pytest.raises(ValueError):
                call(o)
        good = torch.full_like(f, 7)
        assert call(good) is good
    # the classical device forms take the same check: a host `out` is refused, not handed to the kernel
    from elvis_amd import classical
    f1 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=dev)
    m1 = torch.ones((1, 2, 2), dtype=torch.int32, device=dev)
    for fn in (classical.lanczos_restore_device, classical.unsharp_restore_device):
        with pytest.raises(ValueError):
            fn(f1, m1, 4, out=torch.zeros((1, 8, 8, 3), dtype=torch.uint8))
    torch.cuda.synchronize()
