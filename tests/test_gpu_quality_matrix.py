"""The edge matrix of csrc/quality.hip on the device (cases and float64 references: tests/_qualitycases.py; what the
cases reach: tests/test_quality_inpaint_ledger.py).  SSIM: abs <= 1e-9, the bar derived in tests/test_gpu_quality.py, and
exactly 1.0 where the reference says 1.0; boxes and masked frames: equality.  Every case asserts the kernel that ran,
that the inputs and the guard bytes around them are untouched, and - for SSIM - that identical inputs give exactly 1.0
and that a frame's value does not depend on the batch it rides in."""
import numpy as np
import pytest
import torch

import _qualitycases as K

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xC3


def _place(arr, off, dev):
    """`arr` as a contiguous view `off` bytes past a 16-byte boundary of a sentinel-filled allocation."""
    buf = torch.full((2 * GUARD + 64 + arr.size,), FILL, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0 and 0 <= off < 64
    view = buf[GUARD + off:GUARD + off + arr.size].view(arr.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)).to(dev))
    assert view.is_contiguous() and view.data_ptr() % 16 == off % 16
    return buf, view


def _intact(buf, off, arr):
    h = buf.cpu().numpy()
    lo, hi = GUARD + off, GUARD + off + arr.size
    return bool((h[:lo] == FILL).all() and (h[hi:] == FILL).all() and np.array_equal(h[lo:hi].reshape(arr.shape), arr))


def _launch():
    from elvis_amd import _lib
    return _lib.lib().elvis_last_launch().decode()


@pytest.mark.parametrize("case", K.of("ssim"), ids=lambda c: c.id)
def test_ssim(gpu_device, case):
    from elvis_amd import _lib, metrics
    a, b, m = K.inputs(case)
    want = K.expected(case)
    n = case.shape[0]
    (ba, va), (bb, vb) = _place(a, case.offs[0], gpu_device), _place(b, case.offs[1], gpu_device)
    bm, vm = _place(m, case.offs[2], gpu_device) if m is not None else (None, None)
    rects = None if case.rects is None else torch.tensor(case.rects, dtype=torch.int32, device=gpu_device)
    C1, C2 = case.constants

    def run(x, y, masks, rc):
        return metrics.ssim_mean_device(x, y, K.window(case.window), source=_lib.SSIM_LUMA if case.source == "luma" else _lib.SSIM_CHANNELS,
                                        border=_lib.SSIM_REFLECT if case.border == "reflect" else _lib.SSIM_VALID, C1=C1, C2=C2,
                                        cov_norm=1.0, pad=_lib.SSIM_PAD_AUTO if case.pad is None else case.pad, scale=case.scale,
                                        masks=masks, rects=rc).cpu().numpy()
    got = run(va, vb, vm, rects)
    assert _launch() == case.kernel
    assert got.shape == want.shape and got.dtype == np.float64
    print(f"{case.id}: max |device - reference| = {np.abs(got - want).max():.3e}  device {got.ravel()[:4]} reference {want.ravel()[:4]}")
    assert (np.abs(got - want) <= K.BAR).all()
    assert (got[want == 1.0] == 1.0).all(), "exactly 1.0 where the reference says 1.0"
    assert (run(va, va, vm, rects) == 1.0).all(), "identical inputs"
    if n > 1:                                   # a frame alone: another address, often another staging path, the same bits
        for f in range(n):
            alone = run(va[f:f + 1], vb[f:f + 1], None if vm is None else vm[f:f + 1], None if rects is None else rects[f:f + 1].contiguous())
            assert np.array_equal(alone[0], got[f]), f"frame {f} alone"
    assert np.array_equal(run(va, vb, vm, rects), got), "deterministic"
    assert _intact(ba, case.offs[0], a) and _intact(bb, case.offs[1], b) and (bm is None or _intact(bm, case.offs[2], m))
    if rects is not None:
        assert np.array_equal(rects.cpu().numpy(), np.array(case.rects, np.int32))


@pytest.mark.parametrize("case", K.of("bbox"), ids=lambda c: c.id)
def test_bbox(gpu_device, case):
    from elvis_amd import metrics
    m, = K.inputs(case)
    bm, vm = _place(m, case.offs[0], gpu_device)
    assert vm.data_ptr() % 8 == case.offs[0] % 8
    got = metrics.mask_bbox_device(vm).cpu().numpy()
    assert _launch() == case.kernel
    want = K.expected(case)
    assert got.dtype == np.int32 and np.array_equal(got, want), f"{case.id}: device {got.tolist()} reference {want.tolist()}"
    assert _intact(bm, case.offs[0], m)


@pytest.mark.parametrize("case", K.of("apply"), ids=lambda c: c.id)
def test_apply(gpu_device, case):
    from elvis_amd import _lib
    from elvis_amd.ops import _s
    frames, m = K.inputs(case)
    n, h, w, c = case.shape
    (bf, vf), (bm, vm) = _place(frames, case.offs[0], gpu_device), _place(m, case.offs[1], gpu_device)
    garbage = np.full(frames.shape, 0x5A, np.uint8)
    bo, vo = _place(garbage, case.offs[2], gpu_device)
    _lib.check(_lib.lib().elvis_apply_mask_u8(_lib.ptr(vf), _lib.ptr(vm), _lib.ptr(vo), n, h, w, c, int(case.invert), _s(vf)), gpu_device)
    assert _launch() == case.kernel
    want = K.expected(case)
    assert _intact(bo, case.offs[2], want), f"{case.id}: the output or its guard bytes differ"
    assert _intact(bf, case.offs[0], frames) and _intact(bm, case.offs[1], m)
