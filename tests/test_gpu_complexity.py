"""Block complexity on the device (csrc/complexity.hip, elvis_amd/complexity.py) against the numpy float64 statement of
its contract (tests/_complexity_ref.py): |device - reference| <= 1e-9 * max(1, |reference|) over the matrix of block
sizes, frame sizes, grids, frame counts and colour layouts; `prev`; chunking; exact zeros; memory discipline; determinism;
the removability driver; the argument errors.  Shapes are the smallest that reach each branch (at most 3 x 17 blocks)."""
import numpy as np
import pytest
import torch

import _complexity_ref as R
import elvis_amd
from elvis_amd import _lib, complexity

pytestmark = pytest.mark.gpu

GUARD = 16                     # float64 sentinels on either side of each output
SENTINEL = -777.25
KERNELS = sorted({c.kernel for c in R.MATRIX})


def _shifted(host: np.ndarray, dev, shift: int):
    """`host` uploaded into a 0x5A-filled byte buffer, `shift` bytes past its (at least 256-byte aligned) start."""
    buf = torch.full((host.size + 2 * 64,), 0x5A, dtype=torch.uint8, device=dev)
    view = buf[64 + shift:64 + shift + host.size].view(host.shape)
    view.copy_(torch.from_numpy(host))
    assert view.is_contiguous() and view.data_ptr() % 4 == shift % 4
    return buf, view


def _guarded(shape, dev):
    buf = torch.full((int(np.prod(shape)) + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    return buf, buf[GUARD:GUARD + int(np.prod(shape))].view(shape)


def run(frames: np.ndarray, block: int, order: str = "rgb", prev=None, dev="cuda:0", shift: int = 0, prev_shift: int = 0, kernel=None):
    """One guarded launch: (SC, TC) as numpy.  Checks the sentinels round both outputs and round the inputs, that the
    inputs are unchanged and, when `kernel` is given, which instantiation ran."""
    fbuf, fd = _shifted(frames, dev, shift)
    pbuf, pd = _shifted(prev, dev, prev_shift) if prev is not None else (None, None)
    n, h, w, _ = frames.shape
    shape = (n, h // block, w // block)
    sbuf, sc = _guarded(shape, dev)
    tbuf, tc = _guarded(shape, dev)
    got = complexity.block_complexity_device(fd, block, order, prev=pd, out=(sc, tc))
    torch.cuda.synchronize()
    assert got[0] is sc and got[1] is tc
    if kernel is not None:
        assert _lib.lib().elvis_last_launch().decode() == kernel
    for buf in (sbuf, tbuf):
        host = buf.cpu().numpy()
        assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all(), "an output's guard was written"
    for buf, view, src, sh in ((fbuf, fd, frames, shift), (pbuf, pd, prev, prev_shift)):
        if buf is not None:
            host = buf.cpu().numpy()
            assert np.array_equal(view.cpu().numpy(), src), "an input was written"
            assert (host[:64 + sh] == 0x5A).all() and (host[64 + sh + src.size:] == 0x5A).all()
    return sc.cpu().numpy().copy(), tc.cpu().numpy().copy()


# ----------------------------------------------------------------------------- the matrix
@pytest.mark.parametrize("kernel", KERNELS)
def test_matrix_within_the_bar(gpu_device, kernel):
    cases = [c for c in R.MATRIX if c.kernel == kernel]
    assert len(cases) == 76
    worst, where = 0.0, None
    failed = []
    for i, case in enumerate(cases):
        frames, prev = R.inputs(case)
        want_sc, want_tc = R.expected(case.id)
        sc, tc = run(frames, case.block, case.order, prev, gpu_device, shift=i % 4, prev_shift=(i // 4) % 4, kernel=case.kernel)
        for name, got, want in (("SC", sc, want_sc), ("TC", tc, want_tc)):
            assert got.shape == want.shape == (case.shape[0],) + case.grid and np.isfinite(got).all(), case.id
            err = R.worst(got, want)
            if err > worst:
                worst, where = err, f"{case.id} {name}"
            if not R.within_bar(got, want):
                failed.append((case.id, name, err))
        if not case.prev:
            assert (tc[0] == 0.0).all(), case.id
    print(f"{kernel}: worst |device - reference| / max(1, |reference|) = {worst:.3g} at {where} (bar {R.BAR})")
    assert not failed, failed[:5]


@pytest.mark.parametrize("case_id", [c.id for c in R.NAMED])
def test_the_mutants_cases_within_the_bar(gpu_device, case_id):
    case = R.BY_ID[case_id]
    frames, prev = R.inputs(case)
    want = R.expected(case.id)
    got = run(frames, case.block, case.order, prev, gpu_device, kernel=case.kernel)
    print(f"{case_id}: SC {R.worst(got[0], want[0]):.3g}, TC {R.worst(got[1], want[1]):.3g} (bar {R.BAR})")
    assert R.within_bar(got[0], want[0]) and R.within_bar(got[1], want[1])


# ----------------------------------------------------------------------------- prev and chunking
@pytest.mark.parametrize("block,c,order", [(8, 1, "rgb"), (16, 3, "rgb"), (32, 3, "bgr")])
def test_prev(gpu_device, block, c, order):
    rng = np.random.default_rng(block + c)
    clip = rng.integers(0, 256, (4, 2 * block + 5, 5 * block + 3, c), dtype=np.uint8)
    # one frame, no predecessor: TC is zero everywhere
    sc1, tc1 = run(clip[:1], block, order, None, gpu_device)
    assert (tc1 == 0.0).all() and sc1.any()
    # prev given == analysing [prev] + frames and dropping frame 0, to the byte
    whole = run(clip, block, order, None, gpu_device)
    tail = run(clip[1:], block, order, clip[0], gpu_device)
    assert np.array_equal(tail[0], whole[0][1:]) and np.array_equal(tail[1], whole[1][1:])
    assert np.array_equal(sc1, whole[0][:1]) and whole[1][1:].all()
    want = R.complexity(clip[1:], block, order, clip[0])
    assert R.within_bar(tail[0], want[0]) and R.within_bar(tail[1], want[1])


def test_analyze_frames_does_not_depend_on_the_chunk_size(gpu_device):
    rng = np.random.default_rng(11)
    clip = rng.integers(0, 256, (5, 37, 53, 3), dtype=np.uint8)
    want = R.complexity(clip, 16, "rgb")
    runs = [complexity.analyze_frames(clip, complexity.EVCAConfig(block_size=16), gpu_device, chunk_frames=k) for k in (1, 2, None, 5)]
    for r in runs:
        assert r.SC.dtype == r.TC.dtype == np.float64 and r.SC.shape == r.TC.shape == (5, 2, 3)
        assert r.SC.tobytes() == runs[0].SC.tobytes() and r.TC.tobytes() == runs[0].TC.tobytes()
    assert R.within_bar(runs[0].SC, want[0]) and R.within_bar(runs[0].TC, want[1]) and (runs[0].TC[0] == 0.0).all()
    # Presley's call shape: a list of frames, the default config; grey frames without a channel axis; bgr
    as_list = elvis_amd.analyze_frames([f for f in clip])
    assert as_list.SC.tobytes() == runs[0].SC.tobytes() and as_list.TC.tobytes() == runs[0].TC.tobytes()
    grey = complexity.analyze_frames(clip[..., 0], complexity.EVCAConfig(block_size=8), gpu_device, chunk_frames=3)
    want = R.complexity(clip[..., :1], 8)
    assert R.within_bar(grey.SC, want[0]) and R.within_bar(grey.TC, want[1])
    bgr = complexity.analyze_frames(clip, complexity.EVCAConfig(block_size=32), gpu_device, order="bgr", chunk_frames=2)
    want = R.complexity(clip, 32, "bgr")
    assert R.within_bar(bgr.SC, want[0]) and R.within_bar(bgr.TC, want[1])


# ----------------------------------------------------------------------------- exact zeros
@pytest.mark.parametrize("block", R.BLOCKS)
def test_exact_zeros_on_the_device(gpu_device, block):
    rng = np.random.default_rng(block)
    for c, order in R.COLOURS:
        frames = rng.integers(0, 256, (3, 2 * block + 3, 3 * block + 1, c), dtype=np.uint8)
        frames[:, :block, block:2 * block] = np.asarray([[[[0]]], [[[16]]], [[[255]]]], np.uint8)     # flat blocks of 0, 16, 255
        frames[1, block:2 * block, :block] = frames[0, block:2 * block, :block]                       # frame 1 = frame 0 in one block
        frames[2, block:2 * block, 2 * block:3 * block] = frames[1, block:2 * block, 2 * block:3 * block]
        sc, tc = run(frames, block, order, None, gpu_device)
        assert (sc[:, 0, 1] == 0.0).all() and np.count_nonzero(sc) == sc.size - 3
        assert (tc[0] == 0.0).all() and tc[1, 1, 0] == 0.0 and tc[2, 1, 2] == 0.0 and (tc[:, 0, 1] == 0.0).all()
        assert np.count_nonzero(tc[1:]) == tc[1:].size - 4
        want = R.complexity(frames, block, order)
        assert np.array_equal(sc == 0.0, want[0] == 0.0) and np.array_equal(tc == 0.0, want[1] == 0.0)
        assert R.within_bar(sc, want[0]) and R.within_bar(tc, want[1])


# ----------------------------------------------------------------------------- memory discipline and determinism
@pytest.mark.parametrize("block,c,order", [(8, 3, "rgb"), (16, 1, "rgb"), (32, 3, "bgr"), (16, 3, "bgr")])
def test_memory_discipline_and_determinism(gpu_device, block, c, order):
    rng = np.random.default_rng(100 + block + c)
    # a width that is a multiple of 4 (rows can start on a dword) and one that is not
    for w in (5 * block + 4, 5 * block + 3):
        frames = rng.integers(0, 256, (2, 2 * block + 2, w, c), dtype=np.uint8)
        prev = rng.integers(0, 256, frames.shape[1:], dtype=np.uint8)
        base = run(frames, block, order, prev, gpu_device, 0, 0)
        want = R.complexity(frames, block, order, prev)
        assert R.within_bar(base[0], want[0]) and R.within_bar(base[1], want[1])
        for shift, prev_shift in ((1, 0), (2, 3), (3, 1), (0, 2), (0, 0)):       # views 1, 2, 3 bytes off a dword; again: determinism
            again = run(frames, block, order, prev, gpu_device, shift, prev_shift)
            assert again[0].tobytes() == base[0].tobytes() and again[1].tobytes() == base[1].tobytes(), (w, shift, prev_shift)
        # the remainder rows and columns take other values: no output changes
        by, bx = frames.shape[1] // block, w // block
        other, other_prev = frames.copy(), prev.copy()
        for a in (other, other_prev[None]):
            a[:, by * block:] ^= 0xFF
            a[:, :, bx * block:] ^= 0xFF
        moved = run(other, block, order, other_prev, gpu_device, 1, 2)
        assert moved[0].tobytes() == base[0].tobytes() and moved[1].tobytes() == base[1].tobytes(), w


# ----------------------------------------------------------------------------- the driver
def test_removability_driver(gpu_device):
    rng = np.random.default_rng(21)
    block, margin = 16, 1e-6
    clip = rng.integers(0, 256, (3, 48, 96, 3), dtype=np.uint8)
    clip[:, :16, :32] //= 4                                                    # quieter blocks: a spread of scores
    masks = [rng.choice(np.asarray([0, 255], np.uint8), size=(13, 9)), None, np.zeros((48, 96), np.uint8)]
    sc, tc = R.complexity(clip, block, "bgr")
    for alpha, beta in ((0.5, 1), (0.3, 0.5)):
        want = complexity.removability_from_complexity(sc, tc, masks, alpha, beta)
        rows = np.sort(want, axis=2)
        assert np.diff(rows, axis=2).min() > margin > 1e-9, "the reference's scores must be tie-free by a margin above the bar"
        got = elvis_amd.calculate_removability_scores_from_frames(clip, masks, block, alpha, beta, device=gpu_device)
        assert got.shape == want.shape == (3, 3, 6) and got.dtype == np.float64
        print(f"driver alpha={alpha} beta={beta}: worst |got - want| = {np.abs(got - want).max():.3g}")
        assert np.abs(got - want).max() <= 1e-9 and got.min() == 0.0 and got.max() == 1.0
        for f in range(3):
            shrunk, removed, cols = elvis_amd.apply_selective_removal(clip[f], got[f], block, 0.34, device=gpu_device)
            top2 = np.sort(np.argsort(-want[f], axis=1)[:, :2], axis=1)            # int(0.34 * 6) = 2 per row, tie-free
            assert shrunk.shape == (48, 64, 3) and removed.shape == (3, 6) and [sorted(r) for r in cols] == top2.tolist()


# ----------------------------------------------------------------------------- errors
def test_value_errors_come_before_any_launch(gpu_device):
    h = _lib.lib()
    f = torch.zeros((2, 16, 24, 3), dtype=torch.uint8, device=gpu_device)
    complexity.block_complexity_device(torch.zeros((1, 8, 8, 1), dtype=torch.uint8, device=gpu_device), 8)
    torch.cuda.synchronize()
    marker = h.elvis_last_launch()
    assert marker == b"block_complexity_kernel<8,1,0>"
    sbuf, sc = _guarded((2, 1, 1), gpu_device)
    tbuf, tc = _guarded((2, 1, 1), gpu_device)
    bad = [
        (f, dict(block_size=12), "block_size"),
        (f, dict(block_size=64), "block_size"),
        (f, dict(order="yuv"), "order"),
        (f, dict(block_size=32), "smaller than one block"),
        (f[:, :, :15], dict(), "contiguous"),
        (f[:, :, :15].contiguous(), dict(), "smaller than one block"),
        (f.to(torch.int32), dict(), "uint8"),
        (f.cpu(), dict(), "CUDA"),
        (f[0], dict(), "1 or 3 channels"),
        (torch.zeros((2, 16, 24, 2), dtype=torch.uint8, device=gpu_device), dict(), "1 or 3 channels"),
        (torch.zeros((2, 16, 24, 4), dtype=torch.uint8, device=gpu_device), dict(), "1 or 3 channels"),
        (f, dict(prev=f[0].cpu()), "prev must be"),
        (f, dict(prev=f[0, :, :, :1].contiguous()), "prev must be"),
        (f, dict(prev=f[0].float()), "prev must be"),
        (f, dict(prev=torch.zeros((16, 24, 6), dtype=torch.uint8, device=gpu_device)[..., ::2]), "prev must be"),
        (f, dict(out=(sc, tc.float())), "out must be"),
        (f, dict(out=(sc,)), "out must be"),
        (f, dict(out=(sc, tc[:1])), "out must be"),
        (f, dict(out=(sc.cpu(), tc.cpu())), "out must be"),
    ]
    for frames, kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            complexity.block_complexity_device(frames, **{"block_size": 16, **kw})
    torch.cuda.synchronize()
    assert (sbuf.cpu().numpy() == SENTINEL).all() and (tbuf.cpu().numpy() == SENTINEL).all()
    assert h.elvis_last_launch() == marker
    # the same conditions at the C boundary, with real device pointers
    dct_d, weight_d = complexity._device_tables(16, gpu_device)
    args = lambda **k: [k.get("frames", f.data_ptr()), None, dct_d.data_ptr(), weight_d.data_ptr(), sc.data_ptr(), tc.data_ptr(),
                        2, k.get("h", 16), k.get("w", 24), k.get("c", 3), 0, k.get("block", 16), None]
    for kw, word in ((dict(block=12), b"block"), (dict(c=2), b"channels"), (dict(h=15), b"bad shape"), (dict(w=15), b"bad shape"),
                     (dict(frames=None), b"null")):
        assert h.elvis_block_complexity_f64(*args(**kw)) == -1 and word in h.elvis_last_error()
    # no frames: nothing is launched, the (empty) outputs come back
    empty = complexity.block_complexity_device(f[:0], 8)
    assert empty[0].shape == empty[1].shape == (0, 2, 3) and h.elvis_last_launch() == marker
