"""The wavefront Telea inpainter on the device (csrc/inpaint.hip) against its numpy statement (tests/_inpaint_ref.py):
every comparison is exact equality on bytes.  The references are computed once per module and never modified."""
import os

import numpy as np
import pytest
import torch

import _inpaint_ref as R
import _shrink_ref as S
import elvis_amd
from elvis_amd import _lib, drivers, frameio, inpaint, shrink

pytestmark = pytest.mark.gpu

CASES = R.cases()
_expected = {}


def expected(name):
    """The reference output of a case, computed once; read-only."""
    if name not in _expected:
        frames, masks = CASES[name]
        ref = R.inpaint(frames, masks)
        ref.setflags(write=False)
        _expected[name] = ref
    return _expected[name]


def _launch():
    return _lib.lib().elvis_last_launch().decode()


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _report(name, got, ref, masks):
    diff = got != ref
    return f"{name}: {int(diff.sum())} bytes differ, first at {tuple(np.argwhere(diff)[0]) if diff.any() else None}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_numpy_statement(gpu_device, name):
    frames, masks = CASES[name]
    ref = expected(name)
    fd, md = _dev(frames, gpu_device), _dev(masks, gpu_device)
    got = inpaint.inpaint_device(fd, md)
    assert got.shape == fd.shape and got.dtype == torch.uint8 and got.data_ptr() != fd.data_ptr()
    got_h = got.cpu().numpy()
    assert np.array_equal(got_h, ref), _report(name, got_h, ref, masks)
    assert np.array_equal(fd.cpu().numpy(), frames) and np.array_equal(md.cpu().numpy(), masks)     # inputs unchanged
    assert _launch() == f"inpaint_fill_kernel<{frames.shape[3]}>"


@pytest.mark.parametrize("name", sorted(CASES))
def test_prepare_counts_the_pixels_of_every_wave(gpu_device, name):
    """The first h + w + 2 int32 of the workspace (include/elvis_amd.h) against np.bincount of the reference's wave index
    over the hole pixels of the frames that have a known pixel.  Nothing else of the workspace is read: its layout is
    not ABI."""
    frames, masks = CASES[name]
    n, h, w = masks.shape
    bins = h + w + 2
    want = R.wave_counts(masks)
    nbytes = _lib.lib().elvis_inpaint_workspace_bytes(n, h, w)
    assert nbytes >= 4 * bins
    md = _dev(masks, gpu_device)
    for sentinel in (0x00, 0xFF):                                        # whatever the workspace held before
        ws = torch.full((nbytes,), sentinel, dtype=torch.uint8, device=gpu_device)
        assert ws.data_ptr() % 256 == 0
        _lib.check(_lib.lib().elvis_inpaint_prepare(_lib.ptr(md), 0, _lib.ptr(ws), n, h, w, torch.cuda.current_stream(gpu_device).cuda_stream),
                   gpu_device)
        assert _launch() == "inpaint_scatter_kernel"
        got = ws[:4 * bins].view(torch.int32).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), \
            f"{name}: first difference at wave {int(np.flatnonzero(got != want)[0])}: device {got[got != want][:4]} reference {want[got != want][:4]}"
        deepest = int(np.flatnonzero(want)[-1]) if want.any() else 0
        assert got[0] == 0 and not got[deepest + 1:].any()
    assert np.array_equal(md.cpu().numpy(), masks)


@pytest.mark.parametrize("name", ["merged_2_3_L", "odd_random60", "mixed_clip", "interior_b8_c1", "deep_70x40", "wide_3x513"])
def test_in_place_garbage_under_the_holes_and_guarded_out(gpu_device, name):
    frames, masks = CASES[name]
    ref = expected(name)
    md = _dev(masks, gpu_device)
    fillable = [i for i in range(len(masks)) if not masks[i].all()]       # a frame without a known pixel stays as it is
    results = []
    for garbage in (0xA5, 0x5A):
        f = frames.copy()
        f[masks != 0] = garbage
        fd = _dev(f, gpu_device)
        same = inpaint.inpaint_device(fd, md, out=fd)                      # in place
        assert same is fd
        results.append(fd.cpu().numpy())
        assert np.array_equal(results[-1][fillable], ref[fillable]), _report(name, results[-1], ref, masks)
    assert np.array_equal(results[0][fillable], results[1][fillable])
    # out: a view into a sentinel-filled allocation, guard bytes on both sides
    n_bytes, guard = frames.size, 512
    buf = torch.full((n_bytes + 2 * guard,), 0xC3, dtype=torch.uint8, device=gpu_device)
    out = buf[guard:guard + n_bytes].view(frames.shape)
    fd = _dev(frames, gpu_device)
    assert inpaint.inpaint_device(fd, md, out=out) is out
    buf_h = buf.cpu().numpy()
    assert (buf_h[:guard] == 0xC3).all() and (buf_h[guard + n_bytes:] == 0xC3).all()
    assert np.array_equal(buf_h[guard:guard + n_bytes].reshape(frames.shape), ref)
    assert np.array_equal(fd.cpu().numpy(), frames)


def test_no_fill_launch_for_a_clip_without_holes(gpu_device):
    frames = R.make_image(37, 53, 3, seed=40)[None].repeat(2, axis=0)
    fd = _dev(frames, gpu_device)
    md = torch.zeros((2, 37, 53), dtype=torch.uint8, device=gpu_device)
    shrink.block_gather_device(_dev(frames[:, :32, :48], gpu_device), torch.zeros((2, 4, 6), dtype=torch.int32, device=gpu_device), 8)
    assert _launch().startswith("block_gather_u8_kernel")
    got = inpaint.inpaint_device(fd, md)
    assert _launch() == "inpaint_scatter_kernel"                         # the preparation ran, no fill followed
    assert np.array_equal(got.cpu().numpy(), frames)
    # nor for a clip without a known pixel
    got = inpaint.inpaint_device(fd, torch.full_like(md, 7), out=fd)
    assert _launch() == "inpaint_scatter_kernel" and np.array_equal(got.cpu().numpy(), frames)


def _block_case(c=3, b=8, h=44, w=61, n=3, seed=50):
    """Frames with rows and columns past the last whole block, and a removal mask per frame."""
    rng = np.random.default_rng(seed)
    frames = np.stack([R.make_image(h, w, c, seed=seed + i) for i in range(n)])
    bm = rng.random((n, h // b, w // b)) < 0.3
    bm[0, 0, 0] = bm[1, -1, -1] = True
    return frames, bm, b


def test_block_masks_are_expanded_over_whole_blocks(gpu_device):
    frames, bm, b = _block_case()
    ref = R.inpaint(frames, R.expand_block_mask(bm, b, frames.shape[1], frames.shape[2]))
    for dtype in (torch.bool, torch.uint8, torch.int8):
        md = torch.from_numpy(bm).to(gpu_device).to(dtype)
        got = inpaint.inpaint_blocks_device(_dev(frames, gpu_device), md, b).cpu().numpy()
        assert np.array_equal(got, ref), dtype
    one = frames[..., :1].copy()
    ref1 = R.inpaint(one, R.expand_block_mask(bm, b, frames.shape[1], frames.shape[2]))
    assert np.array_equal(inpaint.inpaint_blocks_device(_dev(one, gpu_device), _dev(bm, gpu_device), b).cpu().numpy(), ref1)


def test_reference_call_surface(gpu_device):
    dev = str(gpu_device)
    frames, bm, b = _block_case(h=40, w=56)
    full = R.expand_block_mask(bm, b, 40, 56)
    ref = R.inpaint(frames, full)
    f0, m0 = frames.copy(), bm.copy()
    for arg in (frames, [f for f in frames]):
        got = elvis_amd.inpaint_with_opencv(arg, bm, device=dev)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, ref)
    for i in range(len(frames)):
        got = elvis_amd.inpaint_frame(frames[i], full[i], device=dev)
        assert got.shape == frames[i].shape and np.array_equal(got, ref[i])
    grey = frames[0, :, :, 1].copy()
    got = elvis_amd.inpaint_frame(grey, full[0], device=dev)
    assert got.shape == grey.shape and np.array_equal(got, R.inpaint(grey[None, :, :, None], full[:1])[0, :, :, 0])
    assert np.array_equal(frames, f0) and np.array_equal(bm, m0)


def _shrunk_clip(n=6, by=5, bx=7, b=8, k=2, seed=60):
    rng = np.random.default_rng(seed)
    masks = np.zeros((n, by, bx), np.uint8)
    for i in range(n):
        for r in range(by):
            masks[i, r, rng.choice(bx, k, replace=False)] = 1
    shrunk = [R.make_image(by * b, (bx - k) * b, 3, seed=seed + i) for i in range(n)]
    return shrunk, masks, b


def test_stretch_and_inpaint_resident(gpu_device):
    shrunk, masks, b = _shrunk_clip()
    stretched = np.stack([S.stretch_frame(shrunk[i], masks[i], b) for i in range(len(shrunk))])
    ref = R.inpaint(stretched, R.expand_block_mask(masks, b, stretched.shape[1], stretched.shape[2]))
    sd, md = _dev(np.stack(shrunk), gpu_device), _dev(masks, gpu_device)
    got = elvis_amd.stretch_and_inpaint_device(sd, md, b)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), ref)
    assert np.array_equal(sd.cpu().numpy(), np.stack(shrunk))


def test_restore_shrunk_frames_equals_the_frame_level_path(gpu_device, tmp_path):
    from PIL import Image
    shrunk, masks, b = _shrunk_clip()
    d = tmp_path / "frames"
    d.mkdir()
    for i, f in enumerate(shrunk):
        frameio.save_frame(f, d / f"{i + 1:05d}.png")
    frameio.save_block_masks(masks, tmp_path / "shrink_masks_8.npz")
    out, st, full = tmp_path / "inpainted", tmp_path / "stretched", tmp_path / "full"
    got = drivers.restore_shrunk_frames(str(d), str(tmp_path / "shrink_masks_8.npz"), b, str(out), stretched_dir=str(st),
                                        fullres_masks_dir=str(full), devices=[gpu_device])
    assert np.array_equal(got, masks)
    names = [f"{i + 1:05d}.png" for i in range(len(shrunk))]
    assert sorted(os.listdir(out)) == sorted(os.listdir(st)) == sorted(os.listdir(full)) == names
    for i, name in enumerate(names):
        stretched = elvis_amd.stretch_frame(shrunk[i], masks[i], b, device=str(gpu_device))
        fullres = np.repeat(np.repeat(masks[i] * 255, b, 0), b, 1).astype(np.uint8)
        assert np.array_equal(frameio.load_frame(st / name), stretched)
        assert np.array_equal(frameio.load_frame(out / name), elvis_amd.inpaint_frame(stretched, fullres, device=str(gpu_device)))
        assert np.array_equal(frameio.load_frame(out / name), R.inpaint_frame(S.stretch_frame(shrunk[i], masks[i], b), fullres))
        assert np.array_equal(frameio.load_frame(d / name), shrunk[i])
        with Image.open(full / name) as im:
            assert np.array_equal(np.asarray(im), fullres)
