"""The temporal fill on the device (csrc/tfill.hip) against its numpy statement (tests/_tfill_ref.py): every comparison
is exact equality on bytes.  The references are computed once per module and never modified."""
import importlib
import os

import numpy as np
import pytest
import torch

import _inpaint_ref as I
import _shrink_ref as S
import _tfill_ref as R
import elvis_amd
from elvis_amd import _lib, drivers, frameio

# the package exports the function `inpaint_temporal` under the module's own name: the module comes from the import system
inpaint_temporal = importlib.import_module("elvis_amd.inpaint_temporal")

pytestmark = pytest.mark.gpu

CASES = R.cases()
_expected = {}


def expected(name):
    """The statement's (out, left) of a case, computed once; read-only."""
    if name not in _expected:
        frames, masks, p = CASES[name]
        out, left = R.temporal_fill(frames, masks, **p)
        out.setflags(write=False)
        left.setflags(write=False)
        _expected[name] = (out, left)
    return _expected[name]


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)          # a copy: the shared references are read-only


def _report(name, got, ref):
    diff = got != ref
    return f"{name}: {int(diff.sum())} bytes differ, first at {tuple(np.argwhere(diff)[0]) if diff.any() else None}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_numpy_statement(gpu_device, name):
    frames, masks, p = CASES[name]
    ref_out, ref_left = expected(name)
    fd, md = _dev(frames, gpu_device), _dev(masks, gpu_device)
    out, left = inpaint_temporal.temporal_fill_device(fd, md, **p)
    assert out.shape == fd.shape and out.dtype == torch.uint8 and out.data_ptr() != fd.data_ptr()
    assert left.shape == md.shape and left.dtype == torch.uint8
    assert torch.equal(left, _dev(ref_left, gpu_device)), _report(name + " left", left.cpu().numpy(), ref_left)
    assert torch.equal(out, _dev(ref_out, gpu_device)), _report(name + " out", out.cpu().numpy(), ref_out)
    assert np.array_equal(fd.cpu().numpy(), frames) and np.array_equal(md.cpu().numpy(), masks)     # inputs unchanged
    assert _lib.lib().elvis_last_launch().decode() == f"tfill_kernel<{frames.shape[3]}>"
    # known pixels and the bytes under `left` are the input's, on the raw tensors
    keep = (md == 0) | (left != 0)
    assert torch.equal(out[keep], fd[keep])
    assert not ((left != 0) & (md == 0)).any() and set(torch.unique(left).tolist()) <= {0, 255}


def test_block_masks_equal_their_expansion(gpu_device):
    rng = np.random.default_rng(70)
    for (h, w, c, mb) in ((48, 64, 3, 16), (33, 49, 1, 8)):
        noisy, _ = R.pan_clip(4, h, w, c, seed=71)
        bm = rng.random((4, h // mb, w // mb)) < 0.3
        full = R.expand_block_mask(bm, mb, h, w)
        frames = R.holed(noisy, full, seed=72)
        ref_out, ref_left = R.temporal_fill(frames, full, block=8, margin=8, radius=2, search=5, max_mad=6)
        fd = _dev(frames, gpu_device)
        for mask in (bm, bm.astype(np.uint8) * 7, bm.astype(np.int8)):
            out, left = inpaint_temporal.temporal_fill_blocks_device(fd, _dev(mask, gpu_device), mb, block=8, margin=8, search=5)
            assert torch.equal(out, _dev(ref_out, gpu_device)) and torch.equal(left, _dev(ref_left, gpu_device))


def test_inpaint_temporal_equals_the_statement_followed_by_the_telea_statement(gpu_device):
    rng = np.random.default_rng(73)
    noisy, _ = R.pan_clip(4, 48, 64, 3, seed=74)
    bm = rng.random((4, 3, 4)) < 0.3
    full = R.expand_block_mask(bm, 16, 48, 64)
    frames = R.holed(noisy, full, value=0)
    out, left = R.temporal_fill(frames, full)
    assert 0 < (left != 0).sum() < (full != 0).sum()
    ref = I.inpaint(out, left)
    fd, md = _dev(frames, gpu_device), _dev(full, gpu_device)
    got = elvis_amd.inpaint_temporal_device(fd, md)
    assert got.data_ptr() != fd.data_ptr() and torch.equal(got, _dev(ref, gpu_device))
    assert np.array_equal(fd.cpu().numpy(), frames)
    for arg in (frames, [f for f in frames]):
        host = elvis_amd.inpaint_temporal(arg, bm, device=str(gpu_device))
        assert isinstance(host, np.ndarray) and host.dtype == np.uint8 and np.array_equal(host, ref)
    # a frame strided in memory is read as it is
    wide = torch.zeros((4, 48, 64, 6), dtype=torch.uint8, device=gpu_device)
    wide[..., ::2] = fd
    assert torch.equal(elvis_amd.inpaint_temporal_device(wide[..., ::2], md), got)


def test_the_library_refuses_an_aliased_output(gpu_device):
    frames, masks, p = CASES["defaults_48x64"]
    fd, md = _dev(frames, gpu_device), _dev(masks, gpu_device)
    left = torch.empty_like(md)
    n, h, w, c = fd.shape
    rc = _lib.lib().elvis_tfill(fd.data_ptr(), md.data_ptr(), 0, fd.data_ptr(), left.data_ptr(), n, h, w, c, 16, 8, 2, 7, 6, None)
    assert rc == -1 and b"alias" in _lib.lib().elvis_last_error()
    assert np.array_equal(fd.cpu().numpy(), frames)


def _shrunk_pan(n=5, by=5, bx=7, b=8, k=2, seed=80):
    rng = np.random.default_rng(seed)
    noisy, _ = R.pan_clip(n, by * b, bx * b, 3, seed=seed)
    masks = np.zeros((n, by, bx), np.uint8)
    shrunk = []
    for i in range(n):
        for r in range(by):
            masks[i, r, rng.choice(bx, k, replace=False)] = 1
        rows = [np.concatenate([noisy[i, r * b:(r + 1) * b, c * b:(c + 1) * b] for c in range(bx) if not masks[i, r, c]], axis=1)
                for r in range(by)]
        shrunk.append(np.concatenate(rows, axis=0))
    return shrunk, masks, b


PARAMS = dict(block=8, margin=8, radius=2, search=4, max_mad=8)


@pytest.fixture(scope="module")
def shrunk_reference():
    """The composition the driver must equal: the stretch, the fill's statement, the Telea statement."""
    shrunk, masks, b = _shrunk_pan()
    stretched = np.stack([S.stretch_frame(shrunk[i], masks[i], b) for i in range(len(shrunk))])
    full = R.expand_block_mask(masks, b, stretched.shape[1], stretched.shape[2])
    out, left = R.temporal_fill(stretched, full, **PARAMS)
    assert 0 < (left != 0).sum() < (full != 0).sum()
    ref = I.inpaint(out, left)
    for a in (stretched, full, ref):
        a.setflags(write=False)
    return shrunk, masks, b, stretched, full, ref


def test_the_result_is_independent_of_sharding(gpu_device, shrunk_reference, tmp_path, monkeypatch):
    """The shard step on [0, 3) and [3, 5), each with `radius` frames of context, concatenated, equals the whole clip;
    the side directories get every file once."""
    shrunk, masks, b, stretched, full, ref = shrunk_reference
    written = []
    write_clip = drivers._write_clip
    monkeypatch.setattr(drivers, "_write_clip", lambda clip, d, names, w: (written.extend((d, n) for n in names),
                                                                          write_clip(clip, d, names, w)))
    st, fm = tmp_path / "stretched", tmp_path / "full"
    st.mkdir(), fm.mkdir()
    n, halo = len(shrunk), PARAMS["radius"]
    parts = []
    for start, end in ((0, 3), (3, 5)):
        lo, hi = max(0, start - halo), min(n, end + halo)
        clip = _dev(np.stack(shrunk[lo:hi]), gpu_device)
        got = drivers._v1_shard(clip, masks[lo:hi], b, gpu_device, lo, inpaint=True, stretched_dir=str(st),
                                fullres_masks_dir=str(fm), inpainter="temporal", inpaint_params=PARAMS, own=(start, end))
        assert len(got) == hi - lo
        parts.append(got[start - lo:end - lo])
    assert torch.equal(torch.cat(parts), _dev(ref, gpu_device))
    whole = drivers._v1_shard(_dev(np.stack(shrunk), gpu_device), masks, b, gpu_device, 0, inpaint=True, inpainter="temporal",
                              inpaint_params=PARAMS)
    assert torch.equal(whole, _dev(ref, gpu_device))
    names = [f"{i + 1:05d}.png" for i in range(n)]
    assert sorted(written) == sorted((str(d), name) for d in (st, fm) for name in names)
    assert sorted(os.listdir(st)) == sorted(os.listdir(fm)) == names
    for i, name in enumerate(names):
        assert np.array_equal(frameio.load_frame(st / name), stretched[i])


def test_restore_shrunk_frames_temporal_equals_the_composition(gpu_device, shrunk_reference, tmp_path):
    from PIL import Image
    shrunk, masks, b, stretched, full, ref = shrunk_reference
    shrunk, masks = shrunk[:4], masks[:4]
    out4, left4 = R.temporal_fill(stretched[:4], full[:4], **PARAMS)
    ref4 = I.inpaint(out4, left4)
    d = tmp_path / "frames"
    d.mkdir()
    for i, f in enumerate(shrunk):
        frameio.save_frame(f, d / f"{i + 1:05d}.png")
    frameio.save_block_masks(masks, tmp_path / "shrink_masks_8.npz")
    out, st, fm = tmp_path / "inpainted", tmp_path / "stretched", tmp_path / "full"
    got = drivers.restore_shrunk_frames(str(d), str(tmp_path / "shrink_masks_8.npz"), b, str(out), stretched_dir=str(st),
                                        fullres_masks_dir=str(fm), devices=[gpu_device], inpainter="temporal",
                                        inpaint_params=PARAMS)
    assert np.array_equal(got, masks)
    names = [f"{i + 1:05d}.png" for i in range(4)]
    assert sorted(os.listdir(out)) == sorted(os.listdir(st)) == sorted(os.listdir(fm)) == names
    for i, name in enumerate(names):
        assert np.array_equal(frameio.load_frame(out / name), ref4[i]), name
        assert np.array_equal(frameio.load_frame(st / name), stretched[i])
        assert np.array_equal(frameio.load_frame(d / name), shrunk[i])
        with Image.open(fm / name) as im:
            assert np.array_equal(np.asarray(im), full[i])
    # the default is the wavefront Telea alone, as before
    plain = tmp_path / "plain"
    drivers.restore_shrunk_frames(str(d), str(tmp_path / "shrink_masks_8.npz"), b, str(plain), devices=[gpu_device])
    tel = I.inpaint(stretched[:4], full[:4])
    assert all(np.array_equal(frameio.load_frame(plain / name), tel[i]) for i, name in enumerate(names))
    assert not np.array_equal(tel, ref4)
