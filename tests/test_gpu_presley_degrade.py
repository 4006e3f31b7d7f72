"""Presley's adaptive degraders on the device, bit-exact against the numpy restatement (tests/_presley_degrade_ref.py):
the two device forms over every block size class, map value, channel count and a ragged frame; old kernel against new
kernel where both apply; the seven public functions; the golden maps through the public functions; the round trip into
the classical restorers; the error paths."""
import os

import numpy as np
import pytest
import torch

import _classical_ref as CR
import _presley_degrade_ref as R

pytestmark = pytest.mark.gpu


def _frames(seed, n, h, w, c=3):
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, c), dtype=np.uint8)


def _ragged(extra, b):
    """Rows or columns past the last whole block: `extra` of them, fewer where that would make another block."""
    return min(extra, b - 1)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _launched():
    from elvis_amd import _lib
    return _lib.lib().elvis_last_launch().decode()


def _check_device_form(fn, ref_fn, frames, maps, b, device):
    """With and without `out=`; the rows and columns past the last whole block: returned as the input's without `out`,
    left as the caller put them with it.  The launch note names the form's one kernel."""
    n, h, w, _ = frames.shape
    by, bx = maps.shape[1:]
    ref = ref_fn(frames, maps, b)
    fd, md = _dev(frames, device), _dev(maps, device)
    got = fn(fd, md, b)
    assert _launched() == {"degrade_scale_device": "degrade_scale_kernel", "degrade_gaussian_fx_device": "degrade_gaussian_fx_kernel"}[fn.__name__]
    assert got.data_ptr() != fd.data_ptr() and np.array_equal(fd.cpu().numpy(), frames)
    assert np.array_equal(got.cpu().numpy(), ref)
    assert np.array_equal(ref[:, by * b:], frames[:, by * b:]) and np.array_equal(ref[:, :, bx * b:], frames[:, :, bx * b:])
    out = torch.full_like(fd, 7)
    assert fn(fd, md, b, out=out) is out
    expect = np.full_like(frames, 7)
    expect[:, :by * b, :bx * b] = ref[:, :by * b, :bx * b]
    assert np.array_equal(out.cpu().numpy(), expect)
    return ref


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("b", [2, 8, 12, 16, 20, 32])
def test_degrade_scale_device(gpu_device, b, c):
    from elvis_amd import degrade as D
    values = np.arange(-1, b + 2, dtype=np.int32)                 # one block per scale -1 .. b + 1
    bx = (len(values) + 1) // 2
    grid = np.full(2 * bx, 3, np.int32)
    grid[:len(values)] = values
    maps = np.stack([grid.reshape(2, bx), grid[::-1].reshape(2, bx)])
    frames = _frames(100 * b + c, 2, 2 * b + _ragged(3, b), bx * b + _ragged(5, b), c)
    ref = _check_device_form(D.degrade_scale_device, R.scale_clip, frames, maps, b, gpu_device)
    keep = np.repeat(np.repeat(maps <= 1, b, 1), b, 2)
    assert np.array_equal(ref[:, :2 * b, :bx * b][keep], frames[:, :2 * b, :bx * b][keep])
    assert not np.array_equal(ref, frames)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("b", [2, 3, 5, 8, 16, 32])
def test_degrade_gaussian_fx_device(gpu_device, b, c):
    from elvis_amd import degrade as D
    maps = np.array([[[-1, 0, 1], [2, 10, 64]], [[64, 10, 2], [1, 0, -1]]], np.int32)
    frames = _frames(200 * b + c, 2, 2 * b + _ragged(3, b), 3 * b + _ragged(5, b), c)
    ref = _check_device_form(D.degrade_gaussian_fx_device, R.blur_clip, frames, maps, b, gpu_device)
    assert np.array_equal(ref[0, :b, :2 * b], frames[0, :b, :2 * b]) and not np.array_equal(ref[0, :b, 2 * b:3 * b], frames[0, :b, 2 * b:3 * b])
    # nothing leaks between blocks: inverting one block changes only that block
    other = frames.copy()
    other[0, b:2 * b, b:2 * b] = 255 - other[0, b:2 * b, b:2 * b]
    got = D.degrade_gaussian_fx_device(_dev(other, gpu_device), _dev(maps, gpu_device), b).cpu().numpy()
    diff = np.any(got != ref, axis=3)
    assert diff[0, b:2 * b, b:2 * b].any()
    diff[0, b:2 * b, b:2 * b] = False
    assert not diff.any()
    maps[1, 1, 1] = 65
    with pytest.raises(ValueError, match="rounds"):
        D.degrade_gaussian_fx_device(_dev(frames, gpu_device), _dev(maps, gpu_device), b)


@pytest.mark.parametrize("b", [2, 12, 32])
def test_two_channels_through_both_kernels(gpu_device, b):
    """c = 2 is inside check_block_maps' 1..4 and has a branch of its own in pixel_of (xc >> 1): every scale of a block
    size, whole ratios and fractional ones, and 0, 1, 2 and 10 blur rounds, on a ragged frame."""
    from elvis_amd import degrade as D
    values = np.arange(-1, b + 2, dtype=np.int32)
    bx = (len(values) + 1) // 2
    grid = np.full(2 * bx, 3, np.int32)
    grid[:len(values)] = values
    maps = np.stack([grid.reshape(2, bx), grid[::-1].reshape(2, bx)])
    frames = _frames(800 * b + 2, 2, 2 * b + _ragged(3, b), bx * b + _ragged(5, b), 2)
    ref = _check_device_form(D.degrade_scale_device, R.scale_clip, frames, maps, b, gpu_device)
    assert not np.array_equal(ref, frames)
    maps = np.array([[[-1, 0, 1], [2, 10, 64]], [[64, 10, 2], [1, 0, -1]]], np.int32)
    frames = _frames(900 * b + 2, 2, 2 * b + _ragged(3, b), 3 * b + _ragged(5, b), 2)
    ref = _check_device_form(D.degrade_gaussian_fx_device, R.blur_clip, frames, maps, b, gpu_device)
    assert not np.array_equal(ref[0, :b, 2 * b:3 * b], frames[0, :b, 2 * b:3 * b])


@pytest.mark.parametrize("b", [2, 4, 8, 16])
def test_new_scale_kernel_equals_old_downsample_kernel(gpu_device, b):
    from elvis_amd import degrade as D
    frames = _frames(300 + b, 2, 3 * b, 5 * b)
    levels = np.random.default_rng(b).integers(0, 5, size=(2, 3, 5)).astype(np.int32)
    levels.flat[:5] = np.arange(5)
    scales = np.where(levels > 0, 1 << levels, 0).astype(np.int32)
    fd = _dev(frames, gpu_device)
    old = D.degrade_downsample_device(fd, _dev(levels, gpu_device), b)
    new = D.degrade_scale_device(fd, _dev(scales, gpu_device), b)
    assert torch.equal(old, new)


@pytest.mark.parametrize("h,w,b", [(64, 96, 8), (32, 48, 16)])
def test_filter_frame_gaussian_arithmetic(gpu_device, h, w, b):
    from elvis_amd import degrade as D
    from oracle import degrade_ref
    img = _frames(400 + b, 1, h, w)[0]
    scores = np.random.default_rng(b).random((h // b, w // b))
    scores.flat[0], scores.flat[1] = 0.0, 1.0
    fx, rounds = D.filter_frame_gaussian(img, scores, b, gpu_device, arithmetic="opencv")
    assert rounds.dtype == np.int32 and np.array_equal(rounds, np.round(scores * 10).astype(np.int32)) and rounds.max() == 10
    dev = D.degrade_gaussian_fx_device(_dev(img[None], gpu_device), _dev(rounds[None], gpu_device), b)[0].cpu().numpy()
    assert np.array_equal(fx, dev) and np.array_equal(fx, R.blur_clip(img[None], rounds[None], b)[0])
    f32, rounds32 = D.filter_frame_gaussian(img, scores, b, gpu_device)
    ref, _ = degrade_ref.filter_frame_gaussian(img, scores, b)
    assert np.array_equal(f32, ref) and np.array_equal(rounds32, rounds)
    assert not np.array_equal(f32, fx)                            # the two arithmetics do differ


@pytest.mark.parametrize("h,w", [(43, 59), (64, 96)])
@pytest.mark.parametrize("b", [8, 16])
def test_public_functions(gpu_device, h, w, b):
    import elvis_amd as E
    frames = list(_frames(h + b, 3, h, w))
    by, bx = h // b, w // b
    rng = np.random.default_rng(h * b)
    imps = [rng.random((by, bx)), rng.random((by, bx)).astype(np.float32), rng.integers(0, 5, size=(by, bx)) / 4]
    imps[2].flat[:2] = 0.0, 1.0                                   # the strongest degrade and an untouched block
    for imp in imps[:2]:
        got, gmap = E.degrade_adaptive_downsample(frames[0], imp, b, device=gpu_device)
        ref, rmap = R.degrade_adaptive_downsample(frames[0], imp, b)
        assert gmap.dtype == np.int32 and np.array_equal(gmap, rmap) and set(np.unique(gmap)) <= {0, 2, 3, 4}
        assert np.array_equal(got, ref)
        got, gmap = E.degrade_adaptive_blur(frames[1], imp, b, device=gpu_device)
        ref, rmap = R.degrade_adaptive_blur(frames[1], imp, b)
        assert gmap.dtype == np.int32 and np.array_equal(gmap, rmap) and gmap.max() <= 10
        assert np.array_equal(got, ref)
    got, gmap = E.degrade_adaptive_downsample(frames[2], imps[2], b, 7, gpu_device)
    ref, rmap = R.degrade_adaptive_downsample(frames[2], imps[2], b, 7)
    assert np.array_equal(gmap, rmap) and gmap.max() == 7 and np.array_equal(got, ref)
    for imp in imps:
        assert np.array_equal(E.generate_degradation_map(imp, 4), R.generate_degradation_map(imp, 4))
    block = np.ascontiguousarray(frames[0][:b, :b])
    for scale in (1, 2, 3, 5, b, b + 1):
        assert np.array_equal(E.downscale_block(block, scale, gpu_device), R.downscale_block(block, scale)), scale
    for rounds in (1, 3):
        assert np.array_equal(E.blur_block(block, rounds, gpu_device), R.blur_block(block, rounds)), rounds
    for method, ref_method, max_value in ((E.downscale_block, R.downscale_block, 4), (E.blur_block, R.blur_block, 4),
                                          (E.blur_block, R.blur_block, 10)):
        dmap = R.generate_degradation_map(imps[0], max_value)
        assert np.array_equal(E.degrade_frame(frames[0], dmap, b, method, gpu_device), R.degrade_frame(frames[0], dmap, b, ref_method))
        got, gmaps = E.degrade_video_adaptive(frames, imps, b, max_value, method, gpu_device)
        ref, rmaps = R.degrade_video_adaptive(frames, imps, b, max_value, ref_method)
        assert len(got) == len(gmaps) == 3
        for i in range(3):
            assert gmaps[i].dtype == np.int32 and np.array_equal(gmaps[i], rmaps[i])
            assert got[i].shape == frames[i].shape and np.array_equal(got[i], ref[i])
    # zip semantics: the shorter of the two lists decides
    assert len(E.degrade_video_adaptive(frames, imps[:2], b, 4, E.blur_block, gpu_device)[0]) == 2


def test_golden_maps_through_the_public_functions(gpu_device, golden_dir):
    import elvis_amd as E
    cases, _ = R.golden_cases(os.path.join(golden_dir, "presley_degrade.npz"))
    for k, c in enumerate(cases):
        by, bx = c["importance"].shape
        b, mx = c["block"], c["max_value"]
        frame = _frames(500 + k, 1, by * b + c["extra"][0], bx * b + c["extra"][1])[0]
        if c["family"] == "utils_downsample":
            got, gmap = E.degrade_adaptive_downsample(frame, c["importance"], b, mx, gpu_device)
        elif c["family"] == "utils_blur":
            got, gmap = E.degrade_adaptive_blur(frame, c["importance"], b, mx, gpu_device)
        else:
            method = E.downscale_block if c["family"] == "presley_downsample" else E.blur_block
            got, gmap = (r[0] for r in E.degrade_video_adaptive([frame], [c["importance"]], b, mx, method, gpu_device))
        assert gmap.dtype == np.int32 and np.array_equal(gmap, c["map"]), c["family"]
        ref_fn = R.scale_clip if "downsample" in c["family"] else R.blur_clip
        assert np.array_equal(got, ref_fn(frame[None], c["map"][None], b)[0]), c["family"]
        changed = np.any(got[:by * b, :bx * b].reshape(by, b, bx, b, 3) != frame[:by * b, :bx * b].reshape(by, b, bx, b, 3), axis=(1, 3, 4))
        assert not changed[c["touched"] == 0].any()


@pytest.mark.parametrize("h,w,b", [(64, 96, 16), (43, 59, 8)])
def test_round_trip_into_the_classical_restorers(gpu_device, h, w, b):
    import elvis_amd as E
    frame = _frames(600 + b, 1, h, w)[0]
    imp = np.random.default_rng(b).random((h // b, w // b))
    blurred, rounds = E.degrade_adaptive_blur(frame, imp, b, 4, gpu_device)
    restored = E.restore_with_opencv_unsharp([blurred], [rounds], b, device=gpu_device)
    ref_blurred, ref_rounds = R.degrade_adaptive_blur(frame, imp, b, 4)
    assert np.array_equal(restored[0], CR.ref_restore_with_opencv_unsharp([ref_blurred], [ref_rounds], b)[0])
    small, scales = E.degrade_adaptive_downsample(frame, imp, b, 4, gpu_device)
    restored = E.restore_with_opencv_lanczos([small], [scales], b, device=gpu_device)
    ref_small, ref_scales = R.degrade_adaptive_downsample(frame, imp, b, 4)
    assert np.array_equal(restored[0], CR.ref_restore_with_opencv_lanczos([ref_small], [ref_scales], b)[0])
    assert not np.array_equal(restored[0], small)


def test_errors(gpu_device):
    import elvis_amd as E
    from elvis_amd import degrade as D
    frame = _frames(700, 1, 32, 48)[0]
    imp = np.zeros((2, 3))
    with pytest.raises(ValueError, match="method"):
        E.degrade_frame(frame, np.ones((2, 3), np.int32), 16, R.blur_block, gpu_device)
    with pytest.raises(ValueError, match="method"):
        E.degrade_video_adaptive([frame], [imp], 16, 4, lambda blk, lv: blk, gpu_device)
    for fn in (E.degrade_adaptive_downsample, E.degrade_adaptive_blur):
        with pytest.raises(ValueError, match="block grid"):
            fn(frame, np.zeros((4, 6)), 16, device=gpu_device)
        with pytest.raises(ValueError, match="uint8"):
            fn(frame.astype(np.int16), imp, 16, device=gpu_device)
    fd = _dev(frame[None], gpu_device)
    for fn in (D.degrade_scale_device, D.degrade_gaussian_fx_device):
        for b in (1, 33):
            with pytest.raises(ValueError, match="block_size"):
                fn(fd, torch.zeros((1, 32 // b, 48 // b), dtype=torch.int32, device=gpu_device), b)
        with pytest.raises(ValueError):
            fn(fd.to(torch.int16), torch.zeros((1, 2, 3), dtype=torch.int32, device=gpu_device), 16)
        with pytest.raises(ValueError, match="block grid"):
            fn(fd, torch.zeros((1, 3, 2), dtype=torch.int32, device=gpu_device), 16)
        with pytest.raises(ValueError):
            fn(fd, torch.zeros((1, 2, 3), dtype=torch.int64, device=gpu_device), 16)
        with pytest.raises(ValueError):
            fn(fd, torch.zeros((1, 2, 3), dtype=torch.int32, device=gpu_device), 16, out=torch.empty((1, 32, 48, 4), dtype=torch.uint8, device=gpu_device))
    # a frame smaller than one block holds no block: it comes back as it is
    tiny = _dev(frame[None, :8, :8], gpu_device)
    assert torch.equal(D.degrade_scale_device(tiny, torch.zeros((1, 0, 0), dtype=torch.int32, device=gpu_device), 16), tiny)
