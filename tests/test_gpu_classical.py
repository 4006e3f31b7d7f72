"""Classical restorers on the device (Lanczos, unsharp mask, temporal blend) against the numpy restatement in
tests/_classical_ref.py: bit-exact, np.array_equal everywhere."""
import numpy as np
import pytest
import torch

import _classical_ref as R

pytestmark = pytest.mark.gpu


def _frame(h, w, c, seed):
    rng = np.random.default_rng(seed)
    base = rng.random((h // 4 + 1, w // 4 + 1, c))
    up = np.kron(base, np.ones((4, 4, 1)))[:h, :w]
    return np.round(np.clip(up + rng.normal(0, 0.15, up.shape), 0, 1) * 255).astype(np.uint8)


def _levels(by, bx, b, seed):
    """Random levels plus the corner cases: 0, 1, log2 b, above log2 b and 10."""
    lb = int(np.log2(b))
    lv = np.random.default_rng(seed).integers(0, lb + 3, size=(by, bx)).astype(np.int32)
    lv.flat[:5] = [0, 1, lb, lb + 1, 10]
    return lv


@pytest.mark.parametrize("b", [2, 4, 8, 16, 32])
@pytest.mark.parametrize("c", [1, 3])
def test_lanczos_blocks(gpu_device, b, c):
    from elvis_amd import classical
    h, w = 2 * b, 4 * b
    img = _frame(h, w, c, b + c)
    lv = _levels(2, 4, b, b)
    got = classical.restore_downsample_opencv_lanczos(img, lv, b, device=gpu_device)
    assert np.array_equal(got, R.lanczos_restore(img[None], lv[None], b)[0])
    assert np.array_equal(got, R.ref_restore_downsample_opencv_lanczos(img, lv, b))
    assert np.array_equal(got[:b, :b], img[:b, :b]) and not np.array_equal(got, img)


@pytest.mark.parametrize("b", [2, 4, 8, 16, 32])
@pytest.mark.parametrize("c", [1, 3])
def test_unsharp_blocks(gpu_device, b, c):
    from elvis_amd import classical
    h, w = 2 * b, 4 * b
    img = _frame(h, w, c, 40 + b + c)
    lv = _levels(2, 4, b, 50 + b)
    got = classical.restore_blur_opencv_unsharp_mask(img, lv.astype(np.float64) + 0.7, b, device=gpu_device)  # int() truncates
    assert np.array_equal(got, R.unsharp_restore(img[None], lv[None], b)[0])
    assert np.array_equal(got, R.ref_restore_blur_opencv_unsharp_mask(img, lv, b))


def test_lanczos_flat_block_at_factor_16(gpu_device):
    """f = 16 has phases whose taps sum to 2046..2050, yet a flat u8 block comes back flat (the host test
    test_lanczos_flat_blocks_stay_flat proves it for every phase pair); s = 1 takes the full Lanczos path."""
    from elvis_amd import classical
    for v in (0, 1, 128, 200, 255):
        img = np.full((16, 32, 3), v, np.uint8)
        img[:, 16:] = 255 - v
        lv = np.array([[4, 0]], np.int32)
        got = classical.restore_downsample_opencv_lanczos(img, lv, 16, device=gpu_device)
        assert np.array_equal(got, R.lanczos_restore(img[None], lv[None], 16)[0])
        assert np.array_equal(got, img)


@pytest.mark.parametrize("halo", [0, 4, 16])
def test_unsharp_halo_clipped_at_every_edge(gpu_device, halo):
    """Every block of a 5 x 6 grid has level > 0, so the tiles of the border blocks are clipped at all four edges."""
    from elvis_amd import classical
    b, h, w = 8, 40, 48
    clip = np.stack([_frame(h, w, 3, 60 + i) for i in range(2)])
    lv = np.random.default_rng(halo).integers(1, 6, size=(2, 5, 6)).astype(np.int32)
    lv[0, 2, 3] = 10
    fd = torch.from_numpy(clip).to(gpu_device)
    got = classical.unsharp_restore_device(fd, torch.from_numpy(lv).to(gpu_device), b, halo=halo).cpu().numpy()
    assert np.array_equal(got, R.unsharp_restore(clip, lv, b, halo))
    frames = classical.restore_with_opencv_unsharp(list(clip), list(lv), b, halo=halo, device=gpu_device)
    assert np.array_equal(np.stack(frames), got)


@pytest.mark.parametrize("halo,tb", [(0, 0.0), (4, 0.3), (16, 0.3)])
def test_utils_surface(gpu_device, halo, tb):
    """Frame sizes b does not divide, a map of the wrong shape, a missing map, temporal blend over 5 frames."""
    from elvis_amd import classical
    b, h, w = 8, 43, 61
    frames = [_frame(h, w, 3, 70 + i) for i in range(5)]
    rng = np.random.default_rng(int(tb * 10) + halo)
    maps = [rng.integers(0, 5, size=(5, 7)) for _ in range(3)] + [rng.integers(0, 5, size=(3, 4))]   # 5th: missing
    ref = R.ref_restore_with_opencv_unsharp(frames, maps, b, halo=halo, temporal_blend=tb)
    for fn in (classical.restore_with_opencv_unsharp, classical.restore_with_opencv_lanczos):
        got = fn(frames, maps, b, halo=halo, temporal_blend=tb, device=gpu_device, tile_coords=None)
        assert len(got) == 5 and all(np.array_equal(g, r) for g, r in zip(got, ref))
    assert np.array_equal(got[0][40:], frames[0][40:]) and np.array_equal(got[0][:, 56:], frames[0][:, 56:])


def test_all_zero_map_returns_input(gpu_device):
    from elvis_amd import classical
    img = _frame(32, 48, 3, 80)
    zero = np.zeros((4, 6))
    assert classical.restore_downsample_opencv_lanczos(img, zero, 8, device=gpu_device) is img
    assert np.array_equal(classical.restore_blur_opencv_unsharp_mask(img, zero, 8, device=gpu_device), img)
    out = classical.restore_with_opencv_unsharp([img, img], [zero, zero], 8, halo=4, device=gpu_device)
    assert all(np.array_equal(o, img) for o in out)


def test_temporal_blend_device(gpu_device):
    from elvis_amd import classical
    clip = np.stack([_frame(24, 40, 3, 90 + i) for i in range(5)])
    fd = torch.from_numpy(clip).to(gpu_device)
    for tb in (0.0, 0.3, 1.0):
        got = classical.temporal_blend_device(fd, tb).cpu().numpy()
        assert np.array_equal(got, R.temporal_blend(clip, tb))
    inplace = fd.clone()
    classical.temporal_blend_device(inplace, 0.3, out=inplace)
    assert np.array_equal(inplace.cpu().numpy(), R.temporal_blend(clip, 0.3))


def test_device_and_numpy_entry_points_agree(gpu_device):
    from elvis_amd import classical
    b = 8
    clip = np.stack([_frame(48, 64, 3, 100 + i) for i in range(3)])
    lv = np.stack([_levels(6, 8, b, 110 + i) for i in range(3)])
    fd, ld = torch.from_numpy(clip).to(gpu_device), torch.from_numpy(lv).to(gpu_device)
    lz = classical.lanczos_restore_device(fd, ld, b).cpu().numpy()
    us = classical.unsharp_restore_device(fd, ld, b).cpu().numpy()
    for i in range(3):
        assert np.array_equal(lz[i], classical.restore_downsample_opencv_lanczos(clip[i], lv[i], b, device=gpu_device))
        assert np.array_equal(us[i], classical.restore_blur_opencv_unsharp_mask(clip[i], lv[i], b, device=gpu_device))
    with pytest.raises(ValueError):
        classical.lanczos_restore_device(fd, ld[:1], b)


def test_one_1080p_frame(gpu_device):
    from elvis_amd import classical, synth
    b = 8
    frame = synth.synth_clip(7, 1, 1080, 1920)[0]
    lv = synth.synth_level_maps(8, 1, 135, 240).astype(np.int32)[0]
    lv = np.minimum(lv, 4)
    lv[0, 0], lv[-1, -1] = 10, 3
    assert np.array_equal(classical.restore_downsample_opencv_lanczos(frame, lv, b, device=gpu_device),
                          R.lanczos_restore(frame[None], lv[None], b)[0])
    assert np.array_equal(classical.restore_blur_opencv_unsharp_mask(frame, lv, b, device=gpu_device),
                          R.unsharp_restore(frame[None], lv[None], b)[0])
    got = classical.restore_with_opencv_unsharp([frame], [lv], b, halo=8, device=gpu_device)[0]
    assert np.array_equal(got, R.unsharp_restore(frame[None], lv[None], b, 8)[0])
