"""Classical restorers, host side: the tap tables against OpenCV's check values, the int32 headroom of the Lanczos
kernel, the vectorised restatement against the literal reference-loop port, the Python error paths and the C
entry points' argument checks (no GPU needed)."""
import numpy as np
import pytest

import _classical_ref as R
from elvis_amd import classical as C


def test_lanczos_check_values():
    first, taps = C.lanczos_taps(2, 2)
    assert taps[0].tolist() == [-8, 64, -188, 579, 1830, -312, 114, -31]
    assert taps[1].tolist() == taps[0][::-1].tolist()
    assert first.tolist() == [-4, -3]                     # sx = floor(-0.25) = -1 and floor(0.25) = 0, minus 3
    assert C.lanczos4_coeffs(0.0).tolist() == [0, 0, 0, 1, 0, 0, 0, 0]


def test_gaussian_check_values():
    assert C.gaussian_taps_u8(1).tolist() == [1, 14, 62, 102, 62, 14, 1]
    assert C.gaussian_taps_u8(2).tolist() == [1, 2, 7, 16, 31, 45, 52, 45, 31, 16, 7, 2, 1]


@pytest.mark.parametrize("level", range(1, 17))
def test_gaussian_taps_shape(level):
    t = C.gaussian_taps_u8(level)
    assert t.dtype == np.int16 and len(t) == 6 * level + 1 == (int(np.rint(level * 6 + 1)) | 1)
    assert np.array_equal(t, t[::-1]) and int(t.sum()) == 256 and (t >= 0).all()
    taps, offs = C.gaussian_tap_table()
    assert np.array_equal(taps[offs[level]:offs[level] + 6 * level + 1], t)


@pytest.mark.parametrize("f", C.LANCZOS_FACTORS)
def test_lanczos_taps_mirror_and_sums(f):
    _, t = C.lanczos_taps(f, f)
    for d in range(f):
        assert np.array_equal(t[d], t[f - 1 - d][::-1]), (f, d)
    sums = set(t.astype(np.int64).sum(axis=1).tolist())
    expect = {16: {2046, 2047, 2048, 2049, 2050}, 32: {2047, 2048, 2049}}.get(f, {2048})
    assert sums == expect
    # the device table repeats every f destination indices (the phase depends on d mod f only)
    table = C.lanczos_tap_table()
    assert table.shape == (5, 32, 8)
    row = table[int(np.log2(f)) - 1]
    assert all(np.array_equal(row[d], t[d % f]) for d in range(32))


def test_lanczos_int32_headroom():
    """Every partial sum of the kernel's vertical accumulator stays inside int32: a horizontal-pass value of phase
    a lies in [255 N(a), 255 P(a)] (P, N: sums of the positive / negative taps), so a partial sum over any vertical
    taps b is at most 255 (P(b) P(a) + N(b) N(a)) and at least 255 (P(b) N(a) + N(b) P(a)); + 2^21 rounding."""
    worst_hi, worst_lo = 0, 0
    for f in C.LANCZOS_FACTORS:
        t = C.lanczos_taps(f, 32)[1].astype(np.int64)
        p, n = np.where(t > 0, t, 0).sum(1), np.where(t < 0, t, 0).sum(1)
        worst_hi = max(worst_hi, int((255 * (p[:, None] * p[None, :] + n[:, None] * n[None, :])).max()) + (1 << 21))
        worst_lo = min(worst_lo, int((255 * (p[:, None] * n[None, :] + n[:, None] * p[None, :])).min()))
    assert worst_hi < 2 ** 31 and worst_lo > -2 ** 31


def test_lanczos_flat_blocks_stay_flat():
    """A flat block of value v gives (v S + 2^21) >> 22 with S the product of a horizontal and a vertical tap sum.
    The off-2048 sums of f = 16 and 32 keep |v (S - 2^22)| below 2^21 for every u8 v, so flat stays flat."""
    for f in C.LANCZOS_FACTORS:
        sums = C.lanczos_taps(f, f)[1].astype(np.int64).sum(axis=1)
        prod = sums[:, None] * sums[None, :]
        for v in range(256):
            assert ((v * prod + (1 << 21)) >> 22 == v).all(), (f, v)


def _frame(h, w, c, seed):
    rng = np.random.default_rng(seed)
    base = rng.random((h // 4 + 1, w // 4 + 1, c))
    up = np.kron(base, np.ones((4, 4, 1)))[:h, :w]
    return np.round(np.clip(up + rng.normal(0, 0.15, up.shape), 0, 1) * 255).astype(np.uint8)


@pytest.mark.parametrize("b,c", [(8, 3), (4, 1), (16, 3), (2, 3)])
def test_lanczos_vectorised_matches_reference_loop(b, c):
    h, w = 2 * b, 3 * b
    img = _frame(h, w, c, b)
    lv = np.random.default_rng(1).integers(0, int(np.log2(b)) + 3, size=(h // b, w // b))
    lv.flat[0], lv.flat[1] = 0, 10
    got = R.lanczos_restore(img[None], lv[None].astype(np.int32), b)[0]
    assert np.array_equal(got, R.ref_restore_downsample_opencv_lanczos(img, lv, b))


@pytest.mark.parametrize("b,c", [(8, 3), (4, 1), (16, 3)])
def test_unsharp_vectorised_matches_reference_loop(b, c):
    h, w = 3 * b, 4 * b
    img = _frame(h, w, c, 10 + b)
    lv = np.random.default_rng(2).integers(0, 5, size=(h // b, w // b))
    lv.flat[0], lv.flat[1] = 0, 10
    got = R.unsharp_restore(img[None], lv[None].astype(np.int32), b)[0]
    assert np.array_equal(got, R.ref_restore_blur_opencv_unsharp_mask(img, lv, b))


@pytest.mark.parametrize("halo,tb", [(0, 0.0), (3, 0.0), (8, 0.3), (20, 0.3)])
def test_utils_form_vectorised_matches_reference_loop(halo, tb):
    b, h, w = 8, 36, 45                                  # not divisible by b: rows / columns past the grid are copied
    rng = np.random.default_rng(halo)
    frames = [_frame(h, w, 3, 20 + i) for i in range(3)]
    maps = [rng.integers(0, 5, size=(4, 5)), rng.integers(0, 5, size=(2, 3))]   # second one resampled, third missing
    ref = R.ref_restore_with_opencv_unsharp(frames, maps, b, halo=halo, temporal_blend=tb)
    levels = np.stack([maps[0], R.nearest_resize(maps[1].astype(np.float32), 4, 5).astype(np.int32), np.zeros((4, 5))])
    got = R.unsharp_restore(np.stack(frames), levels.astype(np.int32), b, halo)
    if tb > 0:
        got = R.temporal_blend(got, tb)
    assert all(np.array_equal(g, r) for g, r in zip(got, ref))


def test_blend_rule_integer_form():
    """addWeighted in float32 equals round_half_even(((2 + L) x - L blur) / 2) for every u8 pair and level."""
    x, blur = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for level in range(1, 17):
        a = R.add_weighted_u8(x.astype(np.uint8), 1.0 + level * 0.5, blur.astype(np.uint8), -level * 0.5)
        v2 = (2 + level) * x - level * blur
        assert np.array_equal(a, np.clip(np.rint(v2 / 2.0), 0, 255).astype(np.uint8))


def test_python_value_errors():
    img = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(ValueError):                      # level above 16
        C.restore_downsample_opencv_lanczos(img, np.full((2, 2), 17), 8)
    with pytest.raises(ValueError):                      # factor int32(2 ** log2(6)): 5 or 6, not a power of two
        C.restore_downsample_opencv_lanczos(img, np.full((2, 2), np.log2(6.0)), 8)
    with pytest.raises(ValueError):
        C.restore_downsample_opencv_lanczos(img[:15], np.ones((2, 2)), 8)
    with pytest.raises(ValueError):
        C.restore_blur_opencv_unsharp_mask(img, np.full((2, 2), 17.0), 8)
    with pytest.raises(ValueError):
        C.restore_blur_opencv_unsharp_mask(img, np.ones((3, 2)), 8)
    with pytest.raises(ValueError):
        C.restore_with_opencv_unsharp([img], [np.full((2, 2), 1.5)], 8)
    with pytest.raises(ValueError):
        C.restore_with_opencv_lanczos([img], [np.full((2, 2), 17)], 8)
    with pytest.raises(ValueError):
        C.restore_with_opencv_unsharp([img], [np.ones((2, 2))], 8, halo=33)
    with pytest.raises(ValueError):
        C.restore_with_opencv_unsharp([img], [np.ones((2, 2))], 8, temporal_blend=1.5)
    with pytest.raises(ValueError):
        C.restore_with_opencv_unsharp([img], [np.ones((2, 2))], 6)
    # the reference's early exit needs no device: largest factor 1 -> the input itself
    assert C.restore_downsample_opencv_lanczos(img, np.zeros((2, 2)), 8) is img


def test_c_entry_points_validate_without_gpu(built_lib):
    """The three entry points reject bad arguments before any device work: ELVIS_E_INVALID (-1) + message."""
    from elvis_amd import _lib
    h = _lib.lib()
    p = 16                                               # any non-null pointer: never dereferenced on these paths
    lz, us, tb = h.elvis_classical_lanczos_u8, h.elvis_classical_unsharp_u8, h.elvis_temporal_blend_u8
    assert lz(None, p, p, 1, 16, 16, 3, 8, 2, 2, p, None) == -1 and b"null" in h.elvis_last_error()
    assert lz(p, p, p, 1, 16, 16, 3, 8, 2, 2, None, None) == -1 and b"null" in h.elvis_last_error()
    for block in (1, 6, 64):
        assert lz(p, p, p, 1, 64, 64, 3, block, 64 // block, 64 // block, p, None) == -1
        assert b"power of two" in h.elvis_last_error()
    assert lz(p, p, p, 1, 16, 16, 5, 8, 2, 2, p, None) == -1 and b"channels" in h.elvis_last_error()
    assert lz(p, p, p, 1, 16, 16, 3, 8, 3, 2, p, None) == -1 and b"map must be" in h.elvis_last_error()
    assert lz(p, p, p, 1, 4, 16, 3, 8, 0, 2, p, None) == -1                           # no whole block row
    assert us(p, p, p, 1, 16, 16, 3, 8, 2, 2, 0, p, None, 16, None) == -1 and b"null" in h.elvis_last_error()
    for halo in (-1, 33):
        assert us(p, p, p, 1, 16, 16, 3, 8, 2, 2, halo, p, p, 16, None) == -1 and b"halo" in h.elvis_last_error()
    for max_level in (0, 17):
        assert us(p, p, p, 1, 16, 16, 3, 8, 2, 2, 0, p, p, max_level, None) == -1
        assert b"max_level" in h.elvis_last_error()
    assert us(p, p, p, 1, 16, 16, 3, 32, 2, 2, 0, p, p, 16, None) == -1                # 16 x 16 has no 32-block
    assert tb(None, p, 2, 100, 0.3, 0.7, None) == -1 and b"null" in h.elvis_last_error()
    assert tb(p, p, 0, 100, 0.3, 0.7, None) == -1 and b"bad shape" in h.elvis_last_error()
    assert tb(p, p, 2, 100, 1.5, -0.5, None) == -1 and b"outside" in h.elvis_last_error()
