"""Presley's adaptive degraders, host side (no GPU needed): the taps and the INTER_AREA table against their quoted values,
properties of the numpy restatement the GPU is pinned to (tests/_presley_degrade_ref.py), the map rules and the
per-block control flow against the reference's own code (tests/golden/presley_degrade.npz), the Python error paths and
the C entry points' argument checks."""
import os

import numpy as np
import pytest

import _presley_degrade_ref as R
from elvis_amd import classical as C
from elvis_amd import degrade as D
from oracle import degrade_ref, glue_ref


def _rng_blocks(seed, n, b, c=3):
    return np.random.default_rng(seed).integers(0, 256, size=(n, b, b, c), dtype=np.uint8)


# ----------------------------------------------------------------------------- tables
def test_taps():
    assert C.gaussian_taps_u8(1.0, 5).tolist() == [14, 62, 104, 62, 14] == list(R.TAPS)
    assert C.gaussian_taps_u8(1).tolist() == C.gaussian_taps_u8(1.0, 7).tolist() == [1, 14, 62, 102, 62, 14, 1]
    with pytest.raises(ValueError):
        C.gaussian_taps_u8(1.0, 4)


def test_area_table_16_to_5():
    for tab in (D.area_table(16, 5), R.area_entries(16, 5)):
        assert len(tab) == 20
        assert [(d, s, float(w)) for d, s, w in tab[:5]] == [(0, 0, .3125), (0, 1, .3125), (0, 2, .3125), (0, 3, .0625), (1, 3, .25)]
        assert all(isinstance(w, np.float32) for _, _, w in tab)


@pytest.mark.parametrize("b", range(2, 33))
def test_area_tables_every_target(b):
    starts, src, wgt = D.area_tables(b)
    hb = b // 2
    assert starts.shape == (hb + 1, hb + 2) and starts.dtype == np.int32 and src.dtype == np.int32 and wgt.dtype == np.float32
    for d in range(1, hb + 1):
        tab = R.area_entries(b, d)
        assert D.area_table(b, d) == tab and len(tab) <= 2 * b
        assert starts[d, d] - starts[d, 0] == len(tab)
        for i in range(d):
            lo, hi = starts[d, i], starts[d, i + 1]
            assert [(i, int(s), w) for s, w in zip(src[lo:hi], wgt[lo:hi])] == [t for t in tab if t[0] == i]
            assert hi > lo and 0 <= src[lo:hi].min() and src[lo:hi].max() < b
            assert abs(float(np.sum(wgt[lo:hi], dtype=np.float64)) - 1.0) <= 2.0 ** -20


# ----------------------------------------------------------------------------- the restatement's own properties
@pytest.mark.parametrize("value", [0, 1, 127, 254, 255])
def test_flat_blocks_stay_flat(value):
    for b in (2, 3, 5, 8, 12, 16, 20, 32):
        flat = np.full((1, b, b, 3), value, np.uint8)
        for d in range(1, b // 2 + 1):
            small = R.resize_area_u8(flat, d)
            assert (small == value).all(), (b, d)
            assert (R.resize_linear_u8(small, b) == value).all(), (b, d)
        blurred = flat
        for _ in range(3):
            blurred = R.gaussian_pass_u8(blurred)
        assert (blurred == value).all(), b


@pytest.mark.parametrize("b,d", [(16, 5), (16, 3), (32, 10), (32, 6), (8, 3)])
def test_general_area_is_the_overlap_mean(b, d):
    """Within 0.5 (the uint8 rounding) + 1e-3 (float32 rounding of at most about 20 terms of at most 255 per sum) of the
    float64 mean over the fractional overlap."""
    blocks = _rng_blocks(b * 100 + d, 1000, b, 1)
    edges = np.arange(d + 1) * (b / d)
    m = np.zeros((d, b))
    for i in range(d):
        for s in range(b):
            m[i, s] = max(0.0, min(edges[i + 1], s + 1) - max(edges[i], s))
    m /= m.sum(axis=1, keepdims=True)
    exact = np.einsum("ir,nrqc,jq->nijc", m, blocks.astype(np.float64), m)
    got = R.resize_area_u8(blocks, d).astype(np.float64)
    assert np.abs(got - exact).max() <= 0.5 + 1e-3


@pytest.mark.parametrize("b,d", [(16, 8), (16, 4), (16, 1), (12, 6), (12, 4), (12, 2), (20, 5), (32, 16), (32, 2), (6, 3), (2, 1)])
def test_whole_ratio_area_is_the_integer_rule(b, d):
    blocks = _rng_blocks(b * 100 + d, 8, b)
    for blk in blocks:
        assert np.array_equal(R.resize_area_u8(blk, d), glue_ref.area_downscale_u8(blk, b // d))


@pytest.mark.parametrize("b", [2, 4, 8, 16])
def test_power_of_two_scales_are_the_elvis_filter(b):
    blocks = _rng_blocks(b, 4, b)
    for level in range(1, 5):
        for blk in blocks:
            assert np.array_equal(R.downscale_block(blk, 1 << level), degrade_ref._downsample_block(blk, level)), (b, level)


@pytest.mark.parametrize("b", [2, 3, 5, 8, 16])
def test_blur_pass_commutes_with_flips_and_transpose(b):
    x = _rng_blocks(b, 6, b)
    y = R.gaussian_pass_u8(x)
    assert np.array_equal(R.gaussian_pass_u8(x[:, :, ::-1]), y[:, :, ::-1])
    assert np.array_equal(R.gaussian_pass_u8(x[:, ::-1]), y[:, ::-1])
    assert np.array_equal(R.gaussian_pass_u8(x.transpose(0, 2, 1, 3)), y.transpose(0, 2, 1, 3))


def test_blur_pass_is_the_separable_fixed_point_pass():
    """The closed form against cv2's two passes: u8 x tap in u16, u16 x tap in u32, (acc + 0x8000) >> 16."""
    for b in (2, 3, 7, 16):
        x = _rng_blocks(b + 50, 5, b).astype(np.int64)
        idx = np.array([[R.reflect101(i + k - 2, b) for k in range(5)] for i in range(b)])
        t = np.array(R.TAPS, np.int64)
        hp = (x[:, :, idx, :] * t[None, None, None, :, None]).sum(axis=3)
        assert hp.max() <= 255 * 256
        acc = (hp[:, idx, :, :] * t[None, None, :, None, None]).sum(axis=2)
        assert np.array_equal(((acc + 0x8000) >> 16).astype(np.uint8), R.gaussian_pass_u8(x.astype(np.uint8)))


def test_clip_forms_are_the_block_loops():
    rng = np.random.default_rng(7)
    frames = rng.integers(0, 256, size=(2, 43, 59, 3), dtype=np.uint8)
    for b in (8, 16, 12):
        grid = (2, 43 // b, 59 // b)
        scales = rng.integers(-1, b + 2, size=grid).astype(np.int32)
        rounds = rng.integers(-1, 5, size=grid).astype(np.int32)
        down = R.scale_clip(frames, scales, b)
        blur = R.blur_clip(frames, rounds, b)
        for f in range(2):
            assert np.array_equal(down[f], R.degrade_frame(frames[f], scales[f], b, R.downscale_block))
            assert np.array_equal(blur[f], R.degrade_frame(frames[f], rounds[f], b, R.blur_block))
        assert np.array_equal(down[:, grid[1] * b:], frames[:, grid[1] * b:]) and np.array_equal(blur[:, :, grid[2] * b:], frames[:, :, grid[2] * b:])


# ----------------------------------------------------------------------------- against the reference's own code
@pytest.fixture(scope="module")
def golden(golden_dir):
    return R.golden_cases(os.path.join(golden_dir, "presley_degrade.npz"))


def test_golden_covers_the_edges(golden):
    cases, kernels = golden
    assert kernels == {(5.0, 5.0, 1.0)}
    assert {c["family"] for c in cases} == {"utils_downsample", "utils_blur", "presley_downsample", "presley_blur"}
    assert {c["importance"].dtype for c in cases} == {np.dtype(np.float32), np.dtype(np.float64)}
    for c in cases:
        imp, mx = c["importance"], c["max_value"]
        assert (imp == 0).any() and (imp == 1).any()
        scaled = (1 - imp) * mx                                   # in the array's own dtype, as the reference computes it
        assert scaled.dtype == imp.dtype and (scaled == np.floor(scaled)).sum() >= 3 and (scaled - np.floor(scaled) == 0.5).any()


def test_map_rules_reproduce_the_reference(golden):
    for c in golden[0]:
        imp, mx = c["importance"], c["max_value"]
        if c["family"] == "utils_downsample":
            for fn in (D._scale_map, lambda i, m: R.degrade_adaptive_downsample(np.zeros(_frame_shape(c), np.uint8), i, c["block"], m)[1]):
                got = fn(imp, mx)
                assert got.dtype == np.int32 and np.array_equal(got, c["map"])
        else:
            for fn in (D.generate_degradation_map, R.generate_degradation_map):
                got = fn(imp, mx)
                assert got.dtype == np.int32 and np.array_equal(got, c["map"])
        # an up-cast would move bin edges: the float32 cases hold values for which it does
    moved = [c for c in golden[0] if c["importance"].dtype == np.float32
             and not np.array_equal(D.generate_degradation_map(c["importance"].astype(np.float64), c["max_value"]),
                                    D.generate_degradation_map(c["importance"], c["max_value"]))]
    assert moved


def _frame_shape(c):
    by, bx = c["importance"].shape
    return by * c["block"] + c["extra"][0], bx * c["block"] + c["extra"][1], 3


def test_control_flow_reproduces_the_reference(golden, monkeypatch):
    for c in golden[0]:
        by, bx = c["importance"].shape
        b, mx = c["block"], c["max_value"]
        frame = R.id_frame(*_frame_shape(c)[:2], b)
        rec = R.Recorder(by, bx)
        monkeypatch.setattr(R, "cv", rec)
        if c["family"] == "utils_downsample":
            out, _ = R.degrade_adaptive_downsample(frame, c["importance"], b, mx)
        elif c["family"] == "utils_blur":
            out, _ = R.degrade_adaptive_blur(frame, c["importance"], b, mx)
        else:
            method = R.downscale_block if c["family"] == "presley_downsample" else R.blur_block
            out = R.degrade_video_adaptive([frame], [c["importance"]], b, mx, method)[0][0]
        assert np.array_equal(rec.resizes, c["resizes"]) and np.array_equal(rec.blurs, c["blurs"]), c["family"]
        assert np.array_equal(rec.sizes[..., 0], c["size0"]) and np.array_equal(rec.sizes[..., 1], c["size1"])
        assert np.array_equal(rec.flags[..., 0], c["flag0"]) and np.array_equal(rec.flags[..., 1], c["flag1"])
        assert rec.kernels <= {(5, 5, 1.0)}
        touched = np.repeat(np.repeat(c["touched"] > 0, b, 0), b, 1)
        assert not out[:by * b, :bx * b][touched].any() and np.array_equal(out[:by * b, :bx * b][~touched], frame[:by * b, :bx * b][~touched])
        assert np.array_equal(out[by * b:], frame[by * b:]) and np.array_equal(out[:, bx * b:], frame[:, bx * b:])
        # what the kernels take from the map: a downscale target of max(1, b // scale) (scale 1: the same size, a copy),
        # `map` blur calls
        if "downsample" in c["family"]:
            assert np.array_equal(c["size0"], np.where(c["map"] > 0, np.maximum(1, b // np.maximum(c["map"], 1)), 0))
            assert np.array_equal(c["size1"], np.where(c["map"] > 0, b, 0))
            assert set(np.unique(c["flag0"])) <= {-1, R.INTER_AREA} and set(np.unique(c["flag1"])) <= {-1, R.INTER_LINEAR}
        else:
            assert np.array_equal(c["blurs"], np.maximum(c["map"], 0))


# ----------------------------------------------------------------------------- error paths that need no GPU
def test_python_errors_before_any_launch():
    frame = np.zeros((32, 48, 3), np.uint8)
    imp = np.zeros((2, 3))
    with pytest.raises(ValueError, match="method"):
        D.degrade_frame(frame, np.zeros((2, 3), np.int32), 16, lambda blk, lv: blk)
    with pytest.raises(ValueError, match="method"):
        D.degrade_video_adaptive([frame], [imp], 16, 4, R.downscale_block)
    for fn in (D.degrade_adaptive_downsample, D.degrade_adaptive_blur):
        with pytest.raises(ValueError, match="block grid"):
            fn(frame, np.zeros((3, 2)), 16)
        with pytest.raises(ValueError, match="uint8"):
            fn(frame.astype(np.float32), imp, 16)
        for b in (1, 33):
            with pytest.raises(ValueError, match="block_size"):
                fn(frame, np.zeros((32 // b, 48 // b)), b)
    with pytest.raises(ValueError, match="rounds"):
        D.degrade_adaptive_blur(frame, imp, 16, max_rounds=65)
    with pytest.raises(ValueError, match="rounds"):
        D.blur_block(np.zeros((8, 8, 3), np.uint8), 65)
    with pytest.raises(ValueError, match="scale"):
        D.downscale_block(np.zeros((8, 8, 3), np.uint8), 0)
    with pytest.raises(ValueError, match="arithmetic"):
        D.filter_frame_gaussian(frame, imp, 16, arithmetic="float64")
    blk = np.zeros((8, 8, 3), np.uint8)
    assert D.blur_block(blk, 0) is blk
    assert D.degrade_video_adaptive([], [], 16, 4, D.blur_block) == ([], [])


def test_c_entry_points_check_their_arguments(built_lib):
    from elvis_amd._lib import lib
    L = lib()
    p = 4096                                    # never dereferenced: every call below fails its checks first
    ok = dict(n=1, h=35, w=37, c=3, b=16, by=2, bx=2)

    def scale(**kw):
        a = {**ok, **kw}
        return L.elvis_degrade_scale_u8(a.get("src", p), p, p, a["n"], a["h"], a["w"], a["c"], a["b"], a["by"], a["bx"],
                                        a.get("tab", p), p, p, a.get("tab_len", 8), None)

    def blur(**kw):
        a = {**ok, **kw}
        t = a.get("taps", (14, 62, 104))
        return L.elvis_degrade_gaussian_fx_u8(a.get("src", p), p, p, a["n"], a["h"], a["w"], a["c"], a["b"], a["by"], a["bx"],
                                              t[0], t[1], t[2], None)

    for fn in (scale, blur):
        for bad in (dict(src=None), dict(n=0), dict(c=0), dict(c=5), dict(b=1), dict(b=33), dict(by=3), dict(bx=1),
                    dict(h=15, by=0), dict(w=8, bx=0)):
            assert fn(**bad) == -1, bad
            assert L.elvis_last_error()
    assert scale(tab=None) == -1 and scale(tab_len=0) == -1
    assert blur(taps=(14, 62, 103)) == -1 and blur(taps=(-1, 77, 104)) == -1
