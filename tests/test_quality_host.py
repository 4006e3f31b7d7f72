"""The quality report without a GPU: tests/_quality_ref.py against the reference-code golden (tests/golden/quality.npz,
tools/make_quality_golden.py), its two filter forms against each other, and the host side of elvis_amd.metrics."""
import os

import numpy as np
import pytest

import _quality_ref as Q
from elvis_amd import _lib, metrics


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "quality.npz"))


def test_masked_ssim_reproduces_reference_records(g):
    ref, dec, masks, names = g["ssim_ref"], g["ssim_dec"], g["ssim_masks"].astype(bool), list(g["ssim_mask_names"])
    values, wins = g["ssim_values"], g["ssim_wins"]
    for i, name in enumerate(names):
        got = Q.masked_ssim(ref, dec, masks[i])
        y0, y1, x0, x1 = Q.mask_bbox(masks[i])
        if wins[i] == 0:                                    # an early return of the reference
            assert got == values[i] == 1.0, name
            assert not masks[i].any() or min(y1 - y0, x1 - x0) < 3
        else:
            assert abs(got - values[i]) <= 1e-12, name
            assert Q.win_size_for(y1 - y0, x1 - x0) == wins[i], name
            assert abs(Q.masked_ssim_taps(ref, dec, masks[i]) - values[i]) <= 1e-12, name
    assert abs(Q.masked_ssim(ref, dec, None) - values[len(names)]) <= 1e-12
    assert Q.masked_ssim(ref, ref, masks[names.index("blob")]) == values[len(names) + 1] == 1.0
    y0, _, x0, _ = Q.mask_bbox(masks[names.index("blob")])
    assert y0 % 2 == 1 and x0 % 2 == 1                      # the offset blob's box starts at odd coordinates
    assert 0.0 < values[names.index("full")] < 0.999


def test_masks_and_boxes_reproduce_reference_records(g):
    ref, masks = g["ssim_ref"], g["ssim_masks"].astype(bool)
    for i in range(len(masks)):
        assert np.array_equal(Q.apply_binary_mask(ref, masks[i]), g["applied"][i])
        assert np.array_equal(Q.apply_binary_mask(ref, masks[i], invert=True), g["applied_inv"][i])
    h, w = ref.shape[:2]
    for ids, ratio, box in zip(g["union_lists"], g["union_ratios"], g["union_boxes"]):
        ms = [None if i == -1 else masks[i] for i in ids if i != -2]
        assert Q.compute_mask_union_bbox(ms, w, h, float(ratio)) == tuple(box)
    assert tuple(g["union_boxes"][1]) == (0, 0, w, h)       # the empty union is the whole frame
    assert g["union_boxes"][8][0] == 0                      # padding clipped at the frame's left edge


def test_fg_bg_ssim_reproduces_reference_records(g):
    maps = list(g["fgbg_maps"])
    for fn in (Q.compute_fg_bg_ssim, metrics.compute_fg_bg_ssim):
        for k in ("same", "resize", "fewer", "all_fg", "all_bg"):
            assert fn(maps, g[f"fgbg_mask_{k}"], 0.5) == pytest.approx(tuple(g[f"fgbg_out_{k}"]), abs=1e-12), k
        assert fn(maps, g["fgbg_mask_same"], 0.8) == pytest.approx(tuple(g["fgbg_out_thr"]), abs=1e-12)
        assert fn([], g["fgbg_mask_same"]) == tuple(g["fgbg_out_nomaps"]) == (0.0, 0.0, 0.0)
        overall, fg, bg = fn(maps, g["fgbg_mask_all_bg"])
        assert fg == overall == bg                          # no foreground block: it takes the overall mean


def test_evaluator_reproduces_reference_records(g):
    refs, decs, fg = list(g["eval_refs"]), list(g["eval_decs"]), list(g["eval_fg"].astype(bool))
    h, w = refs[0].shape[:2]
    bbox = Q.compute_mask_union_bbox(fg, w, h)
    assert bbox == tuple(g["eval_bbox"]) and Q.roi_of_bbox(bbox, w, h) == tuple(g["eval_roi"])
    for stride, want in zip(g["eval_strides"], g["eval_results"]):
        got = Q.flatten_result(Q.evaluate_fg_bg_metrics(refs, decs, fg, int(stride)))
        assert np.abs(got - want).max() <= 1e-12
    assert not fg[2].any() and g["eval_results"][0][0][0] > g["eval_results"][0][1][0]   # FG PSNR above BG PSNR


def test_frame_index_rule(g):
    for (count, stride), row in zip(g["index_pairs"], g["index_rows"]):
        want = [int(i) for i in row if i >= 0]
        assert Q.frame_indices(int(count), int(stride)) == want
        assert metrics.metric_frame_indices(int(count), int(stride)) == want
    assert metrics.metric_frame_indices(7, 3) == [0, 3, 6] and metrics.metric_frame_indices(7, 4) == [0, 4, 6]


@pytest.mark.parametrize("shape", [(3, 3), (3, 4), (5, 9), (6, 6), (4, 17), (26, 31)])
def test_tap_filter_matches_scipy(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    x = rng.integers(0, 256, shape).astype(np.float64)
    for v in (x, x * x):
        assert np.abs(Q.filter_taps(v, Q.gaussian_taps()) - Q.filter_scipy(v)).max() <= 1e-12 * max(1.0, np.abs(v).max())
    assert np.array_equal(Q.gaussian_taps(), metrics.gaussian_window())
    assert np.array_equal(Q.msssim_taps(), metrics.ssim_window().astype(np.float64))


def test_msssim_matches_block_ssim_oracle():
    from oracle import glue_ref
    rng = np.random.default_rng(7)
    for b in (8, 12, 16):
        f1 = rng.integers(0, 256, (b, b, 3), dtype=np.uint8)
        f2 = np.clip(f1.astype(int) + rng.integers(-15, 16, f1.shape), 0, 255).astype(np.uint8)
        want = glue_ref.block_ssim(f1, f2, b)[0, 0]         # float32 output of float64 arithmetic
        assert np.float32(Q.msssim_ssim(f1, f2)) == pytest.approx(want, rel=2 ** -23, abs=0)


def test_luma_rule():
    px = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [13, 200, 77]]], np.uint8)
    assert Q.luma_bgr(px).tolist() == [[255, 0, 29, 150, 76, round(0.114 * 13 + 0.587 * 200 + 0.299 * 77)]]


def test_value_errors_come_before_the_device_check():
    f3, f1 = np.zeros((8, 9, 3), np.uint8), np.zeros((8, 9, 1), np.uint8)
    m = np.ones((8, 9), bool)
    with pytest.raises(ValueError):
        metrics.masked_ssim(f3, np.zeros((8, 10, 3), np.uint8), device="cpu")
    with pytest.raises(ValueError):
        metrics.masked_ssim(f1, f1, device="cpu")                       # luma needs 3 channels
    with pytest.raises(ValueError):
        metrics.masked_ssim(f3, f3, np.ones((9, 8), bool), device="cpu")
    with pytest.raises(ValueError):
        metrics.calculate_ssim([f3], [np.zeros((9, 9, 3), np.uint8)], device="cpu")
    with pytest.raises(ValueError):
        metrics.apply_binary_mask(f3, np.ones((4, 4), bool), device="cpu")
    with pytest.raises(ValueError):
        metrics.compute_mask_union_bbox([np.ones((4, 4), bool)], 9, 8, device="cpu")
    with pytest.raises(ValueError):
        metrics.evaluate_fg_bg_metrics([f3, f3], [f3, f3], [m, np.ones((4, 4), bool)], device="cpu")
    with pytest.raises(ValueError):
        metrics.evaluate_fg_bg_metrics([f1], [f1], [m], device="cpu")
    with pytest.raises(ValueError):
        metrics.calculate_foreground_metric([f3], [f3], [np.ones(4)], metrics.calculate_psnr, device="cpu")
    # well-formed input on a non-GPU device: the house RuntimeError
    for call in (lambda: metrics.masked_ssim(f3, f3, m, device="cpu"), lambda: metrics.calculate_ssim([f3], [f3], device="cpu"),
                 lambda: metrics.apply_binary_mask(f3, m, device="cpu"), lambda: metrics.compute_mask_union_bbox([m], 9, 8, device="cpu"),
                 lambda: metrics.evaluate_fg_bg_metrics([f3], [f3], [m], device="cpu")):
        with pytest.raises(RuntimeError):
            call()
    # what needs no device answers without one
    assert metrics.calculate_ssim([], [], device="cpu") == []
    assert metrics.compute_mask_union_bbox([], 9, 8, device="cpu") == (0, 0, 9, 8)
    assert metrics.calculate_foreground_metric([f3], [f3], [np.zeros((2, 3))], metrics.calculate_psnr, device="cpu") == []
    assert metrics.apply_binary_mask(f3, None, device="cpu") is f3


def test_abi_symbols_and_workspace_query(built_lib):
    h = _lib.lib()
    for name in ("elvis_mask_bbox_u8", "elvis_apply_mask_u8", "elvis_ssim_mean_f64", "elvis_ssim_workspace_bytes"):
        assert hasattr(h, name) and name in _lib.SIGNATURES
    assert h.elvis_ssim_workspace_bytes(1, 1080, 1920, 3) == 3 * 68 * 60 * 8       # one float64 per 16 x 32 tile and channel
    assert h.elvis_ssim_workspace_bytes(2, 37, 53, 1) == 2 * 3 * 2 * 8
    assert h.elvis_ssim_workspace_bytes(0, 8, 8, 3) == 0
    # arguments are validated before the device is touched
    assert h.elvis_ssim_mean_f64(16, 16, None, None, 16, 16, 16, 1, 8, 8, 4, _lib.SSIM_LUMA, _lib.SSIM_REFLECT, 1.0, 1.0, 1.0, 0, 1.0, None) == -1
    assert b"3-channel" in h.elvis_last_error()
    assert h.elvis_ssim_mean_f64(16, 16, None, None, 16, 16, 16, 1, 8, 8, 5, _lib.SSIM_CHANNELS, _lib.SSIM_VALID, 1.0, 1.0, 1.0, 0, 1.0, None) == -1
    assert h.elvis_ssim_mean_f64(16, 16, None, None, 16, None, 16, 1, 8, 8, 3, 0, 0, 1.0, 1.0, 1.0, 0, 1.0, None) == -1
    assert h.elvis_mask_bbox_u8(None, None, 1, 8, 8, None) == -1
    assert h.elvis_apply_mask_u8(16, 16, 16, 1, 0, 8, 3, 0, None) == -1
