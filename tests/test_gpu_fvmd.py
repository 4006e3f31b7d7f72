"""FVMD on the device against the numpy float64 statement of its contract (tests/_fvmd_ref.py), stage by stage.

Bound: the project's 1e-9 * max(1, |value|) for the pyramid, the tracks, the feature rows, the Gram outputs and the
singular values; for the distance 1e-9 * max(1, tr S1 + tr S2 + |dmu|^2), since its terms cancel.  It rests on the fixed
evaluation order: every product, sum and branch of the tracker is the statement's own (the window sums included), so
only atan2 and the order of the Gram sums differ.  Worst seen on an MI355X: pyramid 0 and tracks 0 (the same bytes), rows
5.8e-15, Gram 3.4e-13 (d = 2176), singular values against numpy's SVD 1.8e-14, distance 5e-16 of its scale.  A miss is
first a sign of reassociation or a contracted FMA."""
import numpy as np
import pytest
import torch

import _fvmd_ref as R
from elvis_amd import fvmd, metrics, vmaf

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)                        # a copy: the shared fixtures are read-only


def _report(name, got, want, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    denom = np.maximum(1.0, np.abs(want)) if scale is None else max(1.0, scale)
    worst = float((np.abs(got - want) / denom).max()) if got.size else 0.0
    print(f"{name}: worst |device - statement| / scale = {worst:.3g} (bar {R.BAR:g})")
    return worst


@pytest.mark.parametrize("name", [n for n in R.CLIPS if not n.startswith("static")])
def test_pyramid_tracks_and_rows_against_the_statement(gpu_device, name):
    want = R.tracked(name)
    kind, frames, h, w, seq_len, step = R.CLIPS[name]
    assert R.margins_clear(want["margins"]), "the fixture must keep lambda_min / 225 a factor 10 from the threshold"
    if kind == "half":
        assert (want["margins"] == 0.0).sum() == want["margins"].size // 2       # the black half: G = 0 exactly
    cfg = fvmd.FvmdConfig(segment_step=step)
    luma = _dev(want["clip"], gpu_device)
    lvl1, lvl2 = fvmd.pyramid_device(luma)
    assert _report(f"{name} pyramid 1", lvl1.cpu().numpy(), want["pyramid"][0]) <= R.BAR
    assert _report(f"{name} pyramid 2", lvl2.cpu().numpy(), want["pyramid"][1]) <= R.BAR
    tracks = fvmd.track_keypoints_device(luma, seq_len, cfg)
    b = R.segments(frames, seq_len, step)
    assert tracks.shape == (b, seq_len, 400, 2) and tracks.dtype == torch.float64 and b in (2, 3)
    got = tracks.cpu().numpy()
    assert _report(f"{name} tracks", got, want["tracks"]) <= R.BAR
    if kind == "half":                                                          # a masked region does not move, exactly
        still = got.reshape(b, seq_len, 20, 20, 2)[:, :, :, :10]
        assert (still == still[:, :1]).all()
    if kind == "fast":                                                          # the clamps were reached
        assert (got[..., 0] == w - 1.0).any() and (got[..., 1] == h - 1.0).any()
    rows = fvmd.motion_features_device(tracks)
    assert rows.shape == (b, fvmd.feature_length(seq_len))
    assert _report(f"{name} rows", rows.cpu().numpy(), want["rows"]) <= R.BAR
    assert _report(f"{name} rows of the device's tracks", rows.cpu().numpy(), R.features(got)) <= R.BAR
    assert torch.equal(fvmd.track_keypoints_device(luma, seq_len, cfg), tracks)                  # two runs: the same bytes


@pytest.mark.parametrize("h,w,seq_len,frames", [(64, 64, 10, 11), (67, 81, 16, 18)])
def test_a_static_clip_does_not_move(gpu_device, h, w, seq_len, frames):
    name = {64: "static_64", 67: "static_67x81"}[h]
    want = R.tracked(name)
    cfg = fvmd.FvmdConfig(segment_step=R.CLIPS[name][5])
    tracks = fvmd.track_keypoints_device(_dev(want["clip"], gpu_device), seq_len, cfg)
    assert np.array_equal(tracks.cpu().numpy(), want["tracks"])                                   # d = 0, exactly
    assert (fvmd.motion_features_device(tracks) == 0.0).all()


@pytest.mark.parametrize("ref,dec", R.PAIRS, ids=lambda n: n)
def test_distance_stages_against_the_statement(gpu_device, ref, dec):
    want = R.expected_distance(ref, dec)
    a, b = _dev(R.tracked(ref)["rows"], gpu_device), _dev(R.tracked(dec)["rows"], gpu_device)
    gram, scalars = fvmd.gram_device(a, b)
    assert _report(f"{ref} x {dec} gram", gram.cpu().numpy(), want["gram"]) <= R.BAR
    assert _report(f"{ref} x {dec} scalars", scalars.cpu().numpy(), want["scalars"]) <= R.BAR
    sv = np.sort(fvmd.singular_values_device(gram).cpu().numpy())[::-1]
    k = min(gram.shape)
    assert _report(f"{ref} x {dec} singular values", sv[:k], want["sv"]) <= R.BAR and np.abs(sv[k:]).max(initial=0.0) <= R.BAR * max(1.0, sv[0])
    got = fvmd.frechet_distance_device(a, b)
    assert _report(f"{ref} x {dec} distance", got, want["fd"], scale=want["scale"]) <= R.BAR
    back = fvmd.frechet_distance_device(b, a)
    assert abs(back - want["fd"]) <= R.BAR * max(1.0, want["scale"])
    same = fvmd.frechet_distance_device(a, a)
    assert abs(same) <= R.BAR * max(1.0, R.fd_scale(R.tracked(ref)["rows"], R.tracked(ref)["rows"]))


def test_gram_and_distance_on_full_rank_rows(gpu_device):
    """n and m past one tile and not multiples of it, d not a multiple of the panel: every ragged edge of the product."""
    rng = np.random.default_rng(21)
    for n, m, d in ((2, 2, 1), (17, 35, 50), (40, 33, 2176)):
        a, b = rng.normal(0, 3, (n, d)) + rng.normal(0, 1, d), rng.normal(0, 2, (m, d))
        gram, scalars = fvmd.gram_device(_dev(a, gpu_device), _dev(b, gpu_device))
        want_gram, want_scalars = R.gram_parts(a, b)
        assert _report(f"gram {n}x{m}x{d}", gram.cpu().numpy(), want_gram) <= R.BAR
        assert _report(f"scalars {n}x{m}x{d}", scalars.cpu().numpy(), want_scalars) <= R.BAR
        got = fvmd.frechet_distance_device(_dev(a, gpu_device), _dev(b, gpu_device))
        assert _report(f"distance {n}x{m}x{d}", got, R.frechet(a, b), scale=R.fd_scale(a, b)) <= R.BAR


@pytest.mark.parametrize("n", [2, 3, 33, 130])
def test_jacobi_against_numpy(gpu_device, n):
    """2 and 3: the smallest even and odd counts; 33: odd, one idle vector per round, in LDS; 130: past the in-LDS form
    (130 * 130 > 16384), one launch per pairing round."""
    rng = np.random.default_rng(n)
    mat = rng.normal(0, 1, (n, n)) * rng.uniform(0.1, 10.0, (1, n))
    got = np.sort(fvmd.singular_values_device(_dev(mat, gpu_device)).cpu().numpy())[::-1]
    want = np.linalg.svd(mat, compute_uv=False)
    assert _report(f"jacobi {n}", got, want) <= R.BAR


def test_jacobi_rank_deficient_and_rectangular(gpu_device):
    rng = np.random.default_rng(5)
    low = rng.normal(0, 1, (24, 3)) @ rng.normal(0, 1, (3, 24))                               # rank 3 of 24
    low[7] = 0.0                                                                               # and a zero vector
    for mat in (low, rng.normal(0, 1, (5, 40)), rng.normal(0, 1, (100, 300)), np.zeros((4, 4))):
        got = np.sort(fvmd.singular_values_device(_dev(mat, gpu_device)).cpu().numpy())[::-1]
        want = np.linalg.svd(mat, compute_uv=False)
        assert _report(f"jacobi {mat.shape}", got[:len(want)], want) <= R.BAR
        assert np.isfinite(got).all()


def test_whole_clip_once_equals_each_prefix_afresh(gpu_device):
    clip = _dev(R.clip("pan", 24, 64, 64), gpu_device)
    for step in (1, 2):
        cfg = fvmd.FvmdConfig(segment_step=step)
        whole = fvmd.motion_features_device(fvmd.track_keypoints_device(clip, 16, cfg))
        for count in (17, 20, 23):
            part = fvmd.motion_features_device(fvmd.track_keypoints_device(clip[:count].contiguous(), 16, cfg))
            assert part.shape[0] == R.segments(count, 16, step) and torch.equal(part, whole[:part.shape[0]])


def _masked_clip():
    h, w, n = 64, 96, 24
    ref = np.stack([np.stack([p, np.roll(p, 2, axis=1), 255 - p], axis=-1) for p in R.clip("pan", n, h, w)])
    dec = np.stack([np.stack([p, np.roll(p, 2, axis=1), 255 - p], axis=-1) for p in R.clip("decoded", n, h, w)])
    masks = np.zeros((n, h, w), np.uint8)
    masks[:, :, 10:80] = 255
    return np.ascontiguousarray(ref), np.ascontiguousarray(dec), masks


def test_calculate_fvmd_is_fvmd_device_on_one_window(gpu_device):
    ref, dec, _ = _masked_clip()
    luma_r, luma_d = vmaf.luma_device(_dev(ref, gpu_device), "bgr"), vmaf.luma_device(_dev(dec, gpu_device), "bgr")
    want = fvmd.fvmd_device(luma_r, luma_d)
    assert np.isfinite(want) and want > 0
    value, std = fvmd.calculate_fvmd(list(ref), list(dec), verbose=False, device=gpu_device)
    assert (value, std) == (want, 0.0)
    assert fvmd.calculate_fvmd_device(luma_r, luma_d) == (want, 0.0)
    # two prefixes (17 and 24 frames), scored over the rows of one tracking pass
    value2, _ = fvmd.calculate_fvmd_device(luma_r, luma_d, early_stop_window=17)
    assert value2 == want
    stopped, _ = fvmd.calculate_fvmd_device(luma_r, luma_d, early_stop_window=17, early_stop_delta=1e9)
    assert stopped == want                                                    # the early stop fires at the second prefix, the last
    first, _ = fvmd.calculate_fvmd_device(luma_r[:17].contiguous(), luma_d[:17].contiguous())
    assert first == fvmd.fvmd_device(luma_r[:17].contiguous(), luma_d[:17].contiguous()) != want
    with pytest.raises(RuntimeError, match="even with stride=1"):
        fvmd.calculate_fvmd(list(ref[:16]), list(dec[:16]), verbose=False, device=gpu_device)   # one segment: no distance


def test_evaluate_fg_bg_metrics_gains_the_fvmd_keys(gpu_device):
    ref, dec, masks = _masked_clip()
    refs, decs, fg = list(ref), list(dec), list(masks)
    plain = metrics.evaluate_fg_bg_metrics(refs, decs, fg, device=gpu_device)
    got = metrics.evaluate_fg_bg_metrics(refs, decs, fg, device=gpu_device, fvmd=True)
    h, w = ref.shape[1:3]
    bx, by, bw, bh = metrics.compute_mask_union_bbox(fg, w, h, device=gpu_device)
    roi = (by, min(h, by + bh), bx, min(w, bx + bw))
    assert roi[3] - roi[2] >= 64 and (roi[1] - roi[0], roi[3] - roi[2]) != (h, w)
    ref_d, dec_d, m_d = _dev(ref, gpu_device), _dev(dec, gpu_device), _dev(masks, gpu_device)
    for region, invert, rect in (("foreground", False, roi), ("background", True, None)):
        assert set(got[region]) == set(plain[region]) | {"fvmd", "fvmd_std"}
        assert all(repr(got[region][k]) == repr(plain[region][k]) for k in plain[region])         # the other keys: the same bytes
        want = fvmd.fvmd_device(vmaf.luma_device(ref_d, "bgr", masks=m_d, invert=invert, rect=rect),
                                vmaf.luma_device(dec_d, "bgr", masks=m_d, invert=invert, rect=rect))
        print(region, got[region]["fvmd"], got[region]["fvmd_std"])
        assert np.isfinite(got[region]["fvmd"]) and np.isfinite(got[region]["fvmd_std"])
        assert got[region]["fvmd"] == want and got[region]["fvmd_std"] == 0.0
    same = metrics.evaluate_fg_bg_metrics(refs, decs, fg, device=gpu_device, fvmd=fvmd.FvmdConfig())
    assert same == got
    short = metrics.evaluate_fg_bg_metrics(refs[:9], decs[:9], fg[:9], device=gpu_device, fvmd=True)
    for region in ("foreground", "background"):
        assert np.isnan(short[region]["fvmd"]) and np.isnan(short[region]["fvmd_std"])
    strided = metrics.evaluate_fg_bg_metrics(refs, decs, fg, metric_stride=3, device=gpu_device, fvmd=True)      # 9 frames sampled
    assert np.isnan(strided["foreground"]["fvmd"]) and np.isnan(strided["background"]["fvmd_std"])
