"""The quality report on the device (csrc/quality.hip) against tests/_quality_ref.py and the reference-code golden.

SSIM bar, abs <= 1e-9: a float64 moment is 22 products summed, under 25 ulp or 3e-15 relative on values up to 65 025,
so about 2e-10 absolute on a variance; the denominators are at least C1 C2 and the (vx + vy + C2) factor at least 58.5,
so S moves by less than 1e-11 and so does its mean; 1e-9 leaves two orders for the order of summation.  The same holds
for the [0, 1]-scaled whole-frame form.  PSNR / MSE bars are those of tests/test_gpu_metrics.py.
"""
import os

import numpy as np
import pytest

import _quality_ref as Q

pytestmark = pytest.mark.gpu

BAR = 1e-9


def _pair(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    base = np.stack([100 + 75 * np.sin(yy / 5.0 + c) * np.cos(xx / 7.0 - c) for c in range(3)], axis=-1)
    ref = np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
    dec = np.clip(ref.astype(np.float64) + rng.normal(0, 9, ref.shape), 0, 255).astype(np.uint8)
    return ref, dec


def _masks(h, w):
    """full, offset blob (box from odd coordinates), 3x4 / 5x9 / 6x6 boxes (win_size 3, 5, 5: repeated reflection under
    the radius-5 window), a 2x40 strip and an empty mask (1.0), a mask touching all four edges, a ring."""
    yy, xx = np.mgrid[:h, :w]
    m = {k: np.zeros((h, w), bool) for k in ("full", "blob", "box3x4", "box5x9", "box6x6", "strip2x40", "empty", "edges", "ring")}
    m["full"][:] = True
    m["blob"] = ((yy - h // 2 + 1) ** 2 + (xx - w // 2 + 1) ** 2) < (min(h, w) // 3) ** 2
    m["blob"][:(h // 4) | 1] = False                      # cut the disc at an odd row
    m["box3x4"][5:8, 7:11] = True
    m["box5x9"][11:16, 3:12] = True
    m["box5x9"][13, 5] = False
    m["box6x6"][20:26, 30:36] = True
    m["strip2x40"][30:32, 5:45] = True
    m["edges"][0, 10] = m["edges"][h - 1, 20] = m["edges"][15, 0] = m["edges"][18, w - 1] = True
    m["edges"][10:20, 10:30] = True
    m["ring"][:] = True
    m["ring"][3:h - 3, 3:w - 3] = False
    return m


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "quality.npz"))


@pytest.mark.parametrize("h,w", [(37, 53), (70, 130)])
def test_masked_ssim_matches_reference(gpu_device, h, w):
    from elvis_amd import metrics
    ref, dec = _pair(h, w, h)
    masks = _masks(h, w)
    y0, _, x0, _ = Q.mask_bbox(masks["blob"])
    assert y0 & 1
    keep = ref.copy(), dec.copy(), {k: v.copy() for k, v in masks.items()}
    for name, m in masks.items():
        want = Q.masked_ssim_taps(ref, dec, m)
        got = metrics.masked_ssim(ref, dec, m, gpu_device)
        print(f"{h}x{w} {name}: device {got!r} reference {want!r} diff {abs(got - want):.3e}")
        assert abs(got - want) <= BAR, name
        if name in ("strip2x40", "empty"):
            assert got == 1.0
        assert metrics.masked_ssim(ref, ref, m, gpu_device) == 1.0, name            # identical inputs: exactly 1
    want = Q.masked_ssim_taps(ref, dec, None)
    assert abs(metrics.masked_ssim(ref, dec, device=gpu_device) - want) <= BAR
    assert abs(want - Q.masked_ssim(ref, dec, None)) <= 1e-12                        # the scipy form agrees
    assert np.array_equal(ref, keep[0]) and np.array_equal(dec, keep[1]) and all(np.array_equal(masks[k], keep[2][k]) for k in masks)


def test_masked_ssim_does_not_depend_on_the_batch(gpu_device):
    import torch
    from elvis_amd import metrics
    from elvis_amd.recompose import frames_to_device
    pairs = [_pair(70, 130, s) for s in (1, 2, 3)]
    ms = _masks(70, 130)
    masks = [ms["blob"], ms["box5x9"], ms["edges"]]
    a, b = frames_to_device([p[0] for p in pairs], gpu_device), frames_to_device([p[1] for p in pairs], gpu_device)
    m = metrics.masks_to_device(masks, (70, 130), gpu_device)
    boxes = metrics.mask_bbox_device(m).cpu().numpy()
    assert [tuple(r) for r in boxes] == [Q.mask_bbox(k) for k in masks] and len({tuple(r) for r in boxes}) == 3
    batch = metrics.masked_ssim_device(a, b, m).cpu().numpy()
    assert batch.dtype == np.float64 and batch.shape == (3,)
    for i in range(3):
        alone = float(metrics.masked_ssim_device(a[i:i + 1].contiguous(), b[i:i + 1].contiguous(), m[i:i + 1].contiguous()).cpu()[0])
        assert batch[i] == alone                                                       # bit for bit
        assert abs(batch[i] - Q.masked_ssim_taps(pairs[i][0], pairs[i][1], masks[i])) <= BAR
    again = metrics.masked_ssim_device(a, b, m).cpu().numpy()
    assert np.array_equal(batch, again)                                                # deterministic
    assert torch.equal(metrics.mask_bbox_device(torch.zeros_like(m)).cpu(), torch.zeros((3, 4), dtype=torch.int32))


@pytest.mark.parametrize("border", ["reflect", "valid"])
@pytest.mark.parametrize("source", ["luma", "channels"])
def test_ssim_kernel_contract_every_instantiation(gpu_device, source, border):
    """elvis_ssim_mean_f64 with explicit scalars, a rectangle and a mask, for each (source, border) pair."""
    import torch
    from elvis_amd import _lib, metrics
    from elvis_amd.recompose import frames_to_device
    ref, dec = _pair(37, 53, 11)
    mask = _masks(37, 53)["ring"]
    rect = (2, 35, 1, 50)
    w = Q.gaussian_taps()
    C1, C2, cov, pad, scale = 0.4, 2.5, 49 / 48, 2, 3.0
    out = metrics.ssim_mean_device(frames_to_device([ref], gpu_device), frames_to_device([dec], gpu_device), w,
                                   source=_lib.SSIM_LUMA if source == "luma" else _lib.SSIM_CHANNELS,
                                   border=_lib.SSIM_REFLECT if border == "reflect" else _lib.SSIM_VALID, C1=C1, C2=C2, cov_norm=cov, pad=pad,
                                   scale=scale, masks=metrics.masks_to_device([mask], (37, 53), gpu_device),
                                   rects=torch.tensor([rect], dtype=torch.int32, device=gpu_device)).cpu().numpy()
    y0, y1, x0, x1 = rect
    mc = mask[y0:y1, x0:x1]
    if source == "luma":
        planes = [(Q.luma_bgr(ref)[y0:y1, x0:x1] * mc, Q.luma_bgr(dec)[y0:y1, x0:x1] * mc)]
    else:
        planes = [(ref[y0:y1, x0:x1, c] * mc / scale, dec[y0:y1, x0:x1, c] * mc / scale) for c in range(3)]
    want = [Q.ssim_mean(x, y, w, border, C1, C2, cov, pad) for x, y in planes]
    assert out.shape == (1, len(want)) and np.abs(out[0] - want).max() <= BAR
    assert f"ssim_tile_kernel<{source},{border}>" == _lib.lib().elvis_last_launch().decode()


@pytest.mark.parametrize("shape", [(40, 56, 3), (9, 40, 3), (11, 11, 3)])
def test_calculate_ssim_matches_reference(gpu_device, shape):
    from elvis_amd import metrics
    rng = np.random.default_rng(shape[0])
    f1 = [rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(2)]
    f2 = [np.clip(f.astype(int) + rng.integers(-20, 21, shape), 0, 255).astype(np.uint8) for f in f1]
    got = metrics.calculate_ssim(f1, f2, device=gpu_device)                            # a 2-frame list
    assert isinstance(got, list) and len(got) == 2 and all(isinstance(v, float) for v in got)
    for x, y, v in zip(f1, f2, got):
        want = Q.msssim_ssim(x, y)
        print(f"{shape}: device {v!r} reference {want!r}")
        assert abs(v - want) <= BAR
    assert metrics.calculate_ssim(f1[:1], f2[:1], device=gpu_device) == got[:1]
    assert metrics.calculate_ssim(f1[:1], f1[:1], device=gpu_device) == [1.0]
    assert abs(metrics.calculate_ssim(f1[:1], f2[:1], 200.0, gpu_device)[0] - Q.msssim_ssim(f1[0], f2[0], 200.0)) <= BAR
    assert metrics.calculate_ssim([], [], device=gpu_device) == []


def test_boxes_and_masks_match_reference_records(gpu_device, g):
    import torch
    from elvis_amd import metrics
    ref, masks = g["ssim_ref"], g["ssim_masks"].astype(bool)
    h, w = ref.shape[:2]
    boxes = metrics.mask_bbox_device(torch.from_numpy(g["ssim_masks"]).to(gpu_device)).cpu().numpy()
    assert [tuple(b) for b in boxes] == [Q.mask_bbox(m) for m in masks]
    for i in range(len(masks)):
        assert np.array_equal(metrics.apply_binary_mask(ref, masks[i], device=gpu_device), g["applied"][i])
        assert np.array_equal(metrics.apply_binary_mask(ref, masks[i], True, gpu_device), g["applied_inv"][i])
    for ids, ratio, box in zip(g["union_lists"], g["union_ratios"], g["union_boxes"]):
        ms = [None if i == -1 else masks[i] for i in ids if i != -2]
        assert metrics.compute_mask_union_bbox(ms, w, h, float(ratio), gpu_device) == tuple(box)
    # the vector path (16 pixels a thread) with its byte tail, for 1, 3 and 4 channels, and the byte-wise kernel for 2
    rng = np.random.default_rng(5)
    m = torch.from_numpy((rng.random((2, 33, 47)) < 0.5).astype(np.uint8)).to(gpu_device)
    for c in (1, 2, 3, 4):
        f = torch.from_numpy(rng.integers(1, 256, (2, 33, 47, c), dtype=np.uint8)).to(gpu_device)
        for invert in (False, True):
            keep = (m != 0) != invert
            assert torch.equal(metrics.apply_mask_device(f, m, invert), f * keep[..., None])


def test_foreground_metric_matches_reference(gpu_device):
    from elvis_amd import metrics
    pairs = [_pair(48, 64, s) for s in (21, 22, 23)]
    refs, decs = [p[0] for p in pairs], [p[1] for p in pairs]
    rng = np.random.default_rng(9)
    grids = [np.where(rng.random((6, 8)) < 0.2, 0.9, 0.1), np.zeros((6, 8)), np.full((5, 7), 0.49)]   # frame 1: no foreground
    grids[2][1:4, 2:6] = 0.5                                                            # a 5 x 7 grid on 48 x 64: uneven rows
    for own, ref_fn, tol in ((metrics.calculate_psnr, Q.calculate_psnr, 1e-4), (metrics.calculate_mse, Q.calculate_mse, None),
                             (metrics.calculate_ssim, Q.calculate_ssim, BAR)):
        got = metrics.calculate_foreground_metric(refs, decs, grids, own, device=gpu_device)
        want = Q.calculate_foreground_metric(refs, decs, grids, ref_fn)
        assert len(got) == len(want) == 2                                               # the empty frame is skipped
        assert got == pytest.approx(want, **({"rel": 1e-6} if tol is None else {"abs": tol}))


def test_evaluator_matches_reference_records(gpu_device, g):
    from elvis_amd import _lib, metrics
    refs, decs, fg = list(g["eval_refs"]), list(g["eval_decs"]), list(g["eval_fg"].astype(bool))
    assert len(refs) == 7 and refs[0].shape == (48, 64, 3) and not fg[2].any()
    for stride, want in zip(g["eval_strides"], g["eval_results"]):
        got = metrics.evaluate_fg_bg_metrics(refs, decs, fg, int(stride), gpu_device)
        assert set(got) == set(Q.REGIONS) and all(set(v) == set(Q.KEYS) for v in got.values())
        for r, region in enumerate(Q.REGIONS):
            for k, key in enumerate(Q.KEYS):
                v, ref_v = got[region][key], want[r][k]
                print(f"stride {stride} {region} {key}: device {v!r} reference {ref_v!r}")
                if key.startswith("psnr"):
                    assert abs(v - ref_v) <= 1e-5
                elif key.startswith("mse"):
                    assert v == pytest.approx(ref_v, rel=1e-6, abs=1e-9)
                else:
                    assert abs(v - ref_v) <= BAR
    metrics.masked_ssim(refs[0], decs[0], fg[0], gpu_device)
    assert _lib.lib().elvis_last_launch() == b"ssim_tile_kernel<luma,reflect>"


def test_fullsize_frame(gpu_device):
    """1080 x 1920: 64-bit indexing, the tile grid's limits and the wide staging path on a real frame."""
    from elvis_amd import metrics
    rng = np.random.default_rng(1080)
    h, w = 1080, 1920
    yy, xx = np.mgrid[:h, :w]
    base = np.stack([120 + 90 * np.sin(yy / 37.0 + c) * np.cos(xx / 53.0 - c) for c in range(3)], axis=-1)
    ref = np.clip(base + rng.normal(0, 4, base.shape), 0, 255).astype(np.uint8)
    dec = np.clip(ref.astype(np.int16) + rng.integers(-9, 10, ref.shape), 0, 255).astype(np.uint8)
    mask = ((yy - 611) ** 2 * 3 + (xx - 905) ** 2) < 500 ** 2
    got, want = metrics.masked_ssim(ref, dec, mask, gpu_device), Q.masked_ssim(ref, dec, mask)
    print(f"1080p blob: device {got!r} reference {want!r}")
    assert abs(got - want) <= BAR
    got, want = metrics.calculate_ssim([ref], [dec], device=gpu_device)[0], Q.msssim_ssim(ref, dec)
    print(f"1080p whole frame: device {got!r} reference {want!r}")
    assert abs(got - want) <= BAR
