"""The foreground segmenter, host side (no GPU): its numpy statement (tests/_segment_ref.py) on known pans, histograms,
shares and remainders; the integer bounds of every stage at 3840 x 2160; thirteen mutants of the statement, each told
apart by a case of the device matrix; the scene conditions; the Python argument errors, all before the library is
touched; the C entry points' exports, workspace size and validation."""
import os
import re

import numpy as np
import pytest
import torch

import _segment_ref as R
import elvis_amd
from elvis_amd import _build, _lib, drivers, segment
from elvis_amd.complexity import resize_masks_nearest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"elvis_segment_workspace_bytes": 4, "elvis_segment_foreground_u8": 23}


# ----------------------------------------------------------------------------- the statement itself
@pytest.mark.parametrize("radius", [1, 2, 8])
def test_the_statement_recovers_a_known_pan_exactly(radius):
    side = 4 * (2 * radius + 9)
    for step in ((radius, radius), (-radius, -radius), (radius, -radius), (0, 0), (1, -radius)):
        clip = R.pan_clip(3, side, side + 12, 3, step, seed=5)
        _, det = R.segment(clip, cfg=R.SegmentConfig(radius=radius), details=True)
        assert det["shift"].tolist() == [[-step[0], -step[1]], list(step), list(step)], step
        assert all(det["sad"][e, step[0] + radius, step[1] + radius] == 0 for e in (1, 2))


def test_a_flat_clip_ties_at_zero_shift_and_falls_back_to_ones():
    clip = R.pan_clip(3, 40, 52, 3, None, flat=128)
    out, det = R.segment(clip, cfg=R.SegmentConfig(radius=2), details=True)
    assert not det["sad"].any() and det["shift"].tolist() == [[0, 0]] * 3            # every shift ties: (0, 0) is the least
    assert not det["F"].any() and det["thr"].tolist() == [255] * 3 and not det["pre"].any()
    assert out.shape == (3, 40, 52) and out.dtype == np.uint8 and out.all()           # "no mask": all ones


def test_otsu_on_a_two_level_histogram_picks_the_gap():
    hist = np.zeros(256, np.int64)
    hist[40], hist[200] = 700, 300
    t = R.otsu(hist)
    assert t == 40                                                                    # the first of the equal maxima 40..199
    hist[41] = 5
    assert 40 <= R.otsu(hist) < 200
    one = np.zeros(256, np.int64)
    one[17] = 100
    assert R.otsu(one) == 255                                                         # nothing to split
    f = np.full((10, 10), 30, np.int64)
    f[:3] = 47
    assert R.threshold(f, R.SegmentConfig()) == 255 and R.threshold(f + 1, R.SegmentConfig()) == 31   # min_peak = 48


def test_the_fallback_fires_at_share_zero_and_just_above_max_share_only():
    def mask(count):
        m = np.zeros(100, np.int64)
        m[:count] = 1
        return m.reshape(10, 10)
    assert R.fallback(mask(0), 0.7).all()
    assert np.array_equal(R.fallback(mask(1), 0.7), mask(1))
    assert np.array_equal(R.fallback(mask(70), 0.7), mask(70))                        # exactly max_share: kept
    assert R.fallback(mask(71), 0.7).all()
    assert np.array_equal(R.fallback(mask(100), 1.0), mask(100))
    # 0.7 * 30 is 20.999... in float64: the comparison is in integers
    m = np.zeros(30, np.int64)
    m[:21] = 1
    assert np.array_equal(R.fallback(m.reshape(5, 6), 0.7), m.reshape(5, 6))
    assert R.share_num(0.7) == segment.share_num(0.7) == 7000 and R.SHARE_DEN == segment.SHARE_DEN


def test_the_upsample_replicates_the_remainder_rows_and_columns():
    m = np.arange(6).reshape(2, 3) % 2
    up = R.upsample(m, 11, 14)
    assert up.shape == (11, 14) and up.dtype == np.uint8
    assert np.array_equal(up[:8, :12], np.repeat(np.repeat(m, 4, axis=0), 4, axis=1))
    assert (up[8:] == up[7]).all() and (up[:, 12:] == up[:, 11:12]).all()


def test_the_vote_is_two_of_three_and_the_ends_keep_their_own():
    pre = np.zeros((4, 2, 2), np.int64)
    pre[0, 0, 0] = pre[1, 0, 0] = pre[2, 0, 1] = pre[3, 1, 1] = 1
    pre[1, 1, 0] = 1
    assert np.array_equal(R.vote(pre, 0, 4), pre[0]) and np.array_equal(R.vote(pre, 3, 4), pre[3])
    assert R.vote(pre, 1, 4).tolist() == [[1, 0], [0, 0]] and R.vote(pre, 2, 4).tolist() == [[0, 0], [0, 0]]


def test_value_ranges_at_3840_x_2160():
    """The widths the kernels keep each stage in, from the statement's own extremes."""
    ry, rx, r = 2160 // 4, 3840 // 4, segment.MAX_RADIUS
    white, black = np.full((1, 8, 8, 3), 255, np.uint8), np.zeros((1, 8, 8, 3), np.uint8)
    extremes = np.concatenate([R.yuv(c)[0].reshape(-1, 3) for c in
                               (white, black, white * np.uint8([1, 0, 0]), white * np.uint8([0, 1, 0]), white * np.uint8([0, 0, 1]),
                                white * np.uint8([1, 1, 0]), white * np.uint8([0, 1, 1]), white * np.uint8([1, 0, 1]))])
    assert extremes.min() >= 16 and extremes.max() <= 240
    cell = 16 * 240                                             # red: u16
    assert cell == 3840 and cell < 2 ** 16
    assert 9 * cell < 2 ** 16 and 3 * cell < 2 ** 16            # M and S: u16
    assert 9 * cell * 255 < 2 ** 31 and 3 * cell * 255 < 2 ** 31               # the normalisation's product: int32
    assert 255 * 2 * segment.MAX_WEIGHT < 2 ** 31 and 25 * 255 < 2 ** 31       # the fuse and the 5 x 5 sum
    source = open(os.path.join(ROOT, "elvis_amd", "csrc", "segment.hip")).read()
    ty, tx = (int(re.search(rf"{k} = (\d+)", source).group(1)) for k in ("kSadTileY", "kSadTileX"))
    assert ty * tx * cell < 2 ** 31                             # a tile's SAD: int32
    assert ry * rx * cell < 2 ** 63 and ry * rx * cell >= 2 ** 30              # a frame's SAD: 64-bit, and it needs to be
    bw = max(1, min(ry, rx) // 16)
    assert bw * max(ry, rx) * cell < 2 ** 63                    # a strip's sum
    n = ry * rx                                                 # Otsu: every product of integers is exact in float64
    assert 255 * n * n < 2 ** 53 and n * n < 2 ** 53
    assert n * R.SHARE_DEN < 2 ** 63
    # the extremes through the statement at a small size: a white object on black, moving
    clip = np.zeros((2, 48, 48, 3), np.uint8)
    clip[0, 8:24, 8:24] = 255
    clip[1, 24:40, 24:40] = 255
    _, det = R.segment(clip, cfg=R.SegmentConfig(radius=0), details=True)
    assert det["red"].max() <= cell and det["M"].max() <= 9 * cell and det["S"].max() <= 3 * cell
    assert det["M"].max() == 9 * 16 * (235 - 16)
    for k in ("Mn", "Sn", "F"):
        assert 0 <= det[k].min() and det[k].max() <= 255
    assert det["Mn"].max() == 255 and det["Sn"].max() == 255


# ----------------------------------------------------------------------------- the device matrix can tell
def _zero_padded_box(a, k):
    p = np.pad(a, k, mode="constant")
    return sum(p[i:i + a.shape[0], j:j + a.shape[1]] for i in range(2 * k + 1) for j in range(2 * k + 1))


def _zero_padded_morph(m, dilate):
    p = np.pad(m, 1, mode="constant")
    views = [p[i:i + m.shape[0], j:j + m.shape[1]] for i in range(3) for j in range(3)]
    return np.maximum.reduce(views) if dilate else np.minimum.reduce(views)


def _raster_pick(table, radius):
    i, j = np.unravel_index(np.argmin(table), table.shape)
    return int(i) - radius, int(j) - radius


def _centre_residual(c, o, dy, dx):
    ry, rx = c.shape
    yy, xx = np.mgrid[0:ry, 0:rx]
    inside = (yy + dy >= 0) & (yy + dy < ry) & (xx + dx >= 0) & (xx + dx < rx)
    return np.where(inside, np.abs(c - o[np.clip(yy + dy, 0, ry - 1), np.clip(xx + dx, 0, rx - 1)]), 0)


def _residual_kept_outside(c, o, dy, dx):
    ry, rx = c.shape
    yy, xx = np.mgrid[0:ry, 0:rx]
    return np.minimum.reduce([np.abs(c - o[np.clip(yy + dy + a, 0, ry - 1), np.clip(xx + dx + b, 0, rx - 1)])
                              for a in (-1, 0, 1) for b in (-1, 0, 1)])


def _last_maximum_otsu(hist):
    h = np.asarray(hist, np.float64)
    n, tot = float(h.sum()), float((h * np.arange(256)).sum())
    w0 = s0 = 0.0
    best_v, best_t = -1.0, 255
    for t in range(255):
        w0 += h[t]
        s0 += h[t] * t
        if w0 == 0 or n - w0 == 0:
            continue
        d = tot * w0 - s0 * n
        v = d * d / (w0 * (n - w0))
        if v >= best_v:
            best_v, best_t = v, t
    return best_t


def _rounded_strip_means(red):
    ry, rx, _ = red.shape
    bw = max(1, min(ry, rx) // 16)
    strips = (red[:bw], red[ry - bw:], red[:, :bw], red[:, rx - bw:])
    return np.stack([(2 * s.reshape(-1, 3).sum(axis=0) + s.shape[0] * s.shape[1]) // (2 * s.shape[0] * s.shape[1]) for s in strips])


def _zero_remainder_upsample(mask, h, w):
    up = np.zeros((h, w), np.uint8)
    up[:mask.shape[0] * 4, :mask.shape[1] * 4] = np.repeat(np.repeat(mask, 4, axis=0), 4, axis=1)
    return up


# one clause of the statement changed at a time: (the function replaced, its replacement)
MUTANTS = {
    "ties_go_to_the_first_shift_in_raster_order": ("pick_shift", _raster_pick),
    "the_residual_is_the_centre_difference_alone": ("residual", _centre_residual),
    "the_residual_is_kept_where_the_partner_is_outside": ("residual", _residual_kept_outside),
    "box_sums_pad_with_zero": ("_box", _zero_padded_box),
    "morphology_pads_with_zero": ("_morph", _zero_padded_morph),
    "otsu_takes_the_last_maximum": ("otsu", _last_maximum_otsu),
    "strip_means_are_rounded": ("strip_means", _rounded_strip_means),
    "the_floors_are_ignored": ("normalise", lambda v, floor: np.minimum(255, v * 255 // max(int(v.max()), 1))),
    "min_peak_is_ignored": ("threshold", lambda f, cfg: R.otsu(np.bincount(f.ravel(), minlength=256))),
    "the_vote_needs_all_three": ("vote", lambda pre, e, m: pre[e] if e - 1 < 0 or e + 1 >= m else pre[e - 1] * pre[e] * pre[e + 1]),
    "the_ends_need_their_neighbour": ("vote", lambda pre, e, m: (
        (pre[e - 1] + pre[e] + pre[e + 1] >= 2).astype(np.int64) if 0 < e < m - 1 else pre[e] * pre[1 if e == 0 else e - 1] if m > 1 else pre[e])),
    "a_full_frame_is_kept": ("fallback", lambda mask, share: mask if mask.any() else np.ones_like(mask)),
    "the_remainder_is_background": ("upsample", _zero_remainder_upsample),
}
_CASES = R.cases()
_true = {}


def _run(name):
    frames, order, kw = _CASES[name]
    masks, det = R.segment(frames, order, R.SegmentConfig(**kw), details=True)
    return dict(det, masks=masks)


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_device_matrix_tells_every_mutant_of_the_statement(mutant, monkeypatch):
    """Each mutant gives other bytes - in the masks or in an intermediate the device test compares - on at least one
    case of tests/test_gpu_segment.py: a kernel with that mistake would not pass it."""
    target, replacement = MUTANTS[mutant]
    told = None
    for name in sorted(_CASES):
        if name not in _true:
            _true[name] = _run(name)
        with monkeypatch.context() as mp:
            mp.setattr(R, target, replacement)
            got = _run(name)
        if any(not np.array_equal(got[k], _true[name][k]) for k in got):
            told = name
            break
    assert told is not None, f"no case of the matrix tells the mutant {mutant} from the statement"


# ----------------------------------------------------------------------------- the scene conditions
@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_scene_conditions(name):
    pan, move, noise = R.SCENES[name]
    frames, boxes = R.scene(pan, move, noise)
    assert frames.shape == (6, 240, 320, 3) and all(b[2] - b[0] == 64 and b[3] - b[1] == 96 for b in boxes)
    masks, det = R.segment(frames, details=True)
    assert set(np.unique(masks)) == {0, 1}
    inside_ok, far_ok = R.scene_conditions(masks, boxes)
    assert inside_ok, "a block wholly inside the object is background"
    assert far_ok, "a block two or more blocks away from the object is foreground"
    want = [pan[0] // 4, pan[1] // 4]
    assert det["shift"].tolist() == [[-want[0], -want[1]]] + [want] * 5
    # the block grid of the conditions is the one the pipeline resizes to
    grid = resize_masks_nearest(list(masks), 15, 20)
    assert np.array_equal(np.stack(grid), masks[:, ::16, ::16])


# ----------------------------------------------------------------------------- the Python surface
def test_names_are_exported_and_the_defaults_are_the_statements():
    for name in ("segment_frames", "foreground_masks_device", "save_foreground_masks", "calculate_removability_scores_device",
                 "calculate_removability_scores_from_frames"):
        assert callable(getattr(elvis_amd, name)), name
    assert elvis_amd.SegmentConfig is segment.SegmentConfig
    assert vars(segment.SegmentConfig()) == vars(R.SegmentConfig())
    assert vars(segment.SegmentConfig()) == dict(radius=8, motion_weight=2, spatial_weight=1, motion_floor=864, spatial_floor=384,
                                                 min_peak=48, dilation=1, max_share=0.7, temporal_vote=True)
    assert segment.Q == R.Q == 4
    for doc in (segment.__doc__, segment.segment_frames.__doc__, drivers.calculate_removability_scores_device.__doc__):
        assert "untuned and unmeasured on real video" in " ".join(doc.split()).lower()
    assert "NOT UFO" in segment.__doc__ and "NOT UFO" in segment.segment_frames.__doc__


BAD_CONFIGS = [
    (dict(radius=-1), "radius"), (dict(radius=17), "radius"), (dict(radius=2.0), "radius"), (dict(radius=True), "radius"),
    (dict(dilation=-1), "dilation"), (dict(dilation=5), "dilation"),
    (dict(motion_weight=0), "motion_weight"), (dict(spatial_weight=-2), "spatial_weight"), (dict(spatial_weight=1.5), "spatial_weight"),
    (dict(motion_floor=0), "motion_floor"), (dict(spatial_floor=-1), "spatial_floor"),
    (dict(max_share=0.0), "max_share"), (dict(max_share=1.0001), "max_share"), (dict(max_share=-0.5), "max_share"),
    (dict(max_share="0.5"), "max_share"), (dict(min_peak=256), "min_peak"), (dict(temporal_vote=1), "temporal_vote"),
]


def test_value_errors_fire_before_the_library_is_touched(monkeypatch):
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(segment, "lib", no_lib)
    monkeypatch.setattr(_lib, "lib", no_lib)
    f = torch.zeros((2, 80, 96, 3), dtype=torch.uint8)
    host = np.zeros((2, 80, 96, 3), np.uint8)
    for kw, word in BAD_CONFIGS:
        cfg = segment.SegmentConfig(**kw)
        with pytest.raises(ValueError, match=word):
            segment.foreground_masks_device(f, cfg=cfg)
        with pytest.raises(ValueError, match=word):
            segment.segment_frames(host, cfg=cfg)
        with pytest.raises(ValueError, match=word):
            drivers.calculate_removability_scores_device(host, 16, cfg=cfg)
    with pytest.raises(ValueError, match="SegmentConfig"):
        segment.foreground_masks_device(f, cfg=dict(radius=2))
    for bad, word in ((f.float(), "uint8"), (f[0], "n, H, W, C"), (torch.zeros((2, 80, 96, 2), dtype=torch.uint8), "channels"),
                      (torch.zeros((0, 80, 96, 3), dtype=torch.uint8), "n >= 1"), (host, "uint8 tensor"), (f, "CUDA"),
                      (torch.zeros((2, 80, 192, 3), dtype=torch.uint8)[:, :, ::2], "contiguous")):
        with pytest.raises(ValueError, match=word):
            segment.foreground_masks_device(bad)
    for order in ("RGB", "yuv", None):
        with pytest.raises(ValueError, match="order"):
            segment.foreground_masks_device(f, order)
        with pytest.raises(ValueError, match="order"):
            segment.segment_frames(host, order=order)
    # Ry or Rx below 2 R + 1, in words that name the setting
    for shape in ((2, 67, 96, 3), (2, 96, 64, 3)):                                   # 16 x 24 and 24 x 16 at 1/4: R = 8 needs 17
        with pytest.raises(ValueError, match="radius"):
            segment.foreground_masks_device(torch.zeros(shape, dtype=torch.uint8))
        with pytest.raises(ValueError, match="radius"):
            segment.segment_frames(np.zeros(shape, np.uint8))
    with pytest.raises(ValueError, match="CUDA"):                                    # 17 x 17 is enough: the next check
        segment.foreground_masks_device(torch.zeros((1, 68, 71, 1), dtype=torch.uint8))
    with pytest.raises(ValueError, match="CUDA"):
        segment.foreground_masks_device(torch.zeros((1, 4, 4, 1), dtype=torch.uint8), cfg=segment.SegmentConfig(radius=0))
    with pytest.raises(ValueError, match="frame"):
        segment.foreground_masks_device(torch.zeros((1, 3, 40, 1), dtype=torch.uint8), cfg=segment.SegmentConfig(radius=0))
    for bad in (np.zeros((2, 80, 96, 3), np.float32), np.zeros((2, 80, 96, 4), np.uint8), np.zeros((80, 96), np.uint8)):
        with pytest.raises(ValueError, match="frames"):
            segment.segment_frames(bad)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="chunk_frames"):
            segment.segment_frames(host, chunk_frames=bad)
    assert segment.segment_frames(np.zeros((0, 80, 96, 3), np.uint8)).shape == (0, 80, 96)
    with pytest.raises(ValueError, match="masks"):
        segment.save_foreground_masks(np.zeros((4, 4), np.uint8), "nowhere")
    with pytest.raises(ValueError, match="masks"):
        segment.save_foreground_masks(np.zeros((1, 4, 4), np.float32), "nowhere")
    assert not os.path.exists("nowhere")


def test_mask_files_are_gray_0_255_pngs_numbered_from_one(tmp_path):
    from PIL import Image
    masks = (np.arange(2 * 5 * 7).reshape(2, 5, 7) % 3 == 0).astype(np.uint8)
    segment.save_foreground_masks(masks, tmp_path / "ufo" / "masks")
    segment.save_foreground_masks(masks.astype(bool), tmp_path / "again")
    assert sorted(os.listdir(tmp_path / "ufo" / "masks")) == ["00001.png", "00002.png"]
    for d in (tmp_path / "ufo" / "masks", tmp_path / "again"):
        for i in range(2):
            with Image.open(d / f"{i + 1:05d}.png") as im:
                assert im.mode == "L" and np.array_equal(np.asarray(im), masks[i] * 255)


# ----------------------------------------------------------------------------- the built library
def test_library_exports_the_entries_and_the_tables_agree(built_lib):
    h = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "elvis_amd.h")).read(), flags=re.S)
    for name, nargs in ENTRIES.items():
        assert hasattr(h, name), f"{name} is not exported"
        assert len(_lib.SIGNATURES[name]) == nargs
        decl = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
        assert decl and len([a for a in decl.group(1).split(",") if a.strip()]) == nargs, name
    assert "segment.hip" in _build.SOURCES
    source = open(os.path.join(ROOT, "elvis_amd", "csrc", "segment.hip")).read()
    for const, value in (("kQ", segment.Q), ("kShareDen", segment.SHARE_DEN), ("kMaxRadius", segment.MAX_RADIUS),
                         ("kMaxDilation", segment.MAX_DILATION), ("kMaxWeight", segment.MAX_WEIGHT), ("kMaxSide", segment.MAX_SIDE),
                         ("kMaxFrames", segment.MAX_FRAMES)):
        assert re.search(rf"\b{const} = {value}\b", source), const


def test_workspace_size_is_the_modules_layout(built_lib):
    h = _lib.lib()
    for m, hh, ww, r in ((1, 20, 20, 2), (3, 21, 23, 2), (5, 72, 130, 8), (33, 1080, 1920, 8), (2, 2160, 3840, 16), (1, 4, 4, 0)):
        lay = segment.workspace_layout(m, hh, ww, r)
        assert h.elvis_segment_workspace_bytes(m, hh, ww, r) == lay["total"] > 0
        offs = [v for k, v in lay.items() if k != "total"]
        assert offs == sorted(offs) and all(o % 256 == 0 for o in offs)
    for bad in ((0, 20, 20, 2), (1, 19, 20, 2), (1, 20, 19, 2), (1, 20, 20, 3), (1, 20, 20, -1), (1, 200, 200, 17), (4097, 20, 20, 2),
                (1, 3, 40, 0), (1, 16388, 40, 0)):
        assert h.elvis_segment_workspace_bytes(*bad) == 0, bad


def test_the_entry_point_refuses_bad_arguments_on_a_host_without_a_gpu(built_lib):
    h = _lib.lib()
    F, B, A, M, W = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000        # never dereferenced: every call is refused
    ok = dict(frames=F, before=None, nb=0, after=None, na=0, masks=M, ws=W, ws_bytes=1 << 30, n=2, h=40, w=48, c=3, bgr=0, radius=2,
              wm=2, wsp=1, mf=864, sf=384, peak=48, dil=1, share=7000, vote=1, stream=None)

    def bad(word, **kw):
        rc = h.elvis_segment_foreground_u8(*dict(ok, **kw).values())
        assert rc == -1 and word in h.elvis_last_error(), (kw, rc, h.elvis_last_error())
    bad(b"null", frames=None)
    bad(b"null", masks=None)
    bad(b"null", ws=None)
    bad(b"channels", c=2)
    bad(b"channels", c=4)
    bad(b"frames", n=0)
    bad(b"before", nb=3, before=B)
    bad(b"after", na=2, after=A)
    bad(b"null halo", nb=1)
    bad(b"null halo", na=1)
    bad(b"radius", radius=17)
    bad(b"radius", radius=-1)
    bad(b"radius", radius=5)                                                # 10 x 12 at 1/4: 2 R + 1 = 11 does not fit
    bad(b"limits", h=3)
    bad(b"limits", w=16388)
    bad(b"dilation", dil=5)
    bad(b"dilation", dil=-1)
    bad(b"weights", wm=0)
    bad(b"weights", wsp=1025)
    bad(b"floors", mf=0)
    bad(b"floors", sf=-3)
    bad(b"min_peak", peak=256)
    bad(b"max_share", share=0)
    bad(b"max_share", share=10001)
    need = h.elvis_segment_workspace_bytes(2, 40, 48, 2)
    bad(b"workspace", ws_bytes=need - 1)
    bad(b"workspace", ws_bytes=-1)
    bad(b"aligned", ws=W + 4)
    bad(b"workspace", nb=2, before=B, na=1, after=A, ws_bytes=need)         # five frames need more than two
