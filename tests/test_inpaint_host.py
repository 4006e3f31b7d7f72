"""The wavefront Telea inpainter, host side (no GPU): the properties of its numpy statement (tests/_inpaint_ref.py) and
its mutants; the Python argument errors; the C entry points' exports and validation; the directory driver with a
stand-in device step."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _inpaint_hooks
import _inpaint_ref as R
import _shrink_ref as S
import elvis_amd
from elvis_amd import _build, _lib, drivers, frameio, inpaint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"elvis_inpaint_workspace_bytes": 3, "elvis_inpaint_prepare": 7, "elvis_inpaint_fill": 9}


# ----------------------------------------------------------------------------- the numpy statement
@pytest.fixture(scope="module")
def blocks30():
    rng = np.random.default_rng(0)
    img = R.make_image(96, 128, 3, seed=1)
    mask = R.expand_block_mask(rng.random((1, 6, 8)) < 0.3, 16, 96, 128)
    stats = {}
    return img[None], mask, R.inpaint(img[None], mask, stats=stats), stats


def test_known_pixels_are_unchanged_and_the_holes_are_filled_better_than_by_a_mean(blocks30):
    frames, mask, out, stats = blocks30
    hole = mask != 0
    assert np.array_equal(out[~hole], frames[~hole])
    assert stats["waves"] >= 8 and stats["min_s"] > 0

    def mse(a):
        return float(((a.astype(np.float64) - frames.astype(np.float64))[hole] ** 2).mean())
    mean_fill = frames.copy()
    mean_fill[hole] = frames[~hole].mean(axis=0).astype(np.uint8)
    assert mse(out) < 0.5 * mse(mean_fill)


def test_a_constant_image_is_reproduced_exactly():
    for value in (0, 1, 77, 254, 255):
        for name, (frames, masks) in R.cases().items():
            if name in ("interior_b8_c3", "corners", "odd_random60", "mixed_clip"):
                const = np.full_like(frames, value)
                assert np.array_equal(R.inpaint(const, masks), const), (name, value)


def test_one_known_pixel_gives_every_pixel_its_value():
    frames, masks = R.cases()["deep_63_waves"]
    stats = {}
    out = R.inpaint(frames, masks, stats=stats)
    assert stats["waves"] == 63
    assert (out == frames[0, 0, 0]).all()


def test_the_bytes_under_the_hole_change_nothing():
    for name in ("merged_2_3_L", "odd_random60", "mixed_clip"):
        frames, masks = R.cases()[name]
        a, b = frames.copy(), frames.copy()
        a[masks != 0] = 0xA5
        b[masks != 0] = 0x5A
        fillable = [i for i in range(len(masks)) if not masks[i].all()]          # a frame without a known pixel stays as it is
        assert np.array_equal(R.inpaint(a, masks)[fillable], R.inpaint(b, masks)[fillable]), name


def test_special_frames_come_back_as_they_are():
    frames, masks = R.cases()["mixed_clip"]
    out = R.inpaint(frames, masks)
    assert not masks[0].any() and masks[1].all()
    assert np.array_equal(out[0], frames[0]) and np.array_equal(out[1], frames[1])
    assert not np.array_equal(out[2], frames[2])


def test_waves_equal_the_integer_rule_and_the_distance_is_exact():
    rng = np.random.default_rng(3)
    hole = rng.random((23, 31)) < 0.9
    hole[5:17, 4:20] = True
    known = np.argwhere(~hole)
    d2 = R.squared_distance(~hole)
    for y, x in np.argwhere(hole):
        assert d2[y, x] == ((known - (y, x)) ** 2).sum(axis=1).min()
    T, wave = R.level_set(hole)
    for y, x in np.argwhere(hole):
        k = int(wave[y, x])
        assert k >= 1 and k * k >= d2[y, x] > (k - 1) * (k - 1)
        assert T[y, x] == np.sqrt(np.float32(d2[y, x]))
    assert (wave[~hole] == 0).all() and T.dtype == np.float32
    ring = ~hole & (R.known_side_d2(hole) == 1)
    assert ring.any() and (T[ring] == 0).all() and (T[~hole] <= 0).all()
    big = np.arange(0, 3_000_000, 7919, dtype=np.int64)
    k = R.wave_index(np.concatenate([big, big * big, big * big + 1]))
    assert k.min() == 0


def test_the_small_dir_branch_is_exercised():
    frames, masks = R.cases()["odd_random60"]
    stats = {}
    R.inpaint(frames, masks, stats=stats)
    assert stats["waves"] == 3 and stats["min_s"] < 1e-5


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_every_mutant_gives_other_bytes_on_its_case(mutant):
    frames, masks = R.mutant_cases()[R.MUTANTS[mutant]]
    true = R.inpaint(frames, masks)
    got = R.inpaint(frames, masks, mutant=mutant)
    assert got.shape == true.shape and not np.array_equal(got, true)
    assert np.array_equal(got[masks == 0], true[masks == 0])


def test_the_case_list_covers_the_matrix():
    cases = R.cases()
    assert {f.shape[3] for f, _ in cases.values()} == {1, 3}
    prep = R.preparation_cases()
    assert set(prep) < set(cases) and all(np.array_equal(cases[k][0], prep[k][0]) and np.array_equal(cases[k][1], prep[k][1]) for k in prep)
    assert all(f.dtype == m.dtype == np.uint8 and m.shape == f.shape[:3] for f, m in cases.values())
    assert all(f.shape[1] <= 96 and f.shape[2] <= 128 for k, (f, m) in cases.items() if k not in prep)
    assert all(f.shape[1] <= 300 and f.shape[2] <= 513 and f.shape[1] * f.shape[2] <= 130 * 125 for f, m in prep.values())
    assert set(np.unique(cases["mask_values_1_2_255"][1])) == {0, 1, 2, 255}
    for name in ("corners", "edges"):
        m = cases[name][1][0] != 0
        assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any()
    assert all(cases["corners"][1][0][y, x] for y in (0, -1) for x in (0, -1))


# ----------------------------------------------------------------------------- the Python surface
def test_names_are_exported():
    for name in ("inpaint_device", "inpaint_blocks_device", "inpaint_with_opencv", "inpaint_frame",
                 "stretch_and_inpaint_device", "restore_shrunk_frames"):
        assert callable(getattr(elvis_amd, name)), name


def test_value_errors_need_no_gpu():
    f = torch.zeros((2, 16, 24, 3), dtype=torch.uint8)
    m = torch.zeros((2, 16, 24), dtype=torch.uint8)
    bad = [
        (f.float(), m, None, "uint8"),                                   # dtype of the frames
        (f, m.bool(), None, "masks must be"),                            # dtype of the masks
        (f, m[:, :, :23], None, "do not match"),                         # shape
        (f[0], m, None, "uint8"),                                        # rank
        (torch.zeros((2, 16, 24, 4), dtype=torch.uint8), m, None, "channels"),
        (torch.zeros((2, 16, 24, 2), dtype=torch.uint8), m, None, "channels"),
        (f, m, torch.zeros((2, 16, 24, 6), dtype=torch.uint8)[..., ::2], "contiguous"),
        (f, m, torch.zeros((2, 16, 25, 3), dtype=torch.uint8), "out must be"),
        (f, m, None, "CUDA"),                                            # device: host tensors
    ]
    for frames, masks, out, msg in bad:
        with pytest.raises(ValueError, match=msg):
            inpaint.inpaint_device(frames, masks, out=out)
    with pytest.raises(ValueError, match="do not match"):
        inpaint.inpaint_blocks_device(f, m, 8)
    with pytest.raises(ValueError, match="block_size"):
        inpaint.inpaint_blocks_device(f, torch.zeros((2, 2, 3), dtype=torch.uint8), 0)
    with pytest.raises(ValueError, match="CUDA"):
        inpaint.inpaint_blocks_device(f, torch.zeros((2, 2, 3), dtype=torch.bool), 8)
    frame, mask = np.zeros((16, 24, 3), np.uint8), np.zeros((16, 24), np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        inpaint.inpaint_frame(frame.astype(np.float32), mask)
    with pytest.raises(ValueError, match="mask"):
        inpaint.inpaint_frame(frame, mask[:, :20])
    with pytest.raises(ValueError, match="mask"):
        inpaint.inpaint_frame(frame, mask.astype(bool))
    with pytest.raises(ValueError, match="frames"):
        inpaint.inpaint_with_opencv(np.zeros((2, 16, 24, 3), np.float32), np.zeros((2, 2, 3), bool))
    with pytest.raises(ValueError, match="masks"):
        inpaint.inpaint_with_opencv(np.zeros((2, 16, 24, 3), np.uint8), np.zeros((3, 2, 3), bool))
    with pytest.raises(ValueError, match="whole square blocks"):
        inpaint.inpaint_with_opencv(np.zeros((2, 16, 24, 3), np.uint8), np.zeros((2, 2, 4), bool))


# ----------------------------------------------------------------------------- the built library
def test_library_exports_the_entries_and_the_tables_agree(built_lib):
    h = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "elvis_amd.h")).read(), flags=re.S)
    for name, nargs in ENTRIES.items():
        assert hasattr(h, name), f"{name} is not exported"
        assert len(_lib.SIGNATURES[name]) == nargs
        decl = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
        assert decl and len([a for a in decl.group(1).split(",") if a.strip()]) == nargs, name
    assert h.elvis_inpaint_workspace_bytes.restype is C.c_size_t
    assert "inpaint.hip" in _build.SOURCES


def test_workspace_size_and_argument_errors(built_lib):
    h = _lib.lib()

    def bad(rc, word):
        assert rc == -1 and word in h.elvis_last_error(), (rc, h.elvis_last_error())
    n, hh, ww = 3, 37, 53
    npix = n * hh * ww
    size = h.elvis_inpaint_workspace_bytes(n, hh, ww)
    assert size % 256 == 0 and size >= 10 * npix + 4 * (3 * (hh + ww + 2) + 1)      # T f32, wave u16, list int32, header
    assert size < 10 * npix + 4 * (3 * (hh + ww + 2) + 1) + 4 * 256
    assert h.elvis_inpaint_workspace_bytes(0, 8, 8) == 0 and h.elvis_inpaint_workspace_bytes(1, 40000, 8) == 0
    assert h.elvis_inpaint_workspace_bytes(1 << 20, 64, 64) == 0                   # n * h * w >= 2^31
    bad(h.elvis_inpaint_prepare(None, 0, 256, 1, 8, 8, None), b"null")
    bad(h.elvis_inpaint_prepare(256, 0, None, 1, 8, 8, None), b"null")
    bad(h.elvis_inpaint_prepare(256, 0, 256, 0, 8, 8, None), b"bad shape")
    bad(h.elvis_inpaint_prepare(256, 0, 256, 1, 8, 40000, None), b"bad shape")
    bad(h.elvis_inpaint_prepare(256, -1, 256, 1, 8, 8, None), b"block_size")
    bad(h.elvis_inpaint_prepare(256, 0, 264, 1, 8, 8, None), b"aligned")
    counts = (C.c_int32 * 4)(0, 5, 3, 0)
    at = C.addressof(counts)
    bad(h.elvis_inpaint_fill(None, 256, 1, 8, 8, 3, at, 3, None), b"null")
    bad(h.elvis_inpaint_fill(256, 256, 1, 8, 8, 3, None, 3, None), b"null")
    bad(h.elvis_inpaint_fill(256, 256, 1, 8, 8, 2, at, 3, None), b"channels")
    bad(h.elvis_inpaint_fill(256, 256, 1, 0, 8, 3, at, 3, None), b"bad shape")
    bad(h.elvis_inpaint_fill(256, 256, 1, 8, 8, 3, at, 0, None), b"wave counts")
    bad(h.elvis_inpaint_fill(256, 256, 1, 8, 8, 3, at, 19, None), b"wave counts")
    bad(h.elvis_inpaint_fill(256, 256, 1, 2, 2, 3, at, 3, None), b"not those of this clip")     # 8 pixels listed of 4
    counts[1] = -1
    bad(h.elvis_inpaint_fill(256, 256, 1, 8, 8, 3, at, 3, None), b"negative")
    counts[0], counts[1] = 1, 1
    bad(h.elvis_inpaint_fill(256, 256, 1, 8, 8, 3, at, 3, None), b"not those of this clip")
    counts[0] = 0
    assert h.elvis_inpaint_fill(256, 256, 1, 8, 8, 3, at, 1, None) == 0                          # no wave: no launch


# ----------------------------------------------------------------------------- the driver
def _write_shrunk_clip(tmp_path, n=5, by=3, bx=4, b=8, k=1, seed=0):
    rng = np.random.default_rng(seed)
    d = tmp_path / "frames"
    d.mkdir()
    masks = np.zeros((n, by, bx), np.uint8)
    shrunk = []
    for i in range(n):
        for r in range(by):
            masks[i, r, rng.choice(bx, k, replace=False)] = 1
        f = R.make_image(by * b, (bx - k) * b, 3, seed=seed + i)
        frameio.save_frame(f, d / f"{i + 1:05d}.png")
        shrunk.append(f)
    frameio.save_block_masks(masks, tmp_path / "shrink_masks_8.npz")
    return d, tmp_path / "shrink_masks_8.npz", masks, shrunk


def test_driver_names_directories_and_errors(tmp_path):
    from PIL import Image
    d, npz, masks, shrunk = _write_shrunk_clip(tmp_path)
    out, st, full, blk = (tmp_path / s for s in ("inpainted", "stretched", "full", "blk"))
    names = [f"{i + 1:05d}.png" for i in range(len(shrunk))]
    # a missing frame: ValueError before anything is written
    os.rename(d / names[-1], tmp_path / "aside.png")
    with pytest.raises(ValueError, match="No frame 00005.png"):
        drivers.restore_shrunk_frames(str(d), str(npz), 8, str(out), str(st), str(full), str(blk), devices=["cpu"],
                                      _shard_fn=_inpaint_hooks.restore_on_host)
    os.rename(tmp_path / "aside.png", d / names[-1])
    with pytest.raises(ValueError, match="does not hold"):
        drivers.restore_shrunk_frames(str(d), str(npz), 4, str(out), str(st), str(full), str(blk), devices=["cpu"],
                                      _shard_fn=_inpaint_hooks.restore_on_host)
    assert not any(p.exists() for p in (out, st, full, blk))
    two = [torch.device("cpu"), torch.device("meta")]                      # two workers on a GPU-less host
    got = drivers.restore_shrunk_frames(str(d), str(npz), 8, str(out), stretched_dir=str(st), fullres_masks_dir=str(full),
                                        block_masks_dir=str(blk), devices=two, _shard_fn=_inpaint_hooks.restore_on_host)
    assert np.array_equal(got, masks)
    for sub in (d, out, st, full, blk):
        assert sorted(os.listdir(sub)) == names
    for i, n in enumerate(names):
        stretched = S.stretch_frame(shrunk[i], masks[i], 8)
        fullres = np.repeat(np.repeat(masks[i] * 255, 8, 0), 8, 1)
        assert np.array_equal(frameio.load_frame(d / n), shrunk[i])                # the inputs stay
        assert np.array_equal(frameio.load_frame(st / n), stretched)
        inpainted = frameio.load_frame(out / n)
        assert np.array_equal(inpainted, R.inpaint_frame(stretched, fullres))
        assert np.array_equal(inpainted[fullres == 0], stretched[fullres == 0]) and not np.array_equal(inpainted, stretched)
        with Image.open(blk / n) as im:
            assert im.mode == "L" and np.array_equal(np.asarray(im), masks[i] * 255)
        with Image.open(full / n) as im:
            assert im.mode == "L" and np.array_equal(np.asarray(im), fullres)
    # only the inpainted frames where no other directory is given
    out2 = tmp_path / "only"
    drivers.restore_shrunk_frames(str(d), str(npz), 8, str(out2), devices=["cpu"], _shard_fn=_inpaint_hooks.restore_on_host)
    assert sorted(os.listdir(out2)) == names and sorted(os.listdir(tmp_path)) == sorted(
        ["frames", "shrink_masks_8.npz", "inpainted", "stretched", "full", "blk", "only"])
    assert all(np.array_equal(frameio.load_frame(out2 / n), frameio.load_frame(out / n)) for n in names)
