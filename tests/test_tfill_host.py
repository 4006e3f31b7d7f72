"""The temporal fill, host side (no GPU): its numpy statement (tests/_tfill_ref.py), the mutants, the quality conditions
on the committed pan generator; the Python argument errors; the C entry points' exports, limits and validation; the
directory driver with a stand-in device step."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

import _inpaint_ref as I
import _shrink_ref as S
import _tfill_hooks
import _tfill_ref as R
import elvis_amd
from elvis_amd import _build, _lib, drivers, frameio

# the package exports the function `inpaint_temporal` under the module's own name: the module comes from the import system
inpaint_temporal = importlib.import_module("elvis_amd.inpaint_temporal")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"elvis_tfill_limits_ok": 9, "elvis_tfill": 15}
MUTANT_CASES = R.mutant_cases()


# ----------------------------------------------------------------------------- the numpy statement
@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_every_mutant_gives_other_bytes_on_its_case(mutant):
    frames, masks, p = MUTANT_CASES[R.MUTANTS[mutant]]
    true_out, true_left = R.temporal_fill(frames, masks, **p)
    out, left = R.temporal_fill(frames, masks, **p, mutant=mutant)
    assert out.shape == true_out.shape and left.shape == true_left.shape
    assert not (np.array_equal(out, true_out) and np.array_equal(left, true_left))
    assert np.array_equal(out[masks == 0], frames[masks == 0])


def test_the_required_mutants_are_there():
    assert {"ties_later", "no_half_rule", "next_first", "source_holes_known", "no_max_mad", "float32_division",
            "filled_as_context"} <= set(R.MUTANTS)
    assert set(R.MUTANTS.values()) <= set(MUTANT_CASES)


def test_the_named_cases_are_what_they_say():
    # near_tie: the contract takes (0, 0), float32 division keeps the earlier (0, -1)
    frames, masks, p = MUTANT_CASES["near_tie"]
    a, b = {}, {}
    R.temporal_fill(frames, masks, **p, stats=a)
    R.temporal_fill(frames, masks, **p, stats=b, mutant="float32_division")
    assert a == {(0, 0, 0, 1): (0, 0)} and b == {(0, 0, 0, 1): (0, -1)}
    # contrast: the winning product is below 2^32, every other one above
    frames, masks, p = MUTANT_CASES["contrast"]
    cnt, cost = R._displacement_sums(frames[0], masks[0] == 0, frames[1], masks[1] == 0, 16, 80, 16, 80, p["search"])
    prod = cnt * cost
    assert cnt.min() == cnt.max() == 64 * 64 - 16 and prod.min() < 2 ** 32 and np.sort(prod.ravel())[1] > 2 ** 32
    stats = {}
    R.temporal_fill(frames, masks, **p, stats=stats)
    assert stats == {(0, 32, 32, 1): (1, 2)}
    # tint: every cost per pixel is the same, the first valid displacement in raster order wins
    frames, masks, p = MUTANT_CASES["tint"]
    stats = {}
    out, left = R.temporal_fill(frames, masks, **p, stats=stats)
    assert stats[(1, 8, 8, 0)] == (-2, -2) and stats[(1, 8, 8, 2)] == (-2, -2)
    hole = masks[1] != 0
    assert set(np.unique(out[1][hole])) == {100, 102} and not left[1].any()      # both sources gave pixels, in their tints
    # strangers: nothing is accepted, everything is left
    frames, masks, p = MUTANT_CASES["strangers"]
    out, left = R.temporal_fill(frames, masks, **p)
    assert np.array_equal(out, frames) and np.array_equal(left, masks)


def test_sources_come_in_the_contracts_order():
    assert R.source_order(5, 20, 3) == [4, 6, 3, 7, 2, 8]
    assert R.source_order(0, 3, 2) == [1, 2] and R.source_order(2, 3, 8) == [1, 0] and R.source_order(0, 1, 8) == []
    assert R.source_order(1, 3, 0) == []


def test_known_pixels_and_remaining_holes_keep_their_bytes_and_hole_bytes_change_nothing():
    frames, masks, p = R.cases()["pixel_masks"]
    out, left = R.temporal_fill(frames, masks, **p)
    known, still = masks == 0, left != 0
    assert np.array_equal(out[known], frames[known]) and np.array_equal(out[still], frames[still])
    assert not (still & known).any() and set(np.unique(left)) <= {0, 255}
    other = R.holed(frames, masks, value=0xA5)
    out2, left2 = R.temporal_fill(other, masks, **p)
    assert np.array_equal(left, left2) and np.array_equal(out[~still], out2[~still])


def test_the_case_list_covers_the_matrix():
    cases = R.cases()
    shapes = {f.shape[1:3] for f, m, p in cases.values()}
    assert {(5, 7), (16, 16), (24, 40), (33, 49), (48, 64)} <= shapes
    assert {f.shape[3] for f, m, p in cases.values()} == {1, 3}
    assert {f.shape[0] for f, m, p in cases.values()} >= {1, 2, 5}
    assert {p["radius"] for f, m, p in cases.values()} >= {0, 1, 3}
    assert {p["search"] for f, m, p in cases.values()} >= {0, 3, 7}
    assert {(p["block"], p["margin"]) for f, m, p in cases.values()} >= {(8, 0), (16, 8), (32, 16)}
    assert any(p["radius"] > f.shape[0] for f, m, p in cases.values())
    assert all(f.dtype == m.dtype == np.uint8 and m.shape == f.shape[:3] and f.shape[1] <= 96 and f.shape[2] <= 96
               for f, m, p in cases.values())
    f, m, p = cases["tiny_5x7"]
    assert m.any() and np.array_equal(R.temporal_fill(f, m, **p)[1], np.where(m != 0, 255, 0))    # nk < MIN_CONTEXT
    f, m, p = cases["one_block_16x16"]
    assert m[0].all() and not m[1].any()
    assert cases["all_hole_frame"][1][2].all() and not cases["no_holes"][1].any()
    m = cases["same_mask_every_frame"][1]
    assert m.any() and (m == m[0]).all()


def test_the_cases_reach_both_ends():
    """Something is filled and something is left over the matrix; nothing is filled without sources or context."""
    cases = R.cases()
    # (B, G) = (8, 0): the window is the block, 64 pixels, and a block with a hole has fewer than MIN_CONTEXT known
    for name in ("n1_no_sources", "radius0", "tiny_5x7", "one_block_16x16", "strangers", "b8_g0_24x40_c1", "b8_g0_24x40_c3"):
        frames, masks, p = cases[name]
        out, left = R.temporal_fill(frames, masks, **p)
        assert np.array_equal(out, frames) and np.array_equal(left, np.where(masks != 0, 255, 0)), name
    frames, masks, p = cases["no_holes"]
    out, left = R.temporal_fill(frames, masks, **p)
    assert np.array_equal(out, frames) and not left.any()
    for name in ("defaults_48x64", "ragged_33x49_c3", "b32_g16_48x64", "pixel_masks", "same_mask_every_frame", "search0",
                 "block1", "block5_g3", "all_hole_frame"):
        frames, masks, p = cases[name]
        left = R.temporal_fill(frames, masks, **p)[1]
        assert 0 < (left != 0).sum() < (masks != 0).sum(), name


# ----------------------------------------------------------------------------- quality, on the statement alone
@pytest.fixture(scope="module")
def pan():
    """5 x 64 x 96, B = 16, 30 % of the blocks removed at random in every frame, the defaults."""
    noisy, clean = R.pan_clip(5, 64, 96, 3, seed=0)
    masks = R.random_block_masks(5, 64, 96, 16, 0.3, seed=1)
    frames = R.holed(noisy, masks, value=0)
    out, left = R.temporal_fill(frames, masks)
    return frames, clean, masks, out, left


def test_quality_conditions_on_the_pan_clip(pan):
    """Measured on the committed statement and generator: 15.7 % of the hole pixels left, the temporally filled pixels
    at 47.47 dB against the clean clip, fill + Telea 28.70 dB against 18.88 dB for Telea alone (+9.82 dB), and nothing
    filled with search = 2."""
    frames, clean, masks, out, left = pan
    hole, still = masks != 0, left != 0
    assert 0.25 < hole.mean() < 0.35
    assert still.sum() <= 0.20 * hole.sum()                                         # 15.7 %
    assert R.psnr(out, clean, hole & ~still) >= 40.0                                # 47.47 dB
    telea = I.inpaint(frames, masks)
    both = I.inpaint(out, left)
    assert R.psnr(both, clean, hole) >= R.psnr(telea, clean, hole) + 6.0            # 28.70 dB against 18.88 dB
    out2, left2 = R.temporal_fill(frames, masks, search=2)                          # the (2, 3) pan is out of reach
    assert np.array_equal(out2, frames) and np.array_equal(left2, masks)


# ----------------------------------------------------------------------------- the Python surface
def test_names_are_exported():
    for name in ("temporal_fill_device", "temporal_fill_blocks_device", "inpaint_temporal_device", "inpaint_temporal",
                 "restore_shrunk_frames"):
        assert callable(getattr(elvis_amd, name)), name
    assert inpaint_temporal.MIN_CONTEXT == R.MIN_CONTEXT and inpaint_temporal.DEFAULTS == R.DEFAULTS
    assert inpaint_temporal.LIMITS == R.LIMITS
    doc = inpaint_temporal.inpaint_temporal.__doc__
    assert "NEITHER ProPainter NOR E2FGVI" in doc


def test_value_errors_need_no_gpu():
    f = torch.zeros((2, 16, 24, 3), dtype=torch.uint8)
    m = torch.zeros((2, 16, 24), dtype=torch.uint8)
    bad = [
        (f.float(), m, "uint8"),
        (f, m.bool(), "masks must be"),
        (f, m[:, :, :23], "do not match"),
        (f[0], m, "uint8"),
        (torch.zeros((2, 16, 24, 4), dtype=torch.uint8), m, "channels"),
        (torch.zeros((2, 16, 24, 2), dtype=torch.uint8), m, "channels"),
        (f, m, "CUDA"),
    ]
    for frames, masks, msg in bad:
        with pytest.raises(ValueError, match=msg):
            inpaint_temporal.temporal_fill_device(frames, masks)
        with pytest.raises(ValueError, match=msg):
            inpaint_temporal.inpaint_temporal_device(frames, masks)
    for name, (lo, hi) in R.LIMITS.items():
        for v in (lo - 1, hi + 1, 2.0, "3", True, None):
            with pytest.raises(ValueError, match=name):
                inpaint_temporal.temporal_fill_device(f, m, **{name: v})
            with pytest.raises(ValueError, match=name):
                inpaint_temporal.temporal_fill_blocks_device(f, torch.zeros((2, 2, 3), dtype=torch.uint8), 8, **{name: v})
        for v in (lo, hi):
            with pytest.raises(ValueError, match="CUDA"):                           # inside the limits: the next check
                inpaint_temporal.temporal_fill_device(f, m, **{name: v})
    with pytest.raises(ValueError, match="unknown parameter"):
        inpaint_temporal.inpaint_temporal_device(f, m, blocks=8)
    with pytest.raises(ValueError, match="do not match"):
        inpaint_temporal.temporal_fill_blocks_device(f, m, 8)
    with pytest.raises(ValueError, match="block_size"):
        inpaint_temporal.temporal_fill_blocks_device(f, torch.zeros((2, 2, 3), dtype=torch.uint8), 0)
    with pytest.raises(ValueError, match="CUDA"):
        inpaint_temporal.temporal_fill_blocks_device(f, torch.zeros((2, 2, 3), dtype=torch.bool), 8)
    with pytest.raises(ValueError, match="frames"):
        inpaint_temporal.inpaint_temporal(np.zeros((2, 16, 24, 3), np.float32), np.zeros((2, 2, 3), bool))
    with pytest.raises(ValueError, match="masks"):
        inpaint_temporal.inpaint_temporal(np.zeros((2, 16, 24, 3), np.uint8), np.zeros((3, 2, 3), bool))
    with pytest.raises(ValueError, match="whole square blocks"):
        inpaint_temporal.inpaint_temporal(np.zeros((2, 16, 24, 3), np.uint8), np.zeros((2, 2, 4), bool))
    with pytest.raises(ValueError, match="search"):
        inpaint_temporal.inpaint_temporal(np.zeros((2, 16, 24, 3), np.uint8), np.zeros((2, 2, 3), bool), search=8)


# ----------------------------------------------------------------------------- the built library
def test_library_exports_the_entries_and_the_tables_agree(built_lib):
    h = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "elvis_amd.h")).read(), flags=re.S)
    for name, nargs in ENTRIES.items():
        assert hasattr(h, name), f"{name} is not exported"
        assert len(_lib.SIGNATURES[name]) == nargs
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
        assert decl and len([a for a in decl.group(1).split(",") if a.strip()]) == nargs, name
    assert "tfill.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "tools", "tfill_host_check.cpp"))
    source = open(os.path.join(ROOT, "elvis_amd", "csrc", "tfill.hip")).read()
    assert f"kMinContext = {R.MIN_CONTEXT};" in source and "__builtin_amdgcn_sad_u8" in source


def test_limits_and_argument_errors(built_lib):
    h = _lib.lib()
    ok = dict(n=2, h=40, w=48, c=3, block=16, margin=8, radius=2, search=7, max_mad=6)

    def limits(**kw):
        a = dict(ok, **kw)
        return h.elvis_tfill_limits_ok(*(a[k] for k in ("n", "h", "w", "c", "block", "margin", "radius", "search", "max_mad")))
    assert limits() == 1
    for name, (lo, hi) in R.LIMITS.items():
        assert limits(**{name: lo}) == 1 and limits(**{name: hi}) == 1
        assert limits(**{name: lo - 1}) == 0 and limits(**{name: hi + 1}) == 0
    assert limits(c=1) == 1 and limits(c=2) == 0 and limits(c=4) == 0
    assert limits(n=0) == 0 and limits(h=0) == 0 and limits(w=0) == 0
    assert limits(h=32767, w=8) == 1 and limits(h=32768, w=8) == 0 and limits(w=32768, h=8) == 0
    assert limits(n=2, h=32767, w=32767, c=1) == 1 and limits(n=1, h=32767, w=32767, c=3) == 0      # n*h*w*c < 2^31

    def bad(rc, word):
        assert rc == -1 and word in h.elvis_last_error(), (rc, h.elvis_last_error())
    F, K, O, L = 0x100000, 0x200000, 0x300000, 0x400000            # never dereferenced: every call is refused
    args = (2, 40, 48, 3, 16, 8, 2, 7, 6, None)
    bad(h.elvis_tfill(None, K, 0, O, L, *args), b"null")
    bad(h.elvis_tfill(F, None, 0, O, L, *args), b"null")
    bad(h.elvis_tfill(F, K, 0, None, L, *args), b"null")
    bad(h.elvis_tfill(F, K, 0, O, None, *args), b"null")
    bad(h.elvis_tfill(F, K, 0, O, L, 2, 40, 48, 2, 16, 8, 2, 7, 6, None), b"channels")
    bad(h.elvis_tfill(F, K, 0, O, L, 0, 40, 48, 3, 16, 8, 2, 7, 6, None), b"limits")
    bad(h.elvis_tfill(F, K, 0, O, L, 2, 40, 48, 3, 33, 8, 2, 7, 6, None), b"limits")
    bad(h.elvis_tfill(F, K, 0, O, L, 2, 40, 48, 3, 16, 17, 2, 7, 6, None), b"limits")
    bad(h.elvis_tfill(F, K, 0, O, L, 2, 40, 48, 3, 16, 8, 9, 7, 6, None), b"limits")
    bad(h.elvis_tfill(F, K, 0, O, L, 2, 40, 48, 3, 16, 8, 2, 8, 6, None), b"limits")
    bad(h.elvis_tfill(F, K, 0, O, L, 2, 40, 48, 3, 16, 8, 2, 7, 256, None), b"limits")
    bad(h.elvis_tfill(F, K, -1, O, L, *args), b"block_mask_size")
    bad(h.elvis_tfill(F, K, 0, F, L, *args), b"out may not alias frames")
    bad(h.elvis_tfill(F, K, 0, F + 2 * 40 * 48 * 3 - 1, L, *args), b"out may not alias frames")
    bad(h.elvis_tfill(F, K, 0, O, K, *args), b"left may not alias")
    bad(h.elvis_tfill(F, K, 0, O, O + 5, *args), b"left may not alias")
    bad(h.elvis_tfill(F, K, 0, K + 100, L, *args), b"out may not alias masks")


# ----------------------------------------------------------------------------- the driver
def test_an_unknown_inpainter_is_a_value_error_before_anything_is_written(tmp_path):
    for kw, msg in ((dict(inpainter="propainter"), "inpainter must be one of"),
                    (dict(inpainter=None), "inpainter must be one of"),
                    (dict(inpainter="telea", inpaint_params={"radius": 1}), "takes no inpaint_params"),
                    (dict(inpainter="temporal", inpaint_params={"radius": 9}), "radius"),
                    (dict(inpainter="temporal", inpaint_params={"window": 9}), "unknown parameter"),
                    (dict(inpainter="temporal", inpaint_params=[1]), "dict")):
        with pytest.raises(ValueError, match=msg):
            drivers.restore_shrunk_frames(str(tmp_path / "none"), str(tmp_path / "none.npz"), 8, str(tmp_path / "out"), **kw)
    assert os.listdir(tmp_path) == []


def _write_shrunk_pan(tmp_path, n=5, by=4, bx=6, b=8, k=2, seed=0):
    """A panning clip with k blocks removed per block row, shrunk: the frames directory and the masks file."""
    rng = np.random.default_rng(seed)
    noisy, _ = R.pan_clip(n, by * b, bx * b, 3, seed=seed)
    d = tmp_path / "frames"
    d.mkdir()
    masks = np.zeros((n, by, bx), np.uint8)
    shrunk = []
    for i in range(n):
        for r in range(by):
            masks[i, r, rng.choice(bx, k, replace=False)] = 1
        rows = [np.concatenate([noisy[i, r * b:(r + 1) * b, c * b:(c + 1) * b] for c in range(bx) if not masks[i, r, c]], axis=1)
                for r in range(by)]
        shrunk.append(np.concatenate(rows, axis=0))
        frameio.save_frame(shrunk[-1], d / f"{i + 1:05d}.png")
    frameio.save_block_masks(masks, tmp_path / "shrink_masks_8.npz")
    return d, tmp_path / "shrink_masks_8.npz", masks, shrunk


def test_driver_with_two_workers_equals_the_whole_clip_and_writes_every_file_once(tmp_path):
    d, npz, masks, shrunk = _write_shrunk_pan(tmp_path)
    params = dict(block=8, margin=8, radius=2, search=4, max_mad=8)
    names = [f"{i + 1:05d}.png" for i in range(len(shrunk))]
    stretched = np.stack([S.stretch_frame(shrunk[i], masks[i], 8) for i in range(len(shrunk))])
    full = R.expand_block_mask(masks, 8, stretched.shape[1], stretched.shape[2])
    out, left = R.temporal_fill(stretched, full, **R.DEFAULTS | params)
    assert 0 < (left != 0).sum() < (full != 0).sum()                          # both inpainters have work
    ref = I.inpaint(out, left)
    for workers, sub in (([torch.device("cpu")], "one"), ([torch.device("cpu"), torch.device("meta")], "two")):
        o, st, fm = (tmp_path / f"{sub}_{s}" for s in ("out", "stretched", "full"))
        got = drivers.restore_shrunk_frames(str(d), str(npz), 8, str(o), stretched_dir=str(st), fullres_masks_dir=str(fm),
                                            devices=workers, inpainter="temporal", inpaint_params=params,
                                            _shard_fn=_tfill_hooks.restore_on_host)
        assert np.array_equal(got, masks)
        for sub_dir in (o, st, fm, str(st) + "_once", str(fm) + "_once"):
            assert sorted(os.listdir(sub_dir)) == names
        for i, n in enumerate(names):
            assert np.array_equal(frameio.load_frame(o / n), ref[i]), (sub, n)
            assert np.array_equal(frameio.load_frame(st / n), stretched[i])
