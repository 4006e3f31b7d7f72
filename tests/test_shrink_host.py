"""ELVIS v1 shrink / stretch, host side (no GPU): the numpy restatement against the reference's own outputs, bit for
bit; the Python argument errors; the C entry points' validation; the directory driver with a stand-in device step."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _shrink_hooks
import _shrink_ref as R
from elvis_amd import _lib, drivers, frameio, shrink


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.fixture(scope="module")
def cases(golden_dir):
    with np.load(os.path.join(golden_dir, "shrink.npz"), allow_pickle=False) as z:
        return R.golden_cases(z)


def test_golden_covers_the_contract(cases):
    fams = {d["family"] for _, d in cases}
    assert fams == set(R.FAMILIES)
    assert {d["block"] for _, d in cases} == {4, 8, 16}
    assert {d["scores"].dtype for _, d in cases} == {np.dtype(np.float32), np.dtype(np.float64)}
    grids = {d["scores"].shape for _, d in cases}
    assert (1, 1) in grids and (12, 20) in grids
    for _, d in cases:
        by, bx = d["scores"].shape
        if d["family"] == "elvis":
            assert all(len(np.unique(r)) == bx for r in d["scores"])          # top-k ties are not pinned
    passes = [d for _, d in cases if d["family"] != "elvis"]
    assert any(len(np.unique(d["scores"])) < d["scores"].size for d in passes)     # argmin ties are
    assert any(d["frame"].shape[0] % d["block"] and d["frame"].shape[1] % d["block"] for d in passes)
    pm = [d for d in passes if d["family"] == "position_map"]
    assert any(len(d["ridx_counts"]) == 0 for d in pm)                             # no removal
    assert any(d["shrunk"].size == 0 for _, d in cases)                            # everything removed
    assert any(d["amount"] == 0.95 for d in pm)
    # partial row pass / partial column pass: the last pass is shorter than the lines it could visit
    last_row = [d for d in pm if len(d["ridx_counts"]) % 2 == 1 and d["shrunk"].shape[1] // d["block"] + len(d["ridx_counts"]) // 2 + 1
                > d["scores"].shape[1]]
    last_col = [d for d in pm if len(d["ridx_counts"]) and len(d["ridx_counts"]) % 2 == 0
                and d["shrunk"].shape[0] // d["block"] + len(d["ridx_counts"]) // 2 > d["scores"].shape[0]]
    assert last_row and last_col
    # the row-only quirk: a partial pass leaves rows with fewer mask entries than columns lost
    assert any(d["family"] == "row_only" and len(set(d["mask"].sum(axis=1))) > 1 for _, d in cases)


def test_restatement_equals_reference_outputs(cases):
    for i, d in cases:
        b, amount, frame, scores = d["block"], d["amount"], d["frame"], d["scores"]
        f0, s0 = frame.copy(), scores.copy()
        by, bx = scores.shape
        if d["family"] == "elvis":
            shrunk, mask, coords = R.apply_selective_removal(frame, scores, b, amount)
            assert _same(shrunk, d["shrunk"]) and _same(mask, d["mask"]) and coords == d["coords"], i
            assert _same(R.stretch_frame(shrunk, mask, b), d["stretched"]), i
        elif d["family"] == "row_only":
            shrunk, mask = R.shrink_frame_row_only(frame, scores, b, amount)
            assert _same(shrunk, d["shrunk"]) and _same(mask, d["mask"]), i
            assert _same(R.stretch_frame_row_only(shrunk, mask, b), d["stretched"]), i
        else:
            shrunk, mask, pmap = R.shrink_frame_position_map(frame, scores, b, amount)
            assert _same(shrunk, d["shrunk"]) and _same(mask, d["mask"]) and _same(pmap, d["posmap"]), i
            shrunk2, mask2, ridx = R.shrink_frame_removal_indices(frame, scores, b, amount)
            assert _same(shrunk2, d["shrunk"]) and _same(mask2, d["mask"]), i
            assert len(ridx) == len(d["ridx"]) and all(_same(x, y) for x, y in zip(ridx, d["ridx"])), i
            assert _same(R.stretch_frame_position_map(shrunk, mask, pmap, b), d["stretched"]), i
            assert _same(R.stretch_frame_removal_indices(shrunk, ridx, by, bx, b), d["stretched_ridx"]), i
        assert _same(R.stretch_video_frames([d["shrunk"]], [d["mask"]], b)[0], d["stretched_presley"]), i
        assert np.array_equal(frame, f0) and np.array_equal(scores, s0)


def test_host_index_maps_equal_restatement(cases):
    """The two stretches whose map is built on the host (elvis_amd.shrink) against the restatement and the plan of
    the pass rule (shrunk grid, per-pass counts) against the reference's outputs."""
    for i, d in cases:
        if d["family"] == "elvis":
            assert shrink.topk_count(d["amount"], d["scores"].shape[1]) == d["scores"].shape[1] - d["shrunk"].shape[1] // d["block"]
            continue
        by, bx = d["scores"].shape
        b = d["block"]
        sgrid = (d["shrunk"].shape[0] // b, d["shrunk"].shape[1] // b)
        mode = "rows" if d["family"] == "row_only" else "rows_cols"
        sby, sbx, counts = shrink.passes_plan(by, bx, shrink.passes_target(by, bx, d["amount"]), mode)
        assert (sby, sbx) == sgrid, i
        if d["family"] == "position_map":
            assert counts == [int(v) for v in d["ridx_counts"]], i
            assert _same(shrink.position_map_to_src_of(d["posmap"], (by, bx)), R.position_map_src_of(d["posmap"], (by, bx))), i
            assert _same(shrink.removal_indices_to_src_of(d["ridx"], sgrid), R.removal_indices_src_of(d["ridx"], sgrid)), i


def test_stretch_frame_count_mismatch_and_argument_errors():
    f = np.zeros((8, 16, 3), np.uint8)
    with pytest.raises(ValueError, match="cannot assign"):
        R.stretch_frame(f, np.zeros((1, 3), np.int8), 8)
    with pytest.raises(ValueError, match="cannot assign"):                 # checked on the host, before any device work
        shrink.stretch_frame(f, np.zeros((1, 3), np.int8), 8)
    with pytest.raises(ValueError, match="divisible"):
        shrink.stretch_frame(np.zeros((8, 15, 3), np.uint8), np.zeros((1, 1), np.int8), 8)
    with pytest.raises(ValueError, match="uint8"):
        shrink.stretch_frame(f.astype(np.float32), np.zeros((1, 2), np.int8), 8)
    with pytest.raises(ValueError, match="divisible"):
        shrink.apply_selective_removal(np.zeros((8, 15, 3), np.uint8), np.zeros((1, 1)), 8, 0.5)
    with pytest.raises(ValueError, match="block grid"):
        shrink.apply_selective_removal(f, np.zeros((1, 3)), 8, 0.5)
    with pytest.raises(ValueError, match="NaN"):
        shrink.shrink_frame_row_only(f, np.array([[0.0, np.nan]]), 8, 0.5)
    with pytest.raises(ValueError, match="shrink_amount"):
        shrink.shrink_frame_position_map(f, np.zeros((1, 2)), 8, 1.5)
    with pytest.raises(ValueError, match="shrink_amount"):
        shrink.apply_selective_removal(f, np.zeros((1, 2)), 8, -0.5)
    with pytest.raises(ValueError, match="smaller than one block"):
        shrink.shrink_frame_removal_indices(np.zeros((4, 4, 3), np.uint8), np.zeros((0, 0)), 8, 0.5)
    with pytest.raises(ValueError, match="outside"):
        shrink.position_map_to_src_of(np.array([[[0, 5]]]), (1, 2))
    with pytest.raises(ValueError, match="non-negative"):
        shrink.removal_indices_to_src_of([np.array([-1], np.int32)], (1, 1))
    with pytest.raises(ValueError, match="mode"):
        shrink.passes_plan(4, 4, 3, "diagonal")
    if not torch.cuda.is_available():                                      # no CPU fallback
        with pytest.raises(RuntimeError):
            shrink.stretch_frame(f, np.zeros((1, 2), np.int8), 8, device="cpu")
        with pytest.raises(RuntimeError):
            shrink.shrink_frame_row_only(f, np.zeros((1, 2)), 8, 0.5)


def test_c_entry_points_validate_without_gpu(built_lib):
    h = _lib.lib()

    def bad(rc, text):
        assert rc == -1 and text in h.elvis_last_error(), h.elvis_last_error()

    bad(h.elvis_block_gather_u8(None, None, None, None, 1, 8, 8, 3, 8, 1, 1, 1, 1, None), b"null")
    bad(h.elvis_block_gather_u8(16, 16, 16, None, 1, 8, 8, 3, 0, 1, 1, 1, 1, None), b"block_size")
    bad(h.elvis_block_gather_u8(16, 16, 16, None, 1, 8, 8, 2, 8, 1, 1, 1, 1, None), b"channels")
    bad(h.elvis_block_gather_u8(16, 16, 16, None, 1, 8, 8, 3, 8, 1, 2, 1, 1, None), b"does not fit")
    bad(h.elvis_block_gather_u8(16, 16, 16, None, 0, 8, 8, 3, 8, 1, 1, 1, 1, None), b"bad shape")
    bad(h.elvis_shrink_select_topk(None, None, None, 1, 2, 2, 1, None), b"null")
    bad(h.elvis_shrink_select_topk(16, 16, 16, 1, 2, 2, 3, None), b"outside [0, 2]")
    bad(h.elvis_shrink_select_topk(16, 16, 16, 1, 0, 2, 1, None), b"bad shape")
    bad(h.elvis_shrink_select_passes(None, None, None, None, None, None, 1, 2, 2, 1, 0, 2, 1, None), b"null")
    bad(h.elvis_shrink_select_passes(16, 16, 16, None, 16, 16, 1, 6, 10, 15, 0, 6, 8, None), b"is 6x7, not 6x8")
    bad(h.elvis_shrink_select_passes(16, 16, 16, None, 16, 16, 1, 6, 10, 61, 1, 6, 8, None), b"target")
    bad(h.elvis_shrink_select_passes(16, 16, 16, None, 16, 16, 1, 6, 10, 15, 2, 6, 8, None), b"mode")
    bad(h.elvis_stretch_index(None, None, 1, 2, 2, 1, 1, 0, None), b"null")
    bad(h.elvis_stretch_index(16, 16, 1, 2, 2, 1, 1, 5, None), b"mode")
    sby, sbx = C.c_int(0), C.c_int(0)
    counts = (C.c_int * 8)()
    assert h.elvis_shrink_passes_plan(6, 10, 19, 1, C.addressof(sby), C.addressof(sbx), C.addressof(counts), 8) == 3
    assert (sby.value, sbx.value, list(counts[:3])) == (5, 9, [6, 9, 4])           # 45 blocks for 41 kept
    assert h.elvis_shrink_passes_plan(6, 10, 15, 0, C.addressof(sby), C.addressof(sbx), None, 0) == 3
    assert (sby.value, sbx.value) == (6, 7)
    bad(h.elvis_shrink_passes_plan(6, 10, 15, 0, None, None, None, 0), b"null")
    bad(h.elvis_shrink_passes_plan(0, 10, 0, 0, C.addressof(sby), C.addressof(sbx), None, 0), b"bad grid")


def _write_shrunk_clip(tmp_path, n=5, by=3, bx=4, b=8, k=1, seed=0):
    rng = np.random.default_rng(seed)
    d = tmp_path / "frames"
    d.mkdir()
    masks = np.zeros((n, by, bx), np.uint8)
    shrunk = []
    for i in range(n):
        for r in range(by):
            masks[i, r, rng.choice(bx, k, replace=False)] = 1
        f = rng.integers(0, 250, size=(by * b, (bx - k) * b, 3), dtype=np.uint8)
        frameio.save_frame(f, d / f"{i + 1:05d}.png")
        shrunk.append(f)
    frameio.save_block_masks(masks, tmp_path / "shrink_masks_8.npz")
    return d, tmp_path / "shrink_masks_8.npz", masks, shrunk


def test_driver_names_and_mask_pngs(tmp_path):
    from PIL import Image
    d, npz, masks, shrunk = _write_shrunk_clip(tmp_path)
    out, full, blk = tmp_path / "stretched", tmp_path / "full", tmp_path / "blk"
    two = [torch.device("cpu"), torch.device("meta")]                      # two workers on a GPU-less host
    got = drivers.stretch_shrunk_frames(str(d), str(npz), 8, out_dir=str(out), fullres_masks_dir=str(full),
                                        block_masks_dir=str(blk), devices=two, _shard_fn=_shrink_hooks.stretch_on_host)
    assert np.array_equal(got, masks)
    names = [f"{i + 1:05d}.png" for i in range(len(shrunk))]
    for sub in (out, full, blk):
        assert sorted(os.listdir(sub)) == names
    for i, n in enumerate(names):
        assert np.array_equal(frameio.load_frame(out / n), R.stretch_frame(shrunk[i], masks[i], 8))
        assert np.array_equal(frameio.load_frame(d / n), shrunk[i])                # inputs untouched with out_dir
        with Image.open(blk / n) as im:
            assert im.mode == "L" and np.array_equal(np.asarray(im), masks[i] * 255)
        with Image.open(full / n) as im:
            assert im.mode == "L" and np.array_equal(np.asarray(im), np.repeat(np.repeat(masks[i] * 255, 8, 0), 8, 1))
    # in place, one worker, no mask directories
    drivers.stretch_shrunk_frames(str(d), str(npz), 8, devices=["cpu"], _shard_fn=_shrink_hooks.stretch_on_host)
    assert sorted(os.listdir(d)) == names
    assert all(np.array_equal(frameio.load_frame(d / n), frameio.load_frame(out / n)) for n in names)
    # the frames are stretched now: they no longer hold what the masks keep
    with pytest.raises(ValueError, match="does not hold"):
        drivers.stretch_shrunk_frames(str(d), str(npz), 8, devices=["cpu"], _shard_fn=_shrink_hooks.stretch_on_host)
    os.unlink(d / names[-1])
    with pytest.raises(ValueError, match="No frame 00005.png"):
        drivers.stretch_shrunk_frames(str(d), str(npz), 8, devices=["cpu"], _shard_fn=_shrink_hooks.stretch_on_host)
