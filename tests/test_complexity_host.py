"""Block complexity, host side (no GPU): the numpy statement of the contract (tests/_complexity_ref.py) and its mutants;
the nearest mask resize; `removability_from_complexity` against the reference's own `calculate_removability_scores`
(tests/golden/removability.npz, tools/make_removability_golden.py); the Python argument errors; the C entry point's
export and validation; the kernel ledger."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _complexity_ref as R
import elvis_amd
from elvis_amd import _build, _lib, complexity, tiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "elvis_amd", "csrc", "complexity.hip")
ENTRY, NARGS = "elvis_block_complexity_f64", 13


# ----------------------------------------------------------------------------- the numpy statement
@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_every_mutant_moves_its_case_by_a_thousand_bars(mutant):
    case = R.BY_ID[R.MUTANTS[mutant]]
    frames, prev = R.inputs(case)
    sc, tc = R.expected(case.id)
    msc, mtc = R.complexity(frames, case.block, case.order, prev, mutant=mutant)
    assert msc.shape == sc.shape and mtc.shape == tc.shape
    moved = max(np.abs(msc - sc).max(), np.abs(mtc - tc).max())
    print(f"{mutant}: moves {case.id} by {moved:.3g}")
    assert moved >= R.MUTANT_MIN
    assert not (R.within_bar(msc, sc) and R.within_bar(mtc, tc))


def test_the_named_cases_are_what_the_mutants_need():
    assert set(R.MUTANTS.values()) <= {c.id for c in R.NAMED}
    assert R.BY_ID[R.MUTANTS["prev_ignored"]].prev and R.BY_ID[R.MUTANTS["tc_against_next_frame"]].shape[0] >= 3
    rem = R.BY_ID[R.MUTANTS["origin_shifted_by_remainder"]]
    assert rem.shape[1] % rem.block and rem.shape[2] % rem.block
    for name in ("rgb_bgr_swapped", "full_range_luma"):
        assert R.BY_ID[R.MUTANTS[name]].shape[3] == 3


def test_a_second_evaluation_order_agrees_far_inside_the_bar():
    """The contract block by block with matrix products, against the einsum over all blocks."""
    worst = 0.0
    for case in R.NAMED:
        frames, prev = R.inputs(case)
        sc, tc = R.expected(case.id)
        b = case.block
        dct, weight = R.tables(b)
        y = R.luma(frames, case.order)
        p = np.concatenate([y[:1] if prev is None else R.luma(prev[None], case.order), y[:-1]])
        for f in range(case.shape[0]):
            for i in range(case.grid[0]):
                for j in range(case.grid[1]):
                    x = y[f, i * b:(i + 1) * b, j * b:(j + 1) * b]
                    d = x - p[f, i * b:(i + 1) * b, j * b:(j + 1) * b]
                    for want, blk in ((sc, x), (tc, d)):
                        got = (weight * np.abs(dct @ (blk - blk[0, 0]).astype(np.float64) @ dct.T)).sum() / b ** 2
                        worst = max(worst, abs(got - want[f, i, j]) / max(1.0, abs(want[f, i, j])))
    print(f"two evaluation orders: worst {worst:.3g} of a bar of {R.BAR}")
    assert worst <= 1e-3 * R.BAR


def test_tables_are_the_contract():
    for b in R.BLOCKS:
        dct, weight = complexity.complexity_tables(b)
        rd, rw = R.tables(b)
        assert dct.dtype == weight.dtype == np.float64 and dct.shape == weight.shape == (b, b)
        assert np.abs(dct - rd).max() <= 4 * np.finfo(np.float64).eps and np.array_equal(weight, rw)
        assert np.abs(dct @ dct.T - np.eye(b)).max() < 1e-14                 # orthonormal: s_0 = sqrt(1/B), s_k = sqrt(2/B)
        assert weight[0, 0] == 0.0 and weight[0, 1] == np.e and weight[b - 1, b - 1] == np.exp(abs(((b - 1) ** 2 / b ** 2) ** 2 - 1))
    with pytest.raises(ValueError, match="block_size"):
        complexity.complexity_tables(12)


def test_flat_blocks_and_unchanged_blocks_are_exactly_zero():
    rng = np.random.default_rng(5)
    for b in R.BLOCKS:
        for c, order in R.COLOURS:
            frames = rng.integers(0, 256, (3, 2 * b + 3, 3 * b + 1, c), dtype=np.uint8)
            frames[:, :b, b:2 * b] = np.asarray([[[[0]]], [[[16]]], [[[255]]]], np.uint8)      # a flat block per frame
            frames[1, b:2 * b, :b] = frames[0, b:2 * b, :b]                                      # one block does not change
            sc, tc = R.complexity(frames, b, order)
            assert (sc[:, 0, 1] == 0.0).all() and np.count_nonzero(sc) == sc.size - 3
            assert tc[1, 1, 0] == 0.0 and (tc[0] == 0.0).all()
            assert (tc[:, 0, 1] == 0.0).all() and np.count_nonzero(tc[1:]) == tc[1:].size - 3      # flat to flat: the difference is flat
            sc2, tc2 = R.complexity(frames[1:], b, order, prev=frames[0])
            assert np.array_equal(sc2, sc[1:]) and np.array_equal(tc2, tc[1:])


def test_the_remainder_never_reaches_an_output():
    case = R.BY_ID["named_b8_gray_remainder"]
    frames, _ = R.inputs(case)
    other = frames.copy()
    by, bx = case.grid
    other[:, by * 8:] ^= 0xFF
    other[:, :, bx * 8:] ^= 0xFF
    for a, b in zip(R.complexity(frames, 8), R.complexity(other, 8)):
        assert np.array_equal(a, b)


def test_the_case_list_covers_the_matrix():
    assert {c.kernel for c in R.MATRIX} == {f"block_complexity_kernel<{b},{c},{int(o == 'bgr')}>" for b in R.BLOCKS for c, o in R.COLOURS}
    for b in R.BLOCKS:
        cs = [c for c in R.MATRIX if c.block == b]
        for ch, order in R.COLOURS:
            mine = [c for c in cs if c.shape[3] == ch and c.order == order]
            assert {(c.shape[1], c.shape[2], c.shape[0]) for c in mine if c.id.startswith("m_")} == {
                (h, w, n) for h in R.sizes(b) for w in R.sizes(b) for n in (1, 2, 3)}
            assert {c.prev for c in mine} == {False, True}
            grids = {c.grid for c in mine}
            assert {(1, 1), (1, 3), (3, 1), (1, 2), (2, 1), (3, 3)} <= grids
            per_group = R.STRIP_PIXELS // (b * b)
            assert any(g[1] > per_group and (per_group == 1 or g[1] % per_group) for g in grids)        # more than a workgroup takes, last strip not full
        assert max(c.grid[0] for c in cs) <= 3 and max(c.grid[1] for c in cs) <= 17
    text = open(SOURCE).read()
    assert int(re.search(r"#define\s+CX_TILE\s+(\d+)", text).group(1)) == R.STRIP_PIXELS


# ----------------------------------------------------------------------------- masks and removability
def test_resize_masks_nearest():
    rng = np.random.default_rng(2)
    for (sh, sw), (by, bx) in [((4, 6), (8, 12)), ((4, 6), (9, 7)), ((64, 48), (4, 3)), ((37, 53), (2, 3)), ((5, 5), (5, 5)),
                               ((1, 1), (3, 4)), ((7, 3), (3, 7)), ((1080, 1920), (67, 120))]:
        m = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
        got, none = complexity.resize_masks_nearest([m, None], by, bx)
        assert none is None and got.shape == (by, bx) and got.dtype == np.uint8
        for y in range(by):
            for x in range(0, bx, max(1, bx // 7)):
                assert got[y, x] == m[(y * sh) // by, (x * sw) // bx]
        assert np.array_equal(got, m[tiler._nearest_rows(sh, by)][:, tiler._nearest_rows(sw, bx)])
    f = complexity.resize_masks_nearest(np.ones((2, 4, 4), np.float32), 2, 2)
    assert len(f) == 2 and f[0].dtype == np.float32 and f[0].shape == (2, 2)
    with pytest.raises(ValueError, match="2-D"):
        complexity.resize_masks_nearest([np.zeros((2, 2, 3), np.uint8)], 2, 2)


def _golden_cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "removability.npz"))
    at = {k: 0 for k in ("spatial", "temporal", "masks", "scores")}

    def take(key, shape):
        size = int(np.prod(shape))
        out = g[key][at[key]:at[key] + size].reshape(shape)
        at[key] += size
        return out
    for (count, by, bx, mh, mw, missing), (alpha, beta) in zip(g["params"], g["alpha_beta"]):
        grid = (count, by, bx)
        yield (take("spatial", grid), take("temporal", grid), take("masks", (count, mh, mw)), take("scores", grid), int(missing),
               float(alpha), float(beta))
    assert all(at[k] == g[k].size for k in at)


def test_removability_equals_the_references_own_function(golden_dir):
    seen = set()
    for spatial, temporal, masks, scores, missing, alpha, beta in _golden_cases(golden_dir):
        given = [None if i == missing else masks[i] for i in range(len(masks))]
        keep = spatial.copy(), temporal.copy()
        got = complexity.removability_from_complexity(spatial, temporal, given, alpha, beta)
        assert got.dtype == np.float64 and np.array_equal(got, scores)
        assert np.array_equal(spatial, keep[0]) and np.array_equal(temporal, keep[1])
        flat = np.ptp(spatial) == 0 and np.ptp(temporal) == 0
        if flat and ((masks == 0).all() or (masks != 0).all()):                 # no spread anywhere: the last guard decides
            assert np.ptp(got) == 0 and got.flat[0] != 0
        seen.add((len(spatial), alpha, beta, missing >= 0, bool(flat), bool((masks == 0).all()), bool((masks != 0).all())))
        if missing >= 0 and (masks[missing] == 0).any():                       # the frame without a mask is left alone
            zeroed = [m for m in masks]
            assert not np.array_equal(complexity.removability_from_complexity(spatial, temporal, zeroed, alpha, beta), scores)
    assert {s[0] for s in seen} == {2, 3} and {s[1] for s in seen} == {0.0, 0.25, 0.5, 1.0} and {s[2] for s in seen} >= {1.0, 0.5}
    assert any(s[3] for s in seen) and any(s[4] for s in seen) and any(s[5] for s in seen) and any(s[6] for s in seen)


def test_removability_by_hand():
    """Two frames, two blocks: every step written out."""
    s = np.asarray([[[0.0, 2.0]], [[4.0, 1.0]]])
    t = np.asarray([[[9.0, 9.0]], [[1.0, 3.0]]])
    sn, tn = s / 4.0, (t - 1.0) / 8.0
    mixed = np.stack([0.25 * sn[0] + 0.75 * tn[1], sn[1]])
    masks = [np.asarray([[0, 7], [0, 7]], np.uint8), None]
    mixed[0, 0, 0] *= 10.0
    smooth = np.stack([mixed[0], 0.5 * mixed[1] + 0.5 * mixed[0]])
    want = (smooth - smooth.min()) / (smooth.max() - smooth.min())
    assert np.array_equal(complexity.removability_from_complexity(s, t, masks, 0.25, 0.5), want)
    # smoothing_beta = 1: no smoothing; no masks at all; a single frame is its normalised SC
    plain = np.stack([0.25 * sn[0] + 0.75 * tn[1], sn[1]])
    assert np.array_equal(complexity.removability_from_complexity(s, t, None, 0.25), (plain - plain.min()) / np.ptp(plain))
    assert np.array_equal(complexity.removability_from_complexity(s[:1], t[:1]), sn[:1] * 2.0)
    # the arrays' own dtype
    assert complexity.removability_from_complexity(s.astype(np.float32), t.astype(np.float32), masks, 0.25, 0.5).dtype == np.float32
    with pytest.raises(ValueError, match="one shape"):
        complexity.removability_from_complexity(s, t[:1])


# ----------------------------------------------------------------------------- the Python surface
def test_names_are_exported():
    for name in ("block_complexity_device", "analyze_frames", "EVCAConfig", "resize_masks_nearest", "removability_from_complexity",
                 "calculate_removability_scores_from_frames"):
        assert callable(getattr(elvis_amd, name)), name
    assert elvis_amd.EVCAConfig().block_size == 16 and elvis_amd.EVCAConfig(block_size=8).block_size == 8
    doc = elvis_amd.calculate_removability_scores_from_frames.__doc__
    assert "elvis.py:968-1224" in doc and "NOT REPRODUCED" in doc


def test_value_errors_need_no_gpu():
    f = torch.zeros((2, 16, 24, 3), dtype=torch.uint8)
    for frames, kw, msg in [
        (f, dict(block_size=12), "block_size"),
        (f, dict(block_size=0), "block_size"),
        (f, dict(order="gbr"), "order"),
        (f.float(), {}, "uint8"),
        (f.numpy(), {}, "uint8"),
        (torch.zeros((2, 16, 24, 6), dtype=torch.uint8)[..., ::2], {}, "contiguous"),
        (f, {}, "CUDA"),
    ]:
        with pytest.raises(ValueError, match=msg):
            complexity.block_complexity_device(frames, **kw)
    clip = np.zeros((2, 16, 24, 3), np.uint8)
    for frames, kw, msg in [
        (clip, dict(config=complexity.EVCAConfig(block_size=4)), "block_size"),
        (clip.astype(np.float32), {}, "uint8"),
        (np.zeros((2, 16, 24, 2), np.uint8), {}, "channels"),
        (clip, dict(config=complexity.EVCAConfig(block_size=32)), "smaller than one block"),
        (clip, dict(order="gbr"), "order"),
        (clip, dict(chunk_frames=0), "chunk_frames"),
    ]:
        with pytest.raises(ValueError, match=msg):
            complexity.analyze_frames(frames, **kw)
    empty = complexity.analyze_frames(np.zeros((0, 16, 24, 3), np.uint8))                  # no frame: no device is asked for
    assert empty.SC.shape == empty.TC.shape == (0, 1, 1) and empty.SC.dtype == np.float64


# ----------------------------------------------------------------------------- the built library
def test_library_exports_the_entry_and_the_tables_agree(built_lib):
    h = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "elvis_amd.h")).read(), flags=re.S)
    assert hasattr(h, ENTRY) and len(_lib.SIGNATURES[ENTRY]) == NARGS
    decl = re.search(r"\bint\s+" + ENTRY + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert decl and len([a for a in decl.group(1).split(",") if a.strip()]) == NARGS
    assert "complexity.hip" in _build.SOURCES
    header = open(os.path.join(ROOT, "include", "elvis_amd.h")).read()
    assert "elvis.py:968-1224" in header and "presley.py:202" in header


def test_argument_errors_without_a_gpu(built_lib):
    h = _lib.lib()

    def bad(rc, word):
        assert rc == -1 and word in h.elvis_last_error(), (rc, h.elvis_last_error())
    p = 256                                                                       # never dereferenced: every call is refused
    for block in (0, 4, 12, 64, -8):
        bad(h.elvis_block_complexity_f64(p, None, p, p, p, p, 1, 64, 64, 3, 0, block, None), b"block")
    for c in (0, 2, 4):
        bad(h.elvis_block_complexity_f64(p, None, p, p, p, p, 1, 64, 64, c, 0, 16, None), b"channels")
    bad(h.elvis_block_complexity_f64(p, None, p, p, p, p, 1, 15, 64, 3, 0, 16, None), b"bad shape")
    bad(h.elvis_block_complexity_f64(p, None, p, p, p, p, 1, 64, 31, 1, 0, 32, None), b"bad shape")
    bad(h.elvis_block_complexity_f64(p, None, p, p, p, p, -1, 64, 64, 1, 0, 8, None), b"bad shape")
    bad(h.elvis_block_complexity_f64(p, None, p, p, p, p, 1, 64, 64, 3, 2, 8, None), b"order")
    for k in range(5):                                                            # frames, dct, weight, sc, tc
        args = [p, None, p, p, p, p]
        args[k + (k > 0)] = None
        bad(h.elvis_block_complexity_f64(*args, 1, 64, 64, 3, 0, 8, None), b"null")
    assert h.elvis_block_complexity_f64(None, None, None, None, None, None, 0, 64, 64, 3, 0, 8, None) == 0     # n == 0: no-op


def test_kernel_ledger(built_lib):
    """Both directions: no kernel of complexity.hip without a case, no case naming a kernel the library lacks."""
    from _glueref import kernel_stems
    from _qualitycases import kernel_names                  # `_Z23block_complexity_kernelILi8ELi3ELi1EEv...` -> `block_complexity_kernel<8,3,1>`
    assert kernel_stems(SOURCE) == {"block_complexity_kernel"}
    built = kernel_names(built_lib, SOURCE)
    named = {c.kernel for c in R.CASES}
    assert not built - named, f"kernels of complexity.hip without a case: {sorted(built - named)}"
    assert not named - built, f"cases naming kernels the library does not build: {sorted(named - built)}"
    assert len(built) == 9
    text = open(SOURCE).read()
    assert len(re.findall(r"hipLaunchKernelGGL\(", text)) == 1 and not re.search(r"\batomic\w*\s*\(", text)
    assert '#include "i420.h"' in text and "269484" not in text                   # the hand-off's luma, not a second copy
    assert '#include "i420.h"' in open(os.path.join(ROOT, "elvis_amd", "csrc", "handoff.hip")).read()
