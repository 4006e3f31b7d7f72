"""CPU-side checks of the quality matrix (tests/_qualitycases.py, tests/test_gpu_quality_matrix.py) and of the inpaint
cases (tests/_inpaint_ref.py, tests/test_gpu_inpaint.py): the ledger (the kernels of csrc/quality.hip and
csrc/inpaint.hip in the built library are exactly the 11 + 6 the cases name), the branches the case lists must reach -
computed from the cases' numbers and the kernels' constants as the source text states them - and the discrimination
test: every mutant of the reference moves its named case by at least 1e-6, a thousand bars."""
import functools
import math
import os
import re
import time

import numpy as np
import pytest

import _inpaint_ref as R
import _qualitycases as K
import _quality_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elvis_amd", "csrc")
QUALITY, INPAINT = os.path.join(CSRC, "quality.hip"), os.path.join(CSRC, "inpaint.hip")
SSIM = K.of("ssim")


def _define(text, name):
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", text).group(1))


@functools.lru_cache(maxsize=None)
def _true(cid):
    return K.expected(K.BY_ID[cid])


@functools.lru_cache(maxsize=None)
def _inpaint_cases():
    return R.cases()


@functools.lru_cache(maxsize=None)
def _counts(name):
    return R.wave_counts(_inpaint_cases()[name][1])


def _deepest(name):
    return int(np.flatnonzero(_counts(name))[-1]) if _counts(name).any() else 0


# ------------------------------------------------------------------------------------------------------- ledger
def test_kernel_names_from_mangled_symbols():
    from _glueref import demangle_kernel, kernel_stems
    assert kernel_stems(QUALITY) == {"mask_bbox_kernel", "apply_mask_u8_kernel", "ssim_tile_kernel", "ssim_finish_kernel"}
    assert kernel_stems(INPAINT) == {"inpaint_rows_kernel", "inpaint_columns_kernel", "inpaint_scan_kernel", "inpaint_scatter_kernel",
                                     "inpaint_fill_kernel"}
    assert demangle_kernel("_Z31__device_stub__ssim_tile_kernelILi0ELi1EEv10SsimParams", kernel_stems(QUALITY)) is None


def test_kernel_ledger(built_lib):
    """Both directions: no kernel of the two sources without a case, no case naming a kernel the library lacks."""
    quality = K.kernel_names(built_lib, QUALITY)
    named = {k for c in K.CASES for k in c.kernels}
    assert not quality - named, f"kernels of quality.hip without a matrix case: {sorted(quality - named)}"
    assert not named - quality, f"cases naming kernels the library does not build: {sorted(named - quality)}"
    assert len(quality) == 11
    for border in K.BORDER_NAMES:
        assert {c.kernels[1] for c in SSIM if c.border == border} == {f"ssim_finish_kernel<{border}>"}
    text = open(QUALITY).read()
    for c in K.CASES:
        assert f'"{c.kernel}"' in text or c.kernel.startswith("apply_mask_u8_kernel<"), c.id
        if c.op == "apply":
            assert c.kernel == K.apply_launch(c.shape[3], c.offs) and f"ELVIS_APPLY_MASK({c.kernel[-2]})" in text

    inpaint = K.kernel_names(built_lib, INPAINT)
    cases = _inpaint_cases()
    prepare = {"inpaint_rows_kernel", "inpaint_columns_kernel", "inpaint_scan_kernel", "inpaint_scatter_kernel"}   # every case runs them
    named = prepare | {f"inpaint_fill_kernel<{f.shape[3]}>" for name, (f, m) in cases.items() if _deepest(name) > 0}
    assert not inpaint - named, f"kernels of inpaint.hip without a case: {sorted(inpaint - named)}"
    assert not named - inpaint, f"cases naming kernels the library does not build: {sorted(named - inpaint)}"
    assert len(inpaint) == 6
    launches = re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", open(INPAINT).read())
    assert set(launches) == prepare | {"inpaint_fill_kernel"}, "elvis_inpaint_prepare launches the four, elvis_inpaint_fill the fifth"


# ------------------------------------------------------------------------------------------------------- coverage: quality
def test_the_constants_are_the_sources():
    text = open(QUALITY).read()
    assert (_define(text, "SSIM_TH"), _define(text, "SSIM_TW"), _define(text, "SSIM_MAX_C")) == (K.TH, K.TW, K.MAX_C)
    assert "#define SSIM_ROWS (SSIM_TH + 10)" in text and "#define SSIM_COLS (SSIM_TW + 10)" in text
    assert (K.ROWS, K.COLS) == (K.TH + 10, K.TW + 10)
    assert _define(text, "BBOX_THREADS") == 1024 and "plane / 8" in text and "pixels / 16" in text
    assert "__launch_bounds__(256) void apply_mask_u8_kernel" in text and (K.BBOX_WORD, K.APPLY_GROUP, K.APPLY_THREADS) == (8, 16, 256)
    text = open(INPAINT).read()
    assert int(re.search(r"constexpr int kLocalBins = (\d+);", text).group(1)) == R.LOCAL_BINS
    assert len(re.findall(r"__launch_bounds__\((\d+)\)", text)) == 5 and set(re.findall(r"__launch_bounds__\((\d+)\)", text)) == {str(R.THREADS)}
    assert "(w + 255) / 256" in text and "(bins + 255) / 256" in text and "const int bins = h + w + 2;" in text


def test_the_ssim_cases_cover_the_branches():
    assert {c.kernel for c in SSIM} == {f"ssim_tile_kernel<{s},{b}>" for s in K.SRC_NAMES for b in K.BORDER_NAMES}
    assert all(c.shape[1] <= 70 and c.shape[2] <= 130 for c in SSIM)
    assert sum(c.shape[1] <= 48 and c.shape[2] <= 80 for c in SSIM) > 0.9 * len(SSIM)
    stag = {c.id: K.staging(c) for c in SSIM}
    for border in K.BORDER_NAMES:
        cs = [c for c in SSIM if c.border == border]
        # every channel count, staged wide and staged per pixel
        for path in ("wide", "narrow"):
            got = {c.shape[3] for c in cs if c.source == "channels" and (stag[c.id][0] if path == "wide" else stag[c.id][1])}
            assert got == {1, 2, 3, 4}, (border, path, got)
        # the shift of a staged row inside its first 4-byte word.  With c = 4 (and c = 2) an aligned tensor cannot be
        # shifted by an odd number of bytes: the three spare bytes of SSIM_RAW_PITCH are reached by c = 3 and c = 1 only
        shifts = {ch: {sh for c in cs if c.shape[3] == ch for name, sh, _ in stag[c.id][0] if name == "a"} for ch in (1, 2, 3, 4)}
        assert shifts == {1: {0, 1, 2, 3}, 2: {0, 2}, 3: {0, 1, 2, 3}, 4: {0}}, (border, shifts)
        assert {c.rects[0][2] for c in cs if c.shape[3] == 4 and c.rects and stag[c.id][0]} >= {0, 1, 2, 3}
        assert {sh for c in cs for name, sh, _ in stag[c.id][0] if name == "m"} == {0, 1, 2, 3}, border
        # a frame whose mask is shifted differently from its pixels (bpp 1 against 3), for every x0
        luma = [c for c in cs if c.source == "luma" and c.mask and c.rects and c.shape[2] % 2 and stag[c.id][0]]
        assert {c.rects[0][2] for c in luma} >= {0, 1, 2, 3}
        assert any(K.frame_shift(c, f) != K.mask_shift(c, f) for c in luma for f in range(c.shape[0]))
        # map sizes at the tile's boundaries, whole frame and inner rectangle
        for inner in (False, True):
            maps = {(K.area(c, 0)["mh"], K.area(c, 0)["mw"]) for c in cs if c.group == "tiles" and (c.rects is not None) == inner}
            assert maps == {(mh, mw) for mh in (K.TH - 1, K.TH, K.TH + 1) for mw in (K.TW - 1, K.TW, K.TW + 1)}, (border, inner)
        for c in cs:
            if c.group == "tiles" and c.rects:
                y0, y1, x0, x1 = c.rects[0]
                assert 0 < y0 and y1 < c.shape[1] and 0 < x0 and x1 < c.shape[2], f"{c.id}: strictly inside"
        # more than one tile on each axis, and a tile whose first output lies past the map (it adds nothing)
        assert any(K.area(c, 0)["mh"] > K.TH and K.area(c, 0)["mw"] > K.TW for c in cs)
        assert any(not K.area(c, 0)["degenerate"] and math.ceil(c.shape[1] / K.TH) * K.TH >= K.area(c, 0)["mh"] + K.TH for c in cs)
        # aligned == 0: by the frames, by the mask alone, by one frame alone; every offset 1..3
        off = [c for c in cs if not K.aligned(c)]
        assert {c.offs for c in off} >= {(1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 0, 1), (1, 0, 0), (0, 2, 0)}
        assert all(not stag[c.id][0] and stag[c.id][1] for c in off) and {c.shape[3] for c in off} == {1, 3, 4}
        assert {c.source for c in off} == set(K.SRC_NAMES)
        # rectangles: clipped on each side, empty, inverted, outside; a pad that eats the area and one that leaves a row
        rects = [c for c in cs if c.group == "rects"]
        assert any(c.rects[0][0] < 0 and c.rects[0][2] < 0 for c in rects)
        assert any(c.rects[0][1] > c.shape[1] and c.rects[0][3] > c.shape[2] for c in rects)
        assert any(c.rects[0][0] == c.rects[0][1] for c in rects) and any(c.rects[0][0] > c.rects[0][1] for c in rects)
        assert any(c.rects[0][0] >= c.shape[1] for c in rects) and any(c.rects[0][3] <= 0 for c in rects)
        eats = [c for c in rects if c.pad and 2 * c.pad == min(K.area(c, 0)["lh"], K.area(c, 0)["lw"])]
        assert len(eats) >= 2 and all((_true(c.id) == 1.0).all() for c in eats)
        assert any(c.pad and 2 * c.pad == min(K.area(c, 0)["lh"], K.area(c, 0)["lw"]) - 1 and K.area(c, 0)["mh"] == 1 for c in rects)
        for c in rects:
            assert (_true(c.id) == 1.0).all() == K.area(c, 0)["degenerate"], c.id
        # a batch of three different rectangles and masks, for both sources
        batch = [c for c in cs if c.group == "batch"]
        assert {c.source for c in batch} == set(K.SRC_NAMES)
        for c in batch:
            assert c.shape[0] == 3 and len(set(c.rects)) == 3
            m = K.inputs(c)[2]
            assert not np.array_equal(m[0], m[1]) and not np.array_equal(m[1], m[2])
            assert len({float(v) for v in _true(c.id)[:, 0]}) == 3
    # the tensor-end fallback: a staged word crosses the end of a tensor whose size is no multiple of 4
    ends = [c for c in SSIM if any(cross for _, _, cross in stag[c.id][0])]
    assert {c.shape for c in ends} >= {(1, 27, 42, 3), (1, 27, 42, 1)}
    assert all(int(np.prod(c.shape)) % 4 for c in ends if c.shape[3] != 1 or not c.mask)
    assert any(cross for c in ends if c.mask for name, _, cross in stag[c.id][0] if name == "m"), "the mask's last word too"
    assert (27 * 42 * 3, 27 * 42 * 3 % 4, 27 * 42 % 4) == (3402, 2, 2)
    # VALID: each side of the smoothing threshold on each axis, both sides below it, a short side over several tiles
    thr = {(c.shape[1], c.shape[2]) for c in SSIM if c.group == "threshold" and c.rects is None}
    assert thr >= {(10, 40), (12, 40), (40, 9), (40, 10), (9, 70), (70, 9), (10, 10), (12, 12)}
    for axis in (0, 1):
        assert {s[axis] for s in thr} >= {9, 10, 11, 12} and {s[axis] >= 11 for s in thr if s[1 - axis] < 11} == {True, False}
    assert all(c.window == "asym" and c.border == "valid" for c in SSIM if c.group == "threshold")
    assert any(c.shape[1] < 11 and c.shape[2] - 10 > K.TW for c in SSIM if c.group == "threshold")
    assert any(c.shape[2] < 11 and c.shape[1] - 10 > K.TH for c in SSIM if c.group == "threshold")
    # the automatic rule: every smallest side 2..8, the short side on either axis; 1.0 below 3
    auto = [c for c in SSIM if c.pad is None and c.group == "auto"]
    for axis in ("lh", "lw"):
        assert {K.area(c, 0)[axis] for c in auto if K.area(c, 0)[axis] == min(K.area(c, 0)["lh"], K.area(c, 0)["lw"])} >= set(range(2, 9))
    for c in auto:
        g = K.area(c, 0)
        side = min(g["lh"], g["lw"])
        assert g["degenerate"] == (side < 3) and ((_true(c.id) == 1.0).all()) == (side < 3), c.id
        assert side < 3 or g["pad"] == {3: 1, 4: 1, 5: 2, 6: 2, 7: 3, 8: 3}[side]
    assert {c.window for c in SSIM} == {"gaussian", "msssim", "asym"}
    assert {(c.border, c.window) for c in SSIM if c.window == "asym"} == {("reflect", "asym"), ("valid", "asym")}
    # the constants are the two evaluators' own, so the bar's derivation applies as written
    assert {(c.scale, c.constants) for c in SSIM} == {(1.0, (Q.C1_255, Q.C2_255)), (255.0, (0.01 ** 2, 0.03 ** 2))}
    for kind in ("gaussian", "msssim", "asym"):
        w = K.window(kind)
        assert w.shape == (11,) and (w >= 0).all() and abs(w.sum() - 1.0) < 1e-7
    w = K.window("asym")
    assert w.sum() == 1.0 and (np.diff(w) > 0).all() and w.dtype == np.float64


def test_the_bbox_and_apply_cases_cover_the_branches():
    bb = K.of("bbox")
    big = 1024 * K.BBOX_WORD + K.BBOX_WORD + 3
    assert {c.shape[1] * c.shape[2] for c in bb} >= {1, 7, 8, 9, big}
    assert {c.mask for c in bb} == set(K.BBOX_KINDS)
    assert {c.offs[0] for c in bb} == set(range(8))
    n3 = [c for c in bb if c.shape[0] == 3 and (c.shape[1] * c.shape[2]) % K.BBOX_WORD]
    assert n3 and all((f * c.shape[1] * c.shape[2] + c.offs[0]) % K.BBOX_WORD for c in n3 for f in (1, 2)) and all(c.offs[0] == 0 for c in n3)
    values = set()
    for c in bb:
        m, = K.inputs(c)
        n, h, w, _ = c.shape
        flat = m.reshape(n, -1)
        values |= set(np.unique(m).tolist())
        want = _true(c.id)
        if c.mask == "first":
            assert flat[0, 0] and tuple(want[0]) == (0, 1, 0, 1)
        if c.mask == "last":
            assert flat[0, -1] and tuple(want[0]) == (h - 1, h, w - 1, w)
        if c.mask == "byte7" and h * w >= 16:
            i, = np.flatnonzero(flat[0])
            assert i % 8 == 7 and (i - 7) // w != i // w, f"{c.id}: byte 7 of a word that straddles two rows"
        if c.mask == "tail" and (h * w) % 8:
            i, = np.flatnonzero(flat[0])
            assert i >= (h * w) // 8 * 8
        if c.mask == "empty_middle":
            assert flat[0].any() and not flat[1].any() and flat[2].any() and tuple(want[1]) == (0, 0, 0, 0)
        if c.mask == "empty":
            assert not want.any()
    assert values == {0, 1, 2, 128, 255}

    ap = K.of("apply")
    px = set(K.APPLY_PIXELS)
    assert px == {1, 15, 16, 17, K.APPLY_GROUP * K.APPLY_THREADS + 5}
    for c in (1, 2, 3, 4, 5):
        for offs in ((0, 0, 0), (1, 1, 1)):
            hit = [k for k in ap if k.shape[3] == c and k.offs == offs]
            assert {k.shape[0] * k.shape[1] * k.shape[2] for k in hit} >= px
            assert {(k.shape[1] * k.shape[2], k.invert) for k in hit} >= {(p, i) for p in px for i in (False, True)}
    assert {k.kernel[-2] for k in ap if k.offs == (0, 0, 0)} == {"0", "1", "3", "4"}
    assert all(k.kernel.endswith("<0>") for k in ap if any(o % 16 for o in k.offs))
    assert {k.shape[3] for k in ap if k.kernel.endswith("<0>") and any(o % 16 for o in k.offs)} == {1, 2, 3, 4, 5}
    for one in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        assert any(k.offs == one and k.shape[3] == 3 for k in ap), "each of the three tensors alone decides the dispatch"
    assert any(all(o and o % 16 == 0 for o in k.offs) and k.kernel.endswith("<3>") for k in ap)
    assert any(k.shape[0] > 1 for k in ap)
    for k in ap:
        out = _true(k.id)
        assert (out == 0).any() and (out != 0).any() or k.shape[1] * k.shape[2] == 1, k.id


# ------------------------------------------------------------------------------------------------------- coverage: inpaint
def test_the_inpaint_cases_cover_the_preparation_branches():
    cases = _inpaint_cases()
    prep = R.preparation_cases()
    bins = {name: f.shape[1] + f.shape[2] + 2 for name, (f, m) in cases.items()}
    deepest = {name: _deepest(name) for name in cases}
    assert max(deepest[k] for k in cases if k not in prep) == R.LOCAL_BINS - 1, "before: one short of the global-atomic path"
    assert any(d > R.LOCAL_BINS for d in deepest.values())
    exact = [k for k, d in deepest.items() if d == R.LOCAL_BINS]
    assert exact and all(_counts(k)[R.LOCAL_BINS] == 1 for k in exact), "exactly one pixel on the global-atomic path"
    assert deepest["row_1x64"] == R.LOCAL_BINS - 1 and deepest["row_1x65"] == R.LOCAL_BINS
    assert {math.ceil(f.shape[2] / R.THREADS) for f, m in cases.values()} >= {1, 2, 3}
    assert {math.ceil(b / R.THREADS) for b in bins.values()} >= {1, 2} and {256, 257} <= set(bins.values())
    assert any(f.shape[1] == 1 and deepest[k] > 0 for k, (f, m) in cases.items())
    assert any(f.shape[2] == 1 and deepest[k] > 0 for k, (f, m) in cases.items())
    # a row without a known pixel in a frame that has known pixels: its row distance is kNoDist
    assert any(((m[i] != 0).all(axis=1).any() and not (m[i] != 0).all()) for k, (f, m) in prep.items() for i in range(len(m)))
    # a known pixel in the middle of a thread's run, a run that is all hole between known neighbours, empty trailing runs
    f, m = cases["row_1x300_mid"]
    chunk = math.ceil(300 / R.THREADS)
    x, = np.flatnonzero(m[0, 0] == 0)
    assert chunk == 2 and x % chunk == 1
    f, m = cases["wide_3x513"]
    chunk = math.ceil(513 / R.THREADS)
    known = np.flatnonzero(m[0, 1] == 0)
    runs = {int(k) // chunk for k in known}
    assert chunk == 3 and {int(k) % chunk for k in known} == {0, 1, 2}
    assert any(t not in runs for t in range(min(runs), max(runs))), "an all-hole run between known neighbours"
    assert math.ceil(513 / chunk) < R.THREADS and math.ceil(257 / 2) < R.THREADS, "trailing threads own empty runs"
    # two frames of one clip add to the same wave >= kLocalBins
    f, m = cases["deep_70x40"]
    per = [R.wave_counts(m[i:i + 1]) for i in range(2)]
    shared = [k for k in range(R.LOCAL_BINS, len(per[0])) if per[0][k] and per[1][k]]
    assert shared and np.array_equal(per[0] + per[1], _counts("deep_70x40"))
    assert {cases[k][0].shape[3] for k in ("deep_70x40", "deep_70x40_c1")} == {1, 3}
    # the counts' own shape: nothing in wave 0, nothing past the deepest wave, every hole pixel of a fillable frame listed
    for name, (f, m) in cases.items():
        c = _counts(name)
        fillable = [i for i in range(len(m)) if (m[i] != 0).any() and not (m[i] != 0).all()]
        assert c[0] == 0 and c.sum() == sum(int((m[i] != 0).sum()) for i in fillable) and len(c) == bins[name], name


# ------------------------------------------------------------------------------------------------------- discrimination
@pytest.mark.parametrize("mutant", sorted(K.MUTANTS))
def test_every_quality_mutant_moves_its_case_by_a_thousand_bars(mutant):
    case = K.BY_ID[K.MUTANTS[mutant]]
    d = np.abs(K.expected(case, mutant) - _true(case.id)).max()
    assert math.isclose(1e-6, 1000 * K.BAR) and d >= 1e-6, f"{mutant} on {case.id}: {d:.3e}"
    assert case.shape[1] * case.shape[2] <= 48 * 80
    if mutant == "edge_clamp":
        assert min(K.area(case, 0)["lh"], K.area(case, 0)["lw"]) < 5
    if mutant == "mask_at_frame_shift":
        assert any(K.frame_shift(case, f) != K.mask_shift(case, f) for f in range(case.shape[0]))
    if mutant in ("windows_swapped", "valid_from_minus_5"):
        assert case.border == "valid" and case.window == "asym"
    if mutant == "win_4_as_5":
        assert min(K.area(case, 0)["lh"], K.area(case, 0)["lw"]) == 4
    if mutant == "map_row_more":
        assert K.area(case, 0)["pad"] >= 1


def test_the_symmetric_windows_cannot_see_a_reversed_window():
    """Why the asym window exists: on a case with the Gaussian the reversed-window mutant is the reference itself."""
    case = K.BY_ID["tile_15x31_reflect"]
    assert case.window == "gaussian" and np.abs(K.expected(case, "window_reversed") - _true(case.id)).max() < 1e-12


def test_the_inpaint_mutants_still_differ():
    assert len(R.MUTANTS) == 7
    cases = R.mutant_cases()
    for mutant, name in R.MUTANTS.items():
        frames, masks = cases[name]
        assert not np.array_equal(R.inpaint(frames, masks, mutant=mutant), R.inpaint(frames, masks)), mutant


# ------------------------------------------------------------------------------------------------------- pins
def test_the_kernel_model_equals_the_reference():
    """The mutants change one clause of `_model_mean`, the reference written the way the kernel indexes; without a mutant
    it is Q.ssim_mean (to the order of the final sum)."""
    for c in SSIM:
        assert np.abs(K.expected(c, "none") - _true(c.id)).max() <= 1e-14, c.id


def test_expected_agrees_with_the_evaluators_where_a_case_is_one():
    done = 0
    for c in SSIM:
        a, b, m = K.inputs(c)
        g = [K.area(c, f) for f in range(c.shape[0])]
        if c.source == "luma" and c.border == "reflect" and c.pad is None and c.window == "gaussian":
            for f in range(c.shape[0]):          # masked_ssim on the crop, the mask cropped with it (its own box may be smaller)
                y0, x0, lh, lw = g[f]["y0"], g[f]["x0"], g[f]["lh"], g[f]["lw"]
                if lh <= 0 or lw <= 0:
                    continue
                ca, cb = a[f, y0:y0 + lh, x0:x0 + lw], b[f, y0:y0 + lh, x0:x0 + lw]
                if m is None:
                    want = Q.masked_ssim_taps(ca, cb, None)
                else:
                    cm = m[f, y0:y0 + lh, x0:x0 + lw]
                    if Q.mask_bbox(cm) != (0, lh, 0, lw):
                        continue
                    want = Q.masked_ssim_taps(ca, cb, cm)
                assert abs(_true(c.id)[f, 0] - want) <= 1e-15, c.id
                done += 1
        if c.source == "channels" and c.border == "valid" and c.pad == 0 and c.window == "msssim" and c.rects is None and m is None:
            for f in range(c.shape[0]):
                assert abs(_true(c.id)[f].mean() - Q.msssim_ssim(a[f], b[f])) <= 1e-15, c.id
                done += 1
    assert done >= 12


# ------------------------------------------------------------------------------------------------------- cost
def test_the_references_of_the_new_cases_are_cheap():
    t = time.perf_counter()
    for c in K.CASES:
        K.expected(c)
    quality = time.perf_counter() - t
    t = time.perf_counter()
    for frames, masks in R.preparation_cases().values():
        R.inpaint(frames, masks)
        R.wave_counts(masks)
    inpaint = time.perf_counter() - t
    print(f"expected values: quality {quality:.2f} s for {len(K.CASES)} cases, inpaint {inpaint:.2f} s for {len(R.preparation_cases())}")
    assert quality + inpaint < 60.0
