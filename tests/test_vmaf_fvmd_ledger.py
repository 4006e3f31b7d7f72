"""CPU-side checks of the VMAF and FVMD matrices (tests/_vmafcases.py, tests/_fvmdcases.py and the two
test_gpu_*_matrix.py files): the ledger (the kernels of csrc/vmaf.hip and csrc/fvmd.hip in the built library are exactly
the 14 + 12 the cases name), the branches the case lists must reach - computed from the cases' numbers and the kernels'
constants as the source text states them - the condition on the VMAF inputs (no pixel within 1e-6 of the one
discontinuous branch), and the discrimination test: every mutant of the two statements moves its named case by at least
1e-6, a thousand bars."""
import math
import os
import re
import time

import numpy as np
import pytest

import _fvmd_ref as FR
import _fvmdcases as F
import _vmaf_ref as VR
import _vmafcases as V
from _qualitycases import kernel_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elvis_amd", "csrc")
VMAF, FVMD, FVMD_INDEX = (os.path.join(CSRC, n) for n in (V.SOURCE, F.SOURCE, "fvmd_index.h"))


def _define(text, name):
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", text).group(1))


# ------------------------------------------------------------------------------------------------------- ledger
def test_kernel_ledger(built_lib):
    """Both directions: no kernel of the two sources without a case, no case naming a kernel the library lacks."""
    vmaf = kernel_names(built_lib, VMAF)
    groups = V.group_kernels()
    assert set(groups) == {"passes", "neighbours", "shapes", "values", "predict", "luma"} and all(groups.values())
    assert groups["predict"] == ("vmaf_predict_kernel",) and groups["luma"] == ("vmaf_luma_kernel",)
    named = {k for ks in groups.values() for k in ks}
    assert not vmaf - named, f"kernels of vmaf.hip without a matrix case: {sorted(vmaf - named)}"
    assert not named - vmaf, f"cases naming kernels the library does not build: {sorted(named - vmaf)}"
    assert len(vmaf) == 14
    assert {k for k in vmaf if "vif_stat" in k} == {f"vmaf_vif_stat_kernel<{n}>" for n in VR.VIF_TAPS}
    assert {k for k in vmaf if "vif_down" in k} == {f"vmaf_vif_down_kernel<{n}>" for n in VR.VIF_TAPS[1:]}
    assert {k for k in vmaf if "dwt" in k} == {"vmaf_dwt_kernel<true>", "vmaf_dwt_kernel<false>"}
    text = open(VMAF).read()
    for noted in V.NOTED.values():                    # the names the GPU file compares elvis_last_launch with are the ones the source notes
        assert f'elvis_note_launch("{noted}")' in text and noted in named

    fvmd = kernel_names(built_lib, FVMD)
    groups = F.group_kernels()
    assert set(groups["jacobi"]) == {"fvmd_jacobi_lds_kernel", "fvmd_jacobi_round_kernel", "fvmd_norm_kernel"}
    assert set(groups) == {"jacobi", "frechet", "hist", "gram", "tracker"} and all(groups.values())
    named = {k for ks in groups.values() for k in ks}
    assert not fvmd - named, f"kernels of fvmd.hip without a matrix case: {sorted(fvmd - named)}"
    assert not named - fvmd, f"cases naming kernels the library does not build: {sorted(named - fvmd)}"
    assert len(fvmd) == 12
    text = open(FVMD).read()
    for k in named:                                   # every name a GPU test compares elvis_last_launch with is one the source notes
        stem = k.split("<")[0]
        assert f"hipLaunchKernelGGL({stem}" in text, k
    for noted in ("fvmd_jacobi_lds_kernel", "fvmd_jacobi_round_kernel", "fvmd_finish_kernel", "fvmd_hist_kernel", "fvmd_gram_kernel",
                  "fvmd_track_kernel"):
        assert f'elvis_note_launch("{noted}")' in text


def test_the_constants_are_the_sources():
    text = open(VMAF).read()
    assert (_define(text, "VMAF_PASS_FRAMES"), _define(text, "VMAF_TH"), _define(text, "VMAF_TW"), _define(text, "VMAF_AT")) == \
        (V.PASS_FRAMES, V.TH, V.TW, V.AT) == (VR.PASS_FRAMES, VR.TILE_H, V.TW, V.AT)
    assert (_define(text, "VMAF_MIN_SIDE"), _define(text, "VMAF_THREADS")) == (V.MIN_SIDE, V.THREADS) and VR.MIN_SIDE == V.MIN_SIDE
    assert "for (int f0 = 0; f0 < n; f0 += VMAF_PASS_FRAMES)" in text and "(int)(p.aw[s] * 0.1 - 0.5)" in text
    assert "blockIdx.x * (VMAF_THREADS / ELVIS_WAVE)" in text and "g = fmin(g, 100.0);" in text and "if (s1 >= nsq)" in text
    text = open(FVMD).read()
    index = open(FVMD_INDEX).read()
    assert (_define(index, "FVMD_LDS_DOUBLES"), _define(index, "FVMD_MAX_ROWS")) == (F.LDS_DOUBLES, F.MAX_ROWS)
    assert (_define(index, "FVMD_MIN_SEQ"), _define(index, "FVMD_MAX_SEQ")) == (F.MIN_SEQ, F.MAX_SEQ) == (FR.seq_len_of(0), FR.seq_len_of(99))
    assert (_define(text, "FVMD_TILE"), _define(text, "FVMD_THREADS"), _define(text, "FVMD_SWEEPS")) == (F.TILE, F.THREADS, F.SWEEPS)
    assert "(long long)k * len <= FVMD_LDS_DOUBLES" in text and F.OPT_IN_DOUBLES * 8 == 64 << 10 and F.LDS_DOUBLES * 8 == 128 << 10
    assert (_define(index, "FVMD_BINS"), _define(index, "FVMD_POINTS"), _define(index, "FVMD_CELLS")) == (FR.BINS, FR.POINTS, FR.CELLS)


# ------------------------------------------------------------------------------------------------------- pins
def _recorded(golden_dir, key, got):
    """Against tests/golden/vmaf_fvmd_statement.npz, written by the statements as they were before they took `mutant=`
    and `counts=` (tools/make_vmaf_fvmd_statement_golden.py regenerates and checks it): the same bytes."""
    want = np.load(os.path.join(golden_dir, "vmaf_fvmd_statement.npz"))[key]
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, key
    worst = float(np.abs(got - want).max())
    assert got.tobytes() == want.tobytes(), f"{key}: not the recorded bytes, worst |difference| = {worst:.3g}"


def test_without_a_mutant_the_statements_are_what_they_were(golden_dir):
    """The `mutant=` and `counts=` arguments are additions: the existing fixtures give what they gave before (recorded),
    the same bytes with and without the arguments, and an unknown mutant is refused."""
    for shape in VR.SHAPES[:3]:
        _recorded(golden_dir, f"vmaf_{shape[0]}x{shape[1]}", VR.expected(*shape))
    _recorded(golden_dir, "vmaf_branch_pair", VR.features(*VR.branch_pair()))
    _recorded(golden_dir, "fvmd_border_64_rows", FR.tracked("border_64")["rows"])
    _recorded(golden_dir, "fvmd_border_static_gram", FR.expected_distance("border_64", "static_64")["gram"])
    _recorded(golden_dir, "fvmd_border_static_scalars", FR.expected_distance("border_64", "static_64")["scalars"])
    for shape in VR.SHAPES[:3]:
        ref, dis = VR.fixture(*shape)
        want = VR.expected(*shape)
        assert np.array_equal(VR.features(ref, dis, mutant=None), want)
        assert np.array_equal(VR.features(ref, dis, counts=VR.new_counts()), want)
        assert np.array_equal(VR.vif(ref, dis), want[:, 2:]) and np.array_equal(VR.adm(ref, dis), want[:, 0])
        assert np.array_equal(VR.motion(ref)[1], want[:, 1])
    ref, dis = VR.branch_pair()
    assert np.array_equal(VR.features(ref, dis, counts=VR.new_counts()), VR.features(ref, dis))
    for name in ("border_64", "static_64"):
        t = FR.tracked(name)
        assert np.array_equal(FR.features(t["tracks"], counts=FR.new_counts()), t["rows"])
        assert np.array_equal(FR.features(t["tracks"], mutant=None), t["rows"])
    want = FR.expected_distance("border_64", "static_64")
    gram, scalars = FR.gram_parts(FR.tracked("border_64")["rows"], FR.tracked("static_64")["rows"], mutant=None)
    assert np.array_equal(gram, want["gram"]) and np.array_equal(scalars, want["scalars"])
    with pytest.raises(ValueError, match="unknown mutant"):
        VR.features(*VR.fixture(64, 64), mutant="no_such")
    with pytest.raises(ValueError, match="unknown mutant"):
        FR.features(FR.tracked("static_64")["tracks"], mutant="no_such")
    old = {"s1_below_eps", "s2_below_eps", "gain_negative", "log_term", "flat_term", "low_term", "adm_flag_set", "adm_flag_clear"}
    assert old < set(VR.new_counts()) and all(VR.new_counts()[k] == [0, 0, 0, 0] for k in old)


def test_the_jacobi_model_is_the_kernels_pairing_and_converges():
    """The pairing of the model is fvmd_pair's: every two vectors meet once per sweep.  In the model, 16 sweeps bring every
    size of the matrix to numpy's singular values - so a miss on the device is the kernel's, not the method's."""
    for K in (2, 4, 10, 130):
        met = set()
        for r in range(K - 1):
            i, j = F.pairing(r, K)
            assert sorted(np.concatenate([i, j]).tolist()) == list(range(K))
            met |= {frozenset(p) for p in zip(i.tolist(), j.tolist())}
        assert len(met) == K * (K - 1) // 2
    text = open(FVMD_INDEX).read()
    assert "*i = (r + p) % m;" in text and "*j = (r - p + m) % m;" in text and "*i = m;" in text and "*j = r;" in text
    for k, ln in F.JACOBI:
        if k * ln > F.LDS_DOUBLES // 2 and (k, ln) != (129, 128):
            continue                                  # the model of the largest sizes costs seconds; one of each path is enough
        got, last = F.jacobi_model(F.jacobi_matrix(k, ln))
        got = np.sort(got)[::-1]
        want = F.jacobi_expected(k, ln)
        r = min(k, ln)
        worst = float((np.abs(got[:r] - want) / np.maximum(1.0, want)).max())
        print(f"jacobi model {k} x {ln}: worst {worst:.3g}, tail {np.abs(got[r:]).max(initial=0.0):.3g}, rotations in sweep 16: {last}")
        assert worst <= F.BAR and np.abs(got[r:]).max(initial=0.0) <= F.BAR * max(1.0, got[0])


# ------------------------------------------------------------------------------------------------------- coverage: VMAF
def test_the_vmaf_cases_cover_the_passes_and_neighbours():
    passes = [V.case_plan(c)["passes"] for c in V.of("passes")]
    assert {len(p) for p in passes} == {2, 3} and {p[-1] for p in passes} == {1, 2, 4}
    assert all(p[:-1] == [V.PASS_FRAMES] * (len(p) - 1) for p in passes)
    assert {(c.h, c.w, c.n) for c in V.of("passes")} == {(64, 64, 5), (64, 64, 8), (64, 64, 9), (66, 70, 6)}
    for c in V.of("passes"):
        ref, dis, prev, nxt = V.inputs(c.id)
        assert prev is None and nxt is None
        assert np.array_equal(ref, VR.fixture(c.h, c.w, c.n)[0]) and np.array_equal(dis, VR.fixture(c.h, c.w, c.n)[1])
        want = V.expected(c.id)
        assert len({float(v) for v in want[:, 2]}) == c.n, "every frame differs, so a frame read from the wrong place shows"
    nb = V.of("neighbours")
    assert {(c.n, c.prev, c.following) for c in nb} == {(n, p, f) for n in (1, 5) for p in (False, True) for f in (False, True)}
    for n in (1, 5):
        m2 = {(c.prev, c.following): V.expected(c.id)[:, 1] for c in nb if c.n == n}
        # without `prev` the motion of frame 0 is 0, and so is its minimum with whatever follows: with one frame
        # `following` alone changes nothing, with five it changes the last frame
        assert len({tuple(v) for v in m2.values()}) == (3 if n == 1 else 4), "the variants give different motion2 columns"
        assert m2[False, False][0] == 0.0 and m2[False, True][0] == 0.0 and m2[True, True].min() > 0.0
        assert m2[True, False][-1] != m2[True, True][-1]
    assert all(len(V.case_plan(c)["passes"]) == (2 if c.n == 5 else 1) for c in nb)


def test_the_vmaf_cases_cover_the_tile_edges_and_the_window_steps():
    shapes = V.of("shapes")
    assert {c.h for c in shapes} == set(V.SIDES) == {c.w for c in shapes}
    assert sum(c.h != c.w for c in shapes) == len(shapes) and all(max(c.h, c.w) <= 130 for c in V.CASES)
    plans = [V.case_plan(c) for c in shapes]
    vh = {s[0] for p in plans for s in p["vif"]}
    vw = {s[1] for p in plans for s in p["vif"]}
    sides = {13, 15, 16, 27, 30, 31, 32, 55, 60, 63, 64}
    assert sides <= vh and sides <= vw, (sorted(vh), sorted(vw))
    ah = {s[0] for p in plans for s in p["adm"]}
    aw = {s[1] for p in plans for s in p["adm"]}
    bands = {4, 5, 7, 8, 9, 14, 15, 16, 17, 28, 30, 32, 33, 56, 60, 64, 65}
    assert bands <= ah and bands <= aw, (sorted(ah), sorted(aw))
    # tile-relative sizes: one under, on and one over a multiple of each tile side, and the exact sides at scales 1 to 3
    assert {v % V.TH for v in vh} >= {V.TH - 1, 0, 1} and {v % V.TW for v in vw} >= {V.TW - 1, 0, 1}
    later_h = {s[0] for p in plans for s in p["vif"][1:]}
    later_w = {s[1] for p in plans for s in p["vif"][1:]}
    assert {V.TH - 1, V.TH, 2 * V.TH - 1, 2 * V.TH} <= later_h and {V.TW - 1, V.TW, 2 * V.TW - 1, 2 * V.TW} <= later_w
    assert {V.AT - 1, V.AT, V.AT + 1, 2 * V.AT, 2 * V.AT + 1} <= ah and {V.AT - 1, V.AT, V.AT + 1, 2 * V.AT, 2 * V.AT + 1} <= aw
    # both sides of each rounding step of the window, on each axis
    top = {s[0]: s[2] for p in plans for s in p["adm"]}
    left = {s[1]: s[3] for p in plans for s in p["adm"]}
    for edge in (top, left):
        assert (edge[14], edge[15], edge[64], edge[65]) == (0, 1, 5, 6)
        assert set(edge.values()) >= {0, 1, 2, 5, 6}
    assert any(s[2] != s[3] for p in plans for s in p["adm"]), "a window whose top and left differ: a swapped axis shows"
    # the motion and scale-0 tiles: more than one tile on each axis, ragged on each
    assert any(c.h > 4 * V.TH and c.h % V.TH and c.w > 2 * V.TW and c.w % V.TW for c in shapes)


def test_the_vmaf_value_cases_reach_their_branches():
    k = {c.content: V.counts(c.id) for c in V.of("values")}
    assert set(k) == {"zero_full", "full_full", "checker", "flat_ref", "branch"}
    for content in ("zero_full", "full_full"):
        assert all(v > 0 for v in k[content]["s1_below_eps"]) and all(v > 0 for v in k[content]["s2_below_eps"])
        assert all(v > 0 for v in k[content]["sv_floored"]) and k[content]["log_term"] == [0, 0, 0, 0]
    n, h, w = 2, 64, 65
    assert k["checker"]["adm_dp_negative"][0] == n * ((h + 1) // 2) * ((w + 1) // 2), "dp < 0 at every pixel of the first band"
    assert k["checker"]["gain_negative"][0] == n * h * w and k["checker"]["adm_flag_set"][0] == 0
    assert all(v > 0 for v in k["flat_ref"]["adm_o_zero"]) and all(v > 0 for v in k["flat_ref"]["s1_below_eps"])
    assert k["flat_ref"]["log_term"] == [0, 0, 0, 0]
    assert all(v > 0 for v in k["branch"]["s2_below_eps"]) and all(v > 0 for v in k["branch"]["gain_negative"])
    c = V.BY_ID["value_branch_67x81"]
    assert c.h != c.w and c.h % V.TH and c.w % V.TW and c.h % 2 and c.w % 2
    assert np.abs(V.expected("value_full_full")[:, 0] - 1.0).max() <= 1e-12 and np.abs(V.expected("value_full_full")[:, 2:] - 1.0).max() <= 1e-12
    for c in V.CASES:
        assert np.isfinite(V.expected(c.id)).all(), c.id
    every = {key: [sum(V.counts(c.id)[key][s] for c in V.CASES) for s in range(4)] for key in
             ("s1_below_eps", "s2_below_eps", "gain_negative", "log_term", "low_term", "adm_flag_set", "adm_flag_clear", "sv_floored",
              "adm_dp_negative", "adm_o_zero")}
    assert all(v > 0 for vs in every.values() for v in vs), every


def test_no_vmaf_input_comes_near_the_discontinuous_branch():
    """|s1 - nsq| / nsq >= 1e-6 at every pixel of every scale of every case: a thousand bars from the step between the
    two terms, so the device and the statement fall the same way.  The gain clamp cannot act on 8-bit input: where the
    log term is taken s1 >= 2 and s2 <= 128^2, so g <= sqrt(s2 / s1) <= 90.6 < 100."""
    worst, gain = math.inf, 0.0
    for c in V.CASES:
        assert V.margin(c.id) >= V.MARGIN, (c.id, V.margin(c.id))
        worst, gain = min(worst, V.margin(c.id)), max(gain, max(V.counts(c.id)["max_gain_log"]))
    print(f"smallest |s1 - nsq| / nsq over {len(V.CASES)} cases: {worst:.3g}; largest gain in the log term: {gain:.3g}")
    assert gain < VR.GAIN_LIMIT and math.sqrt(128.0 ** 2 / VR.NSQ) < 90.6 < VR.GAIN_LIMIT


def test_the_predict_and_luma_cases_cover_the_blocks():
    assert V.PREDICT_FLAGS == tuple(range(8)) and V.PREDICT_NSV == (1, V.WAVE - 1, V.WAVE, V.WAVE + 1)
    assert [V.predict_waves(n) for n in V.PREDICT_N] == [(1, 1), (1, 4), (2, 1)]
    from elvis_amd import vmaf
    for nsv in V.PREDICT_NSV:
        moved = {1: False, 2: False, 4: False}
        for flags in V.PREDICT_FLAGS:
            m = vmaf.VmafModel(**V.predict_model_fields(nsv, flags))
            assert m.flags == flags and m.sv.shape == (nsv, 6)
            for bit in (1, 2, 4):
                if flags & bit:
                    other = vmaf.VmafModel(**{**V.predict_model_fields(nsv, flags), **{
                        1: dict(enable_transform=False), 2: dict(transform=m.transform[:3] + (False,)), 4: dict(score_clip=None)}[bit]})
                    for n in V.PREDICT_N:
                        f = V.predict_features(n)
                        moved[bit] |= bool(np.abs(VR.score(f, m) - VR.score(f, other)).max() >= 1e-6)
        assert all(moved.values()), (nsv, moved)
    assert set(V.luma_pixels()) >= {1, V.THREADS - 1, V.THREADS, V.THREADS + 1}
    rects = [r for _, rs in V.LUMA for r in rs]
    assert any(r[1] - r[0] == 1 and r[3] - r[2] == V.THREADS + 1 for r in rects)
    assert any(r[3] - r[2] == 1 and r[1] - r[0] == V.THREADS + 1 for r in rects)
    for shape, rs in V.LUMA:
        assert all(0 <= r[0] < r[1] <= shape[1] and 0 <= r[2] < r[3] <= shape[2] for r in rs)
        frames, masks = V.luma_inputs(shape)
        assert (masks == 0).any() and (masks != 0).any() and len(np.unique(frames)) == 256


# ------------------------------------------------------------------------------------------------------- coverage: FVMD
def test_the_jacobi_cases_cover_the_lds_boundaries():
    sizes = {k * ln for k, ln in F.JACOBI}
    assert {F.OPT_IN_DOUBLES, F.LDS_DOUBLES, F.LDS_DOUBLES - 1} <= sizes
    assert F.OPT_IN_DOUBLES + 128 in sizes and (65, 128) in F.JACOBI, "one vector of 128 past 64 KiB"
    assert min(s for s in sizes if s > F.LDS_DOUBLES) == F.LDS_DOUBLES + 128 and (129, 128) in F.JACOBI
    assert any(F.OPT_IN_DOUBLES < k * ln < F.LDS_DOUBLES and k == ln for k, ln in F.JACOBI)
    lds = [s for s in F.JACOBI if F.jacobi_kernels(*s) == ("fvmd_jacobi_lds_kernel",)]
    rounds = [s for s in F.JACOBI if s not in lds]
    grams = {(min(n, m), max(n, m)) for n, m, _ in F.FRECHET}                # _frechet_tensor rotates the fewer vectors
    rounds += [g for g in grams if F.jacobi_kernels(*g) != ("fvmd_jacobi_lds_kernel",)]
    assert {k % 2 for k, _ in lds} == {0, 1} == {k % 2 for k, _ in rounds}
    assert any(k > ln for k, ln in lds) and any(k > ln for k, ln in rounds) and any(k < ln for k, ln in lds) and any(k < ln for k, ln in rounds)
    assert any(k > 4 * ln for k, ln in lds) and any(ln > 4 * k for k, ln in lds)
    assert (F.TILE, F.MAX_ROWS) in F.JACOBI and (F.MAX_ROWS, F.TILE) in F.JACOBI and F.TILE * F.MAX_ROWS == F.LDS_DOUBLES
    assert all(k <= F.MAX_ROWS and ln <= F.MAX_ROWS for k, ln in F.JACOBI)
    assert {F.jacobi_kernels(*g)[0] for g in grams} == {"fvmd_jacobi_lds_kernel", "fvmd_jacobi_round_kernel"}
    assert (128, 128) in grams and (128, 129) in grams and all(d == 384 for _, _, d in F.FRECHET)
    assert all(F.FRECHET_JACOBI[s] == F.jacobi_kernels(min(s[:2]), max(s[:2]))[0] for s in F.FRECHET) and len(F.FRECHET_JACOBI) == len(F.FRECHET)
    for shape in F.FRECHET:
        a, b = F.frechet_rows(*shape)
        assert FR.frechet(a, b) > 0.1 * FR.fd_scale(a, b), "a distance that is not all cancellation"


def test_the_histogram_cases_cover_the_boundaries():
    counts = {name: F.hist_counts(name) for name in F.HIST}
    assert {(b, s) for b, s, _ in F.HIST.values()} >= {(1, F.MIN_SEQ), (3, F.MIN_SEQ), (1, F.MAX_SEQ), (3, F.MAX_SEQ)}
    for k in range(FR.BINS):
        assert counts["axes_S10_B1"]["boundary"][k] > 0 and counts["mixed_S16_B3"]["boundary"][k] > 0, k
        ang = math.atan2(F.DIRECTIONS[k][1], F.DIRECTIONS[k][0]) / FR.QUARTER_PI
        assert (ang + 8.0 if ang < 0 else ang) == float(k), "direction k lies on the boundary of bin k, exactly"
    assert counts["negzero_S10_B1"]["negative_zero"] > 0 and counts["negzero_S10_B1"]["zero"] > 0
    tr = F.hist_tracks("negzero_S10_B1")
    v = tr[:, 1:] - tr[:, :-1]
    for axis in (0, 1):                                # -0.0 and +0.0 under each of +1 and -1 in the other coordinate
        z, o = v[..., axis], v[..., 1 - axis]
        assert {(bool(np.signbit(a)), float(b)) for a, b in zip(z[z == 0.0].ravel(), o[z == 0.0].ravel())} == \
            {(False, 1.0), (True, 1.0), (False, -1.0), (True, -1.0)}
    assert counts["ulp_S16_B1"]["to_eight"] > 0 and counts["ulp_S16_B1"]["wrapped"] > 0
    assert len(F.NEIGHBOURS) == 2 * FR.BINS and len(set(F.NEIGHBOURS)) == 16
    for x, y in F.NEIGHBOURS:
        near = [d for d in F.DIRECTIONS if abs(x - d[0]) <= 3e-16 and abs(y - d[1]) <= 3e-16]
        assert len(near) == 1 and (x, y) != tuple(map(float, near[0]))
    zero = counts["zero_S10_B3"]
    assert zero["zero"] == 3 * 17 * FR.POINTS and (F.hist_expected("zero_S10_B3") == 0.0).all()
    tr = F.hist_tracks("tiny_huge_S10_B1")
    mags = np.abs(tr[0, 1] - tr[0, 0]).max(axis=-1)
    assert mags.min() <= 5e-300 and mags.max() >= 1e6 and counts["tiny_huge_S10_B1"]["zero"] > 0
    assert F.hist_expected("tiny_huge_S10_B1").max() > 1e6
    tr = F.hist_tracks("single_cell_S16_B1")
    moving = np.flatnonzero((tr[0, 1:] != tr[0, :-1]).any(axis=(0, 2)))
    assert sorted(moving.tolist()) == sorted(FR.cell_point(F.SINGLE_CELL, a) for a in range(25))
    rows = F.hist_expected("single_cell_S16_B1").reshape(-1, 16, 8)
    assert (rows[:, F.SINGLE_CELL] != 0).any() and (np.delete(rows, F.SINGLE_CELL, axis=1) == 0.0).all()
    assert F.SINGLE_CELL // FR.CELLS != F.SINGLE_CELL % FR.CELLS
    s = F.HIST["constant_velocity_S10_B3"][1]
    rows = F.hist_expected("constant_velocity_S10_B3")
    assert (rows[:, :(s - 1) * 128] != 0).any() and (rows[:, (s - 1) * 128:] == 0.0).all()
    for name in F.HIST:                                # exactness of the hand-made tracks: a step is an integer vector, or v / -v
        if name.startswith(("ulp", "tiny_huge")):
            tr = F.hist_tracks(name)
            v = tr[:, 1:] - tr[:, :-1]
            assert (v[:, 1:] == -v[:, :-1]).all()
    total = [sum(c["boundary"][k] for c in counts.values()) for k in range(FR.BINS)]
    assert all(t > 0 for t in total) and sum(c["wrapped"] for c in counts.values()) > 0


def test_the_gram_cases_cover_the_block_edges():
    assert {(n, m) for n, m, _ in F.GRAM} == {(2, 2), (2, 17), (16, 16), (17, 2), (130, 131)}
    assert {d for _, _, d in F.GRAM} == {1, F.TILE - 1, F.TILE, F.TILE + 1, F.THREADS - 1, F.THREADS, F.THREADS + 1}
    assert (130, 131, 257) in F.GRAM and 130 + 131 > F.THREADS
    assert {n for n, _, _ in F.GRAM} | {m for _, m, _ in F.GRAM} >= {2, F.TILE, F.TILE + 1}
    for shape in F.GRAM:
        a, b = F.gram_rows(*shape)
        gram, scalars = FR.gram_parts(a, b)
        assert gram.shape == shape[:2] and (scalars > 0).all()
    kind, h, w, s = F.TRACKER
    assert (h, w, s) == (64, 65, F.MIN_SEQ) and FR.segments(s, s) == 1 and FR.segments(s - 1, s) == 0
    assert FR.margins_clear(F.tracker_expected()["margins"]) and (F.tracker_expected()["rows"] != 0).any()


# ------------------------------------------------------------------------------------------------------- discrimination
@pytest.mark.parametrize("mutant", sorted(V.MUTANTS))
def test_every_vmaf_mutant_moves_its_case_by_a_thousand_bars(mutant):
    case = V.BY_ID[V.MUTANTS[mutant]]
    d = float(np.abs(V.expected(case.id, mutant) - V.expected(case.id)).max())
    print(f"{mutant} on {case.id}: {d:.3e}")
    assert math.isclose(1e-6, 1000 * V.BAR) and d >= 1e-6, f"{mutant} on {case.id}: {d:.3e}"
    assert case.h <= 130 and case.w <= 130
    plan = V.case_plan(case)
    if mutant == "pass2_from_0":
        assert len(plan["passes"]) > 1
    if mutant == "adm_hw_swapped":
        assert any(s[2] != s[3] for s in plan["adm"])
    if mutant == "adm_window_floor":
        assert any(int(s[0] * 0.1) != s[2] or int(s[1] * 0.1) != s[3] for s in plan["adm"])
    if mutant == "vif_tile_row_more":
        assert any(s[0] % V.TH for s in plan["vif"])
    if mutant == "decimate_odd":
        assert case.h % 2 == 1
    if mutant == "motion2_before":
        assert case.n > 1


@pytest.mark.parametrize("mutant", sorted(F.MUTANTS))
def test_every_fvmd_mutant_moves_its_case_by_a_thousand_bars(mutant):
    stage, case = F.MUTANTS[mutant]
    assert case in {"hist": F.HIST, "gram": F.GRAM, "jacobi": F.JACOBI}[stage], "a case the GPU file runs"
    if stage == "jacobi":                             # without the mutant the model is at numpy's values on that case
        got = np.sort(F.jacobi_model(F.jacobi_matrix(*case))[0])[::-1]
        assert np.abs(got[:min(case)] - F.jacobi_expected(*case)).max() <= F.BAR * max(1.0, got[0]) and max(case) <= 130
    d = F.mutant_distance(mutant)
    print(f"{mutant} on {F.MUTANTS[mutant][1]}: {d:.3e}")
    assert d >= 1e-6, f"{mutant} on {F.MUTANTS[mutant]}: {d:.3e}"


def test_cases_that_cannot_see_a_mutant():
    """Why the cases are what they are: a square plane is blind to swapped h and w in the ADM window, a clip of one pass to
    a second pass that reads from frame 0, a single frame to the order of motion2's minimum, vectors on the bin boundaries
    to a misplaced second share, a set against itself to a wrong mean.  Each mutant here is the statement itself."""
    ref, dis = VR.fixture(64, 64)
    want = VR.expected(64, 64)
    assert np.array_equal(VR.features(ref, dis, mutant="adm_hw_swapped"), want), "square: h and w may be swapped unseen"
    assert np.array_equal(VR.features(ref, dis, mutant="pass2_from_0"), want), "three frames: there is no second pass"
    assert np.array_equal(VR.features(ref[:1], dis[:1], mutant="motion2_before"), want[:1] * [1, 0, 1, 1, 1, 1]), "one frame: no motion"
    axes = F.hist_tracks("axes_S10_B1")
    assert np.array_equal(FR.features(axes, mutant="vote_previous_bin"), F.hist_expected("axes_S10_B1")), \
        "vectors exactly on the boundaries have no second share to misplace"
    a, b = F.gram_rows(2, 17, 15)
    g0, s0 = FR.gram_parts(a, a)
    g1, s1 = FR.gram_parts(a, a, mutant="centre_by_a")
    assert np.array_equal(g0, g1) and np.array_equal(s0, s1), "a set against itself: both means are A's"


# ------------------------------------------------------------------------------------------------------- cost
def test_the_statement_values_of_the_new_cases_are_cheap():
    V.inputs.cache_clear(), V.expected.cache_clear(), V.counts.cache_clear()
    F.hist_expected.cache_clear(), F.tracker_expected.cache_clear(), F.jacobi_expected.cache_clear()
    t = time.perf_counter()
    for c in V.CASES:
        V.expected(c.id)
    from elvis_amd import vmaf
    for nsv in V.PREDICT_NSV:
        for flags in V.PREDICT_FLAGS:
            m = vmaf.VmafModel(**V.predict_model_fields(nsv, flags))
            for n in V.PREDICT_N:
                VR.score(V.predict_features(n), m)
    for shape, rects in V.LUMA:
        frames, masks = V.luma_inputs(shape)
        for rect in rects:
            for order in ("rgb", "bgr"):
                VR.luma(frames, order, rect=rect), VR.luma(frames, order, masks, False, rect), VR.luma(frames, order, masks, True, rect)
    t_vmaf = time.perf_counter() - t
    t = time.perf_counter()
    for name in F.HIST:
        F.hist_expected(name)
    for shape in F.JACOBI:
        F.jacobi_expected(*shape)
    for shape in F.GRAM:
        FR.gram_parts(*F.gram_rows(*shape))
    for shape in F.FRECHET:
        a, b = F.frechet_rows(*shape)
        FR.frechet(a, b), FR.fd_scale(a, b)
    F.tracker_expected()
    t_fvmd = time.perf_counter() - t
    print(f"statement values: vmaf {t_vmaf:.2f} s for {len(V.CASES)} cases, fvmd {t_fvmd:.2f} s")
    assert t_vmaf + t_fvmd < 60.0
