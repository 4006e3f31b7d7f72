"""tests/_gn_fused_model.py on the CPU: the source text it restates, the kernel paths its GPU cases reach, its mutants, the
clamp case, and the sizes of the cases."""
import os

import numpy as np
import pytest

import _gn_fused_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def test_the_model_restates_the_sources_own_expressions():
    src = open(os.path.join(ROOT, "elvis_amd", "csrc", "gn_fused.hip")).read()
    for text in M.SOURCE_TEXT:
        assert text in src, text
    # the three orders the model follows, as the source's header states them
    for text in ("lane v adds the tiles t = v, v + 256, ... in ascending order, in fp64,", "lane[v] += lane[v + o], o = 128 ... 1",
                 "the group's sum over its cpg channels in ascending channel order, from 0"):
        assert text in src, text


def test_the_spans_of_the_issues_table():
    for (c, groups), span in M.SHAPES.items():
        assert M.span_of(c, groups) == span, (c, groups)
        assert M.row_lanes(c, groups) == (8 if span == 16 else 4)
    assert {s: M.span_of(s, 32) for s in (32, 128, 160)} == {32: 16, 128: 16, 160: 20}       # the cases the GPU test had
    assert M.span_of(2112, 32) == 0 and M.span_of(7, 2) == 0
    # channels of the last workgroup, where it is short
    assert {k: k[0] % M.span_of(*k) for k in ((96, 32), (48, 16), (24, 8), (8, 8))} == {(96, 32): 6, (48, 16): 12, (24, 8): 6, (8, 8): 8}
    assert 2 * M.span_of(96, 32) == 36 and 2 * M.span_of(1024, 32) == 64 and 2 * M.span_of(34, 2) == 34 and 2 * M.span_of(90, 6) == 60


def test_paths_of_single_cases():
    assert M.paths(128, 32, 1000) == {"double_sweep", "single_sweep", "ragged_tail"}         # what the old matrix reached at most
    assert M.paths(160, 32, 1000) == {"idle_threads", "single_sweep", "ragged_tail"}
    assert M.paths(64, 32, 512) == {"double_sweep", "no_tail"}
    assert M.paths(64, 32, 768) == {"double_sweep", "single_sweep", "no_tail"}
    assert M.paths(64, 32, 256) == {"single_sweep", "no_tail"}
    assert M.paths(96, 32, 512) == {"short_last_workgroup", "idle_threads", "single_sweep", "no_tail"}      # RL = 4: no double sweep
    assert M.paths(1024, 32, 1) == {"F64_full_row", "ragged_tail"}
    assert M.paths(8, 8, 257) == {"short_last_workgroup", "single_sweep", "ragged_tail"}


def test_the_gpu_cases_reach_every_path_on_both_instantiations_and_stay_small():
    cases = M.gpu_cases()
    assert len(set(cases)) == len(cases) and {c[:2] for c in cases} == set(M.SHAPES)
    assert M.N_IMAGES <= 2 and max(t for _, _, t in cases) <= 769 and max(t for _, _, t in M.CLAMP_CASES) <= 769
    reached = {8: set(), 4: set()}
    for c, groups, tiles in cases:
        reached[M.row_lanes(c, groups)] |= M.paths(c, groups, tiles)
    assert reached[8] == set(M.PATHS) - {"idle_threads", "F64_full_row"}                       # F = 32 fills the workgroup exactly
    assert reached[4] == set(M.PATHS) - {"double_sweep"}                                       # 64 registers: one sweep at a time
    # every tile count on either instantiation; a sweep that ends exactly, alone, on both
    for rl in (8, 4):
        assert {t for c, g, t in cases if M.row_lanes(c, g) == rl} == set(M.TILES)
    assert any(M.paths(c, g, t) >= {"double_sweep", "no_tail"} and "single_sweep" not in M.paths(c, g, t) for c, g, t in cases)
    assert any(M.paths(c, g, t) >= {"short_last_workgroup", "ragged_tail", "idle_threads"} for c, g, t in cases)
    # more than one size on the RL = 8 path and on the RL = 4 path
    assert len({M.span_of(c, g) for c, g, _ in cases if M.row_lanes(c, g) == 4}) >= 5
    assert all(case in cases for case in M.MUTANT_CASES.values())


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_changes_a_bit_on_its_case(mutant):
    c, groups, tiles = M.MUTANT_CASES[mutant]
    p = M.partials(M.N_IMAGES, tiles, c, c // groups)
    args = M.params(c, True) + (tiles * 256, groups, M.EPS)
    info = {}
    pa, pb = M.model(p, *args, info=info)
    assert (info["var"] > 0).any() and np.isfinite(pa).all() and np.isfinite(pb).all()
    qa, qb = M.model(p, *args, mutant=mutant)
    changed = int((_bits(pa) != _bits(qa)).sum() + (_bits(pb) != _bits(qb)).sum())
    print(f"{mutant}: {changed} of {2 * pa.size} words differ")
    assert changed > pa.size // 2, f"{mutant} is not seen on {(c, groups, tiles)}"


def test_inputs_a_few_binades_apart_cannot_tell_one_order_from_another():
    """Why `partials` plants its cancelling pairs: fp32 sums around 20 +- 50 add exactly in float64, whatever the order - the
    inputs of the first GPU matrix, which therefore never depended on the order of the sums."""
    rng = np.random.default_rng(0)
    s = (rng.standard_normal((2, 769, 64)) * 50 + 20).astype(np.float32)
    ss = (s.astype(np.float64) ** 2 / 256 + np.abs(rng.standard_normal(s.shape)) * 100 + 50).astype(np.float32)
    p = np.stack([s, ss], -1)
    args = M.params(64, True) + (769 * 256, 32, M.EPS)
    pa, pb = M.model(p, *args)
    for mutant in M.MUTANTS:
        qa, qb = M.model(p, *args, mutant=mutant)
        assert np.array_equal(_bits(pa), _bits(qa)) and np.array_equal(_bits(pb), _bits(qb)), mutant


@pytest.mark.parametrize("c,groups,tiles", M.CLAMP_CASES)
def test_the_clamp_case_has_a_variance_below_zero(c, groups, tiles):
    v = M.clamp_values(groups)
    assert all(float(np.float32(x * x)) < float(x) * float(x) for x in v) and len(set(v.tolist())) == groups
    p = M.clamp_partials(M.N_IMAGES, tiles, c, groups)
    info = {}
    gam, bet, sc, sh = M.params(c, True)
    pa, pb = M.model(p, gam, bet, sc, sh, tiles * 256, groups, M.EPS, info=info)
    want = np.float32(v * v).astype(np.float64) - v.astype(np.float64) ** 2
    assert (info["var"] < 0).all() and np.array_equal(info["var"], np.broadcast_to(want, info["var"].shape))
    # with the variance clamped to 0, rstd is 1 / sqrt(eps) for every group
    rstd = np.float32(1.0 / np.sqrt(np.float64(np.float32(M.EPS))))
    assert np.array_equal(pa, np.broadcast_to((rstd * gam) * (np.float32(1) + sc), pa.shape))
    # and without the clamp the result would be another (or none): sqrt of eps + var, var about -1e-7 v^2 against eps = 1e-6
    assert (np.abs(info["var"]) > 1e-9).all()
