"""tests/_vq_grid_ref.py on the CPU: the source text it restates, the model against the brute-force first minimum
(`_normref.vq_ref`) on every case the GPU test runs, what the cases contain, and the mutants."""
import os

import numpy as np
import pytest

import _normref as R
import _vq_grid_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_runs = {}


def _run(case_id, mutant=None):
    """(reference index, model index, shells, late) of a case, computed once."""
    key = (case_id, mutant)
    if key not in _runs:
        cb, z = V.BY_ID[case_id].arrays()
        _runs[key] = V.search(cb, z, mutant)
    return _runs[key]


def _ref(case_id):
    if ("ref", case_id) not in _runs:
        cb, z = V.BY_ID[case_id].arrays()
        _runs[("ref", case_id)] = R.vq_ref(z, cb)[0].astype(np.int64)
    return _runs[("ref", case_id)]


def test_the_model_restates_the_sources_own_expressions():
    src = open(os.path.join(ROOT, "elvis_amd", "csrc", "vq_index.hip")).read()
    for text in V.SOURCE_TEXT:
        assert text in src, text
    assert [V.grid_cells(k) for k in (1, 2, 5, 6, 7, 257, 8192, 8193, 16384, 20000)] == [1, 1, 1, 1, 2, 5, 16, 16, 16, 16]
    assert V.grid_cells(7447) == 15 and V.grid_cells(7448) == 16          # 16 cells from 2 * 15.5^3 = 7447.75 codes on


def test_the_cases_stay_small_and_hold_what_their_names_say():
    assert {"mirrored_winner_seen_later", "random_2000", "far_outside"} == {c for c, _ in V.MUTANT_CASES.values()}
    for case in V.CASES:
        cb, z = case.arrays()
        assert cb.shape[1] == z.shape[1] == 3 and cb.shape[0] <= V.MAX_CODES and z.shape[0] <= V.MAX_PIXELS, case.id
        assert cb.shape[0] <= 8192 or z.shape[0] <= 1100
    cells = {c.id: V.grid_cells(c.arrays()[0].shape[0]) for c in V.CASES}
    assert cells["k6_one_cell"] == 1 and cells["k7_two_cells"] == 2 and cells["k16384_grid_capped"] == cells["k20000_grid_capped"] == 16
    assert [V.BY_ID[f"p{p}"].arrays()[1].shape[0] for p in (255, 256, 257)] == [255, 256, 257]
    for name, axes in (("constant_z", (2,)), ("constant_yz", (1, 2)), ("all_identical", (0, 1, 2))):
        cb, z = V.BY_ID[name].arrays()
        ix = V.build(cb)
        for a in range(3):
            flat = a in axes
            assert (np.ptp(cb[:, a]) == 0) == flat
            if flat:
                v = cb[0, a]
                assert (ix.edges[a] == v).all()                                # every edge of the axis is the value
                assert (z[:, a] < v).any() and (z[:, a] == v).any() and (z[:, a] > v).any()
                # every code sits in cell G - 1; a pixel below the value sits in cell 0
                assert V.axis_cell(ix.edges[a], ix.G, v) == ix.G - 1 and V.axis_cell(ix.edges[a], ix.G, v - 1) == 0


@pytest.mark.parametrize("case_id", [c.id for c in V.CASES])
def test_the_model_is_the_first_minimum_of_the_scan(case_id):
    idx, shells, late = _run(case_id)
    ref = _ref(case_id)
    bad = np.flatnonzero(idx != ref)
    assert bad.size == 0, f"pixel {bad[0]}: the model gives {idx[bad[0]]}, the scan {ref[bad[0]]}"
    assert (shells >= 1).all() and (shells <= V.grid_cells(V.BY_ID[case_id].arrays()[0].shape[0])).all()


def test_the_cases_together_walk_every_kind_of_search():
    shells = {c.id: _run(c.id)[1] for c in V.CASES}
    late = {c.id: _run(c.id)[2] for c in V.CASES}
    # a stop at r = 0 in a grid that has more shells to offer, and in the grid of one cell
    assert (shells["random_2000"] == 1).any() and V.grid_cells(2000) == 10 and (shells["k6_one_cell"] == 1).all()
    assert (shells["random_2000"] >= 3).any() and (shells["cluster_and_corners"] >= 3).any()              # a stop at r >= 2
    for name in ("constant_z", "constant_yz", "all_identical"):                                          # all G shells
        cb, z = V.BY_ID[name].arrays()
        assert (shells[name] == V.grid_cells(cb.shape[0])).any(), name
    assert (shells["all_identical"] == V.grid_cells(300)).all()
    # an empty own cell: the first shell gives nothing
    cb, z = V.BY_ID["cluster_and_corners"].arrays()
    ix = V.build(cb)
    empty = 0
    for p in z[:150]:
        c = [V.axis_cell(ix.edges[d], ix.G, p[d]) for d in range(3)]
        cell = (c[0] * ix.G + c[1]) * ix.G + c[2]
        empty += int(ix.start[cell] == ix.start[cell + 1])
    assert empty > 50
    # a tie won by a code that was visited after its rival, and only the mirrored case is built for it
    assert late["mirrored_winner_seen_later"].sum() >= 10
    idx = _run("mirrored_winner_seen_later")[0]
    assert (idx[late["mirrored_winner_seen_later"]] % 2 == 0).all()


@pytest.mark.parametrize("mutant", V.MUTANTS)
def test_every_mutant_is_seen_on_its_case(mutant):
    case_id, what = V.MUTANT_CASES[mutant]
    idx, shells, late = _run(case_id)
    midx, mshells, _ = _run(case_id, mutant)
    ref = _ref(case_id)
    if what == "idx":
        changed = np.flatnonzero(midx != ref)
        print(f"{mutant}: {changed.size} of {ref.size} pixels of {case_id} get another code")
        assert changed.size > 0, f"{mutant} is not seen on {case_id}"
        if mutant == "tie_keeps_first_seen":
            assert set(changed.tolist()) == set(np.flatnonzero(late).tolist())      # exactly the pixels whose winner came later
    else:
        assert np.array_equal(midx, ref), f"{mutant} was meant to change the cost alone"
        print(f"{mutant}: {int((mshells != shells).sum())} of {ref.size} pixels of {case_id} walk another number of shells")
        assert (mshells >= shells).all() and (mshells > shells).any()
