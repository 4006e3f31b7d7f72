"""CPU-side checks of the block matrix (tests/_blockref.py, tests/test_gpu_block_matrix.py): the ledger (the kernels of
csrc/classical.hip, csrc/degrade.hip and csrc/shrink.hip in the built library are exactly the ten the cases name), the
branches the case list must reach, the pins of the hooked restatements against the existing references and of the
shrink cases against the goldens, and the discrimination test: every mutant of a reference differs from the true one
on a small case - otherwise the inputs could not tell a wrong kernel from a right one."""
import functools
import os

import numpy as np
import pytest

import _blockref as R
import _classical_ref as C
import _shrink_ref as S
from oracle import degrade_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elvis_amd", "csrc")
SMALL = [c for c in R.CASES if not c.big]


def _of(op, cases=R.CASES):
    return [c for c in cases if c.op == op]


@functools.lru_cache(maxsize=None)
def _true(cid):
    return R.expected(R.BY_ID[cid])


# ------------------------------------------------------------------------------------------------------- ledger
def test_demangle_kernels_of_an_unnamed_namespace():
    stems = R.kernel_stems(os.path.join(CSRC, "shrink.hip"))
    assert stems == {"block_gather_u8_kernel", "shrink_select_topk_kernel", "shrink_select_passes_kernel", "stretch_index_kernel"}
    from _glueref import demangle_kernel
    assert demangle_kernel("_ZN12_GLOBAL__N_120stretch_index_kernelEPKhPiiiiii", stems) == "stretch_index_kernel"
    assert demangle_kernel("_ZN12_GLOBAL__N_135__device_stub__stretch_index_kernelEPKhPiiiiii", stems) is None
    assert demangle_kernel("elvis_stretch_index", stems) is None


def test_kernel_ledger(built_lib):
    """The kernels of the three source files in the built library == the names the cases resolve to: ten."""
    syms = set()
    for src in R.SOURCES:
        syms |= R.kernel_symbols(built_lib, os.path.join(CSRC, src))
    named = {c.kernel for c in R.CASES}
    assert not syms - named, f"kernels without a matrix case: {sorted(syms - named)}"
    assert not named - syms, f"cases naming kernels the library does not build: {sorted(named - syms)}"
    assert len(syms) == 10 and set(R.OPS) == {c.op for c in R.CASES}
    assert len({c.id for c in R.CASES}) == len(R.CASES)
    assert {c.launch for c in _of("gather")} == {f"block_gather_u8_kernel<{v}>" for v in (16, 8, 4, 1)}
    text = open(os.path.join(CSRC, "shrink.hip")).read()
    for c in _of("gather"):
        assert f'"{c.launch}"' in text


# ------------------------------------------------------------------------------------------------------- coverage
def test_the_shrink_cases_cover_the_branches():
    topk = _of("topk")
    assert {c.grid[2] for c in topk} == set(R.TOPK_BX) and {c.grid[1] for c in topk} == {1, 3} and {c.grid[0] for c in topk} == {1, 2}
    for bx in R.TOPK_BX:
        assert {c.k for c in topk if c.grid[2] == bx} == {0, 1, bx - 1, bx}
        assert {c.kind for c in topk if c.grid[2] == bx} == set(R.TOPK_KINDS)
        assert {c.kind for c in topk if c.grid[2] == bx and c.k == bx} == set(R.TOPK_KINDS)       # NULL src_of
    assert any(c.grid[2] > 256 for c in topk), "the second trip of the lane loops"
    for c in topk:
        s, = R.inputs(c)
        assert not np.isnan(s).any()
        if c.kind == "zeros" and s.size > 3:
            assert np.signbit(s).any() and not np.signbit(s).all() and not s.any()
        if c.kind == "inf" and s.size > 100:
            assert np.isposinf(s).any() and np.isneginf(s).any()

    ps = _of("passes")
    lengths = {0: set(), 1: set()}
    for c in ps:
        for axis, length, _ in R.passes_trace(c):
            lengths[axis].add(length)
    assert lengths[0] >= set(R.LINE_LENGTHS) and lengths[1] >= set(R.LINE_LENGTHS), "working line lengths, rows and columns"
    assert {c.grid[1] for c in ps} >= {15, 16, 17, 33}
    for (by, bx) in ((17, 5), (33, 3)):
        for mode in ("rows", "rows_cols"):
            assert {c.target for c in ps if c.grid == (1, by, bx) and c.mode == mode} >= \
                {0, 1, by, by + 1, by + bx - 1, by * bx - 1, by * bx}
    assert any(c.mode == "rows" and c.grid[2] == 1 and c.target > 0 for c in ps), "rows-only with one column"
    for mode in ("rows", "rows_cols"):
        assert {c.ridx for c in ps if c.mode == mode} == {True, False}
    assert any(c.grid[0] == 3 for c in ps if c.mode == "rows") and any(c.grid[0] == 3 for c in ps if c.mode == "rows_cols")
    for c in ps:
        if c.grid[0] == 3:
            s, = R.inputs(c)
            assert not np.array_equal(s[0], s[1]) and not np.array_equal(s[1], s[2])
    assert any(len(R.passes_counts(c)) and R.passes_counts(c)[-1] < (c.grid[1] if len(R.passes_counts(c)) % 2 or c.mode == "rows"
                                                                     else c.grid[2]) for c in ps), "a partial last pass"
    # where the minimum sits: the indices removed from lines longer than a wave, rows and columns
    seen = {0: set(), 1: set()}
    for c in ps:
        if not c.kind.startswith("place"):
            continue
        passes = _true(c.id)[2][0]
        at = 0
        for axis, length, cnt in R.passes_trace(c):
            if length > 64:
                seen[axis] |= {("last" if i == length - 1 else int(i)) for i in passes[at:at + cnt] if i in (0, 63, 64, length - 1)}
            at += cnt
    assert seen[0] == {0, 63, 64, "last"} and seen[1] == {0, 63, 64, "last"}
    for axis, suffix in ((0, ""), (1, "_cols")):
        assert {c.kind for c in ps} >= {"tie64" + suffix, "tie1" + suffix}

    st = _of("stretch")
    for mode in ("flat", "rows"):
        seg = lambda c: c.grid[1] * c.grid[2] if mode == "flat" else c.grid[2]
        assert {seg(c) for c in st if c.mode == mode} == set(R.STRETCH_LENGTHS)
        assert {c.kind for c in st if c.mode == mode} == set(R.STRETCH_KINDS)
    assert any(c.mode == "rows" and c.sgrid[0] < c.grid[1] for c in st), "rows with limit == 0"
    for c in st:
        m, = R.inputs(c)
        kept = int((m == 0).sum())
        if c.kind == "bytes" and m.size > 50:
            assert set(np.unique(m).tolist()) == {0, 1, 2, 255}
        if c.kind == "all_kept":
            assert kept == m.size
        if c.kind == "all_removed":
            assert kept == 0
        if c.kind == "surplus" and m.size > 50:
            assert kept > c.grid[0] * c.sgrid[0] * c.sgrid[1], "more kept than the shrunk grid holds"

    ga = _of("gather")
    assert {(c.shape[1], c.shape[2], c.block, c.shape[3]) for c in ga} >= set(R.GATHER_WIDTHS)
    assert {c.offs for c in ga} >= set(R.GATHER_OFFSETS)
    for c in ga:
        assert c.launch == R.gather_launch(c.block * c.shape[3], c.shape[2] * c.shape[3], c.offs[0], c.offs[1]), c.id
    base = [c for c in ga if c.offs != (0, 0, 0)]
    assert {c.launch[-4:] for c in base} == {"<16>", "l<8>", "l<4>", "l<1>"}
    for off, name in ((1, "<1>"), (4, "<4>"), (8, "<8>")):      # the narrower name from a misaligned source, and destination
        assert any(c.offs == (off, 0, 0) and c.launch.endswith(name) for c in ga)
        assert any(c.offs == (0, off, 0) and c.launch.endswith(name) for c in ga)
        assert any(c.offs == (0, 0, off) and c.launch.endswith("<16>") for c in ga)
    assert any(c.sgrid == (0, 0) and c.shape[1] == 0 for c in ga), "no source: all holes"
    items = lambda c, v: c.shape[0] * c.dgrid[0] * c.block * c.dgrid[1] * c.block * c.shape[3] // v
    assert any(c.launch.endswith("<1>") and items(c, 1) > R.GATHER_CAP_ITEMS for c in ga)
    assert any(c.launch.endswith("<16>") and items(c, 16) > R.GATHER_CAP_ITEMS for c in ga)
    assert {c.id for c in ga if c.big} == {c.id for c in ga if items(c, int(c.launch[:-1].split("<")[1])) > R.GATHER_CAP_ITEMS}
    for c in _of("gather", SMALL):
        src_of = R.inputs(c)[1]
        n_src = c.sgrid[0] * c.sgrid[1]
        assert (src_of < 0).any() and (src_of >= n_src).any()


def test_the_classical_cases_cover_the_branches():
    la = _of("lanczos")
    for ch in R.CLASSICAL_C:
        for b in R.CLASSICAL_B:
            hit = [c for c in la if c.shape[3] == ch and c.block == b and c.kind == "noise"]
            assert hit, (ch, b)
            lb = int(np.log2(b))
            want = {-1, 16, 17} | set(range(0, lb + 2))
            for c in hit:
                m = R.inputs(c)[1]
                assert set(np.unique(m[0]).tolist()) == want and c.grid[1] != c.grid[2] and c.grid[0] == 2
                assert not np.array_equal(m[0], m[1])
    for f in (4, 8, 16, 32):
        hit = [c for c in la if c.kind == f"ties{f}"]
        assert hit and all(c.levels == (int(np.log2(f)),) for c in hit)
        for c in hit:
            x = R.inputs(c)[0]
            s = x.reshape(1, x.shape[1] // f, f, x.shape[2] // f, f, -1).astype(np.int64).sum((2, 4))
            q, r = np.divmod(s, f * f)
            ties = q[2 * r == f * f]
            assert (ties % 2 == 0).any() and (ties % 2 == 1).any(), f"{c.id}: ties with even and with odd quotients"
    for kind in ("small_step", "small_checker"):
        hit = [c for c in la if c.kind == kind]
        assert hit
        for c in hit:
            x, m = R.inputs(c)
            assert set(np.unique(x).tolist()) == {0, 255}
            ref, = _true(c.id)
            assert (ref == 0).any() and (ref == 255).any()

    un = _of("unsharp")
    noise = [c for c in un if c.kind == "noise" and c.levels == R.UNSHARP_LEVELS]
    assert {(c.shape[3], c.block) for c in noise} == {(ch, b) for ch in R.CLASSICAL_C for b in R.CLASSICAL_B}
    assert {(c.block, c.halo) for c in noise} == {(b, h) for b in R.CLASSICAL_B for h in R.HALOS}
    assert set(R.UNSHARP_LEVELS) >= set(range(1, R.MAX_LEVEL + 2)) and R.MAX_LEVEL == 16
    for c in noise:
        assert set(np.unique(R.inputs(c)[1]).tolist()) == set(R.UNSHARP_LEVELS)
    assert any(c.block == 2 and c.halo == 0 and R.MAX_LEVEL in c.levels for c in un), "reflect101 loops many times"
    ragged = [c for c in un if c.shape[1] % c.block and c.shape[2] % c.block]
    assert {c.halo for c in ragged} >= {0, 3}
    odd = [c for c in un if c.levels and all(lv % 2 == 1 for lv in c.levels)]
    assert {c.kind for c in odd} >= {"checker", "step", "noise"}
    for c in odd:
        if c.kind in ("checker", "step"):
            ref, = _true(c.id)
            assert (ref == 0).any() and (ref == 255).any()
    big = [c for c in un if c.big]
    assert [(c.shape, c.block, c.halo) for c in big] == [((1, 96, 96, 4), 32, 32)]
    assert R.inputs(big[0])[1][0, 1, 1] == R.MAX_LEVEL, "the centre block, with all four halos, at the top level"
    th = 32 + 2 * 32
    assert 2 * th * 32 * 4 + th * th * 4 == 60 * 1024, "the largest dynamic LDS launch"

    bl = _of("blend")
    assert {c.tb for c in bl if c.kind == "pairs" and not c.alias} == set(R.TBS)
    pairs = R.inputs([c for c in bl if c.kind == "pairs"][0])[0]
    assert len({(int(a), int(b)) for a, b in zip(pairs[0].ravel(), pairs[1].ravel())}) == 65536
    for n in (1, 5):
        assert {c.tb for c in bl if c.shape[0] == n} == set(R.TBS)
    for px in (1, 255, 256, 257):
        assert {c.tb for c in bl if int(np.prod(c.shape[1:])) == px} == set(R.TBS)
    assert {c.tb for c in bl if c.alias} >= set(R.TBS)
    assert all(c.big == (c.id.startswith("gather_over_cap") or c.id.startswith("unsharp_largest")) for c in R.CASES)


def test_the_degrade_cases_cover_the_branches():
    for op, blocks, values in (("downsample", R.DOWN_B, R.DOWN_LEVELS), ("gaussian", R.GAUSS_B, R.GAUSS_ROUNDS),
                               ("dct", (8,), R.DCT_MAP)):
        cs = _of(op)
        assert {c.shape[3] for c in cs} >= {1, 3, 4} and {c.shape[0] for c in cs} >= {1, 3}
        assert {c.grid[0] * c.grid[1] * c.grid[2] * c.shape[3] for c in cs} >= {63, 64, 65}, op
        assert {c.block for c in cs} >= set(blocks), op
        for b in blocks:
            reached = set()
            for c in cs:
                if c.block == b:
                    reached |= set(np.unique(R.inputs(c)[1]).tolist())
            assert reached >= set(values), (op, b)
    assert set(R.DOWN_LEVELS) >= {-1, 0, 1, 2, 3, 4, 5, 100} and set(R.GAUSS_ROUNDS) == {-3, 0, 1, 10, 32, 33, 1000}
    assert set(R.DCT_MAP) == {-1, 0, 1, 2, 3, 4, 9} and set(R.GAUSS_B) == {1, 2, 3, 5, 8, 12, 16}
    down = _of("downsample")
    for f in (2, 4, 8, 16):
        hit = [c for c in down if c.kind == f"ties{f}"]
        assert {c.block for c in hit} == {f, 16}
        x = R.inputs(hit[0])[0]
        s = x.reshape(1, x.shape[1] // f, f, x.shape[2] // f, f, -1).astype(np.int64).sum((2, 4))
        q, r = np.divmod(s, f * f)
        assert (q[2 * r == f * f] % 2 == 0).any() and (q[2 * r == f * f] % 2 == 1).any()
    for b in (2, 4):      # s < 1: the level exceeds log2 b
        assert any(c.block == b and max(c.levels) > np.log2(b) for c in down)
    for b in R.GAUSS_B:
        assert {c.kind for c in _of("gaussian") if c.block == b} >= set(R.CONTENTS)
    assert {c.kind for c in _of("dct")} >= set(R.CONTENTS)
    for c in _of("dct"):
        if c.kind in ("flat0", "flat255"):
            assert np.array_equal(_true(c.id)[0], R.inputs(c)[0]), f"{c.id}: a flat block must come back unchanged"


# ------------------------------------------------------------------------------------------------------- pins
@pytest.mark.parametrize("op", R.OPS)
def test_the_hooked_restatements_equal_the_existing_references(op):
    for c in _of(op, SMALL):
        x = R.inputs(c)
        ref = _true(c.id)
        n = (c.grid or c.shape)[0]
        if op == "topk":
            got = [R.topk_ref(x[0][f], c.k) for f in range(n)]
            got = (np.stack([g[0] for g in got]), np.stack([g[1] for g in got]))
        elif op == "passes":
            per = [R.passes_ref(x[0][f], c.target, c.mode == "rows") for f in range(n)]
            got = (np.stack([p[0] for p in per]).astype(np.uint8), np.stack([p[1] for p in per]),
                   np.stack([np.concatenate(p[2]) if p[2] else np.zeros(0, np.int32) for p in per]).astype(np.int32))
            assert [len(p) for p in S.passes_select(x[0][0], c.target, c.mode == "rows")[2]] == R.passes_counts(c), c.id
        elif op == "stretch":
            got = (np.stack([R.stretch_ref(x[0][f], c.sgrid, c.mode) for f in range(n)]),)
        elif op == "gather":
            holes = np.where((x[1] < 0) | (x[1] >= c.sgrid[0] * c.sgrid[1]), -1, x[1])
            assert np.array_equal(ref[1] == 255, np.repeat(np.repeat(holes < 0, c.block, 1), c.block, 2)), c.id
            assert not ref[0][ref[1] == 255].any() and ref[0][ref[1] == 0].all(), c.id
            continue
        elif op == "blend":
            got = (R.blend_ref(x[0], c.tb),)
        elif op == "lanczos":
            got = (R.lanczos_ref(x[0], x[1], c.block),)
        elif op == "unsharp":
            got = (R.unsharp_ref(x[0], x[1], c.block, c.halo),)
        elif op == "downsample":
            got = (R.downsample_ref(x[0], x[1], c.block),)
        elif op == "gaussian":
            got = (R.gaussian_ref(x[0], x[1], c.block),)
            # the wrap only clamps: below 33 rounds the oracle itself is the reference
            low = np.where(x[1] > R.GAUSS_MAX_ROUNDS, 0, x[1])
            keep = np.repeat(np.repeat(x[1] <= R.GAUSS_MAX_ROUNDS, c.block, 1), c.block, 2)
            plain = np.stack([D.degrade_gaussian(x[0][f], low[f], c.block) for f in range(n)])
            assert np.array_equal(plain[keep], ref[0][keep]), c.id
        else:
            continue
        for g, r in zip(got, ref):
            assert g.dtype == r.dtype and g.shape == r.shape and np.array_equal(g, r), c.id


def test_classical_literal_ports_agree_on_divisible_frames():
    """The per-block literal ports of the reference functions (tests/_classical_ref.py) on the cases they apply to:
    three channels or one, frames the block divides, levels inside [0, 16]."""
    done = 0
    for c in _of("unsharp", SMALL):
        x, m = R.inputs(c)
        if c.shape[1] % c.block or c.shape[2] % c.block or c.block > 8:
            continue
        lv = np.clip(m, 0, R.MAX_LEVEL)
        got = C.ref_restore_with_opencv_unsharp(list(x), list(lv), c.block, halo=c.halo)
        assert np.array_equal(np.stack(got), _true(c.id)[0]), c.id
        done += 1
    assert done >= 8


def test_the_shrink_references_still_equal_the_goldens(golden_dir):
    """The matrix's shrink references on the goldens' own inputs (tests/golden/shrink.npz): the same functions the cases
    call reproduce the reference's recorded outputs."""
    with np.load(os.path.join(golden_dir, "shrink.npz"), allow_pickle=False) as z:
        cases = S.golden_cases(z)
    seen = set()
    for i, d in cases:
        scores, b = d["scores"], d["block"]
        by, bx = scores.shape
        if d["family"] == "elvis":
            k = S.topk_count(d["amount"], bx)
            mask, src_of = R.topk_ref(scores, k)
            assert np.array_equal(mask, d["mask"]), i
            out, _ = R.gather_ref(d["frame"][None], src_of[None], b, (by, bx))
            assert np.array_equal(out[0], d["shrunk"]), i
            back = R.stretch_ref(d["mask"], (by, bx - k), "flat")
            assert np.array_equal(R.gather_ref(d["shrunk"][None], back[None], b, (by, bx - k))[0][0], d["stretched"]), i
        else:
            rows_only = d["family"] == "row_only"
            mask, origin, passes, _ = R.passes_ref(scores, int(by * bx * d["amount"]), rows_only)
            assert np.array_equal(mask, d["mask"]), i
            assert np.array_equal(R.gather_ref(d["frame"][None], origin[None], b, (by, bx))[0][0], d["shrunk"]), i
            if rows_only:
                back = R.stretch_ref(d["mask"], origin.shape, "rows")
                assert np.array_equal(R.gather_ref(d["shrunk"][None], back[None], b, origin.shape)[0][0], d["stretched"]), i
            else:
                assert len(passes) == len(d["ridx"]) and all(np.array_equal(p, q) for p, q in zip(passes, d["ridx"])), i
        seen.add(d["family"])
    assert seen == set(S.FAMILIES)


# ------------------------------------------------------------------------------------------------------- discrimination
MUTANTS = {
    "topk": ("tie_higher", "beat_le"),
    "passes": ("argmin_last", "rows_keep_width"),
    "stretch": ("limit_off_by_one", "polarity"),
    "gather": ("hole_fill", "polarity"),
    "lanczos": ("half_up", "fac2_float", "border_reflect", "no_round", "lo"),
    "unsharp": ("tie_odd", "halo_short", "replicate", "reflect", "hi", "lo"),
    "blend": ("round",),
    "downsample": ("half_up", "fac2_float", "lo", "hi"),
    "gaussian": ("replicate", "reflect", "hi", "lo"),
    "dct": ("hi", "lo"),
}


def _differs(op, mutant, pick=lambda c: True):
    hits = []
    for c in _of(op, SMALL):
        if not pick(c):
            continue
        ref, got = _true(c.id), R.expected(c, mutant=mutant)
        if any(not (g.shape == r.shape and np.array_equal(g, r)) for g, r in zip(got, ref)):
            hits.append(c)
    return hits


@pytest.mark.parametrize("op,mutant", [(op, m) for op, ms in MUTANTS.items() for m in ms])
def test_the_inputs_tell_the_mutant_apart(op, mutant):
    hits = _differs(op, mutant)
    assert hits, f"{op}: the mutant `{mutant}` equals the reference on every small case"
    ids = {c.id for c in hits}
    if (op, mutant) == ("topk", "tie_higher"):
        assert not any(c.kind == "random" for c in hits) and {c.kind for c in hits} == {"equal", "ties", "zeros", "inf"}
    if (op, mutant) == ("passes", "argmin_last"):
        assert {c.kind for c in hits} >= {"tie64", "tie1", "tie64_cols", "tie1_cols", "ties"}
        assert not any(c.kind.startswith("place") for c in hits)
    if (op, mutant) == ("passes", "rows_keep_width"):
        assert all(c.mode == "rows" for c in hits)
    if mutant == "half_up":
        assert {c.kind for c in hits} >= {f"ties{f}" for f in ((4, 8, 16, 32) if op == "lanczos" else (4, 8, 16))}
        assert not any(c.kind == "ties2" for c in hits)
    if mutant == "fac2_float":
        assert any(c.kind == "ties2" for c in hits)
    if (op, mutant) == ("unsharp", "tie_odd"):
        assert any(all(lv % 2 for lv in c.levels) for c in hits)
    if (op, mutant) == ("unsharp", "halo_short"):
        assert all(c.halo > 0 for c in hits) and {c.halo for c in hits} >= {1, 3, 32}
    if (op, mutant) == ("blend", "round"):
        assert {c.tb for c in hits} == {0.3, 0.5, 0.7}
    if (op, mutant) == ("gather", "polarity"):
        assert len(ids) == len(_of("gather", SMALL))


def test_the_lanczos_upper_clamp_changes_no_output():
    """include/elvis_amd.h: every level above log2(block) gives s = 1, so no mutant of the clamp at 16 can exist - the
    blocks of level 16 and 17 equal the blocks of level log2(block) + 1."""
    for c in _of("lanczos", SMALL):
        if c.kind != "noise":
            continue
        x, m = R.inputs(c)
        lb = int(np.log2(c.block))
        assert np.array_equal(_true(c.id)[0], C.lanczos_restore(x, np.where(m > lb, lb, m), c.block)), c.id
