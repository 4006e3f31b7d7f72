"""CPU-side checks of the Real-ESRGAN matrix (tests/_srcases.py and tests/test_gpu_sr_matrix.py): the ledger (the kernels of
csrc/rrdb.hip and csrc/srvgg.hip in the built library are exactly the five the cases name), the branches the case list
must reach - computed from the cases' numbers and the tile constants as csrc/sr_conv3x3.h states them -, the conditions
the value-edge and tie cases claim, the discrimination test (every mutant of the two statements moves its named case
past the bound, the structural ones by at least ten bounds), the cases that cannot see a mutant, the host packer's
rounding against numpy's over every f16 value and midpoint, and the cost of the statement values."""
import ctypes as C
import importlib.util
import os
import re
import time

import numpy as np
import pytest
import torch

import _rrdb_ref as RR
import _srcases as S
import _srmut as M
import _srvgg_ref as SR
from _qualitycases import kernel_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elvis_amd", "csrc")
KERNELS = {"rrdb_conv3x3_kernel<32>", "rrdb_conv3x3_kernel<64>", "rrdb_input_u8_kernel", "srvgg_conv3x3_kernel<64,false>",
           "srvgg_conv3x3_kernel<48,true>"}


# ------------------------------------------------------------------------------------------------------- ledger
def test_kernel_ledger(built_lib):
    """Both directions: no kernel of the two sources without a case, no case naming a kernel the library lacks."""
    built = set()
    for src in S.SOURCES:
        built |= kernel_names(built_lib, os.path.join(CSRC, src))
    assert built == KERNELS, sorted(built)
    groups = S.group_kernels()
    assert set(groups) == {"shapes", "exact", "values", "ties", "input"} and all(groups.values())
    named = {k for ks in groups.values() for k in ks}
    assert not built - named, f"kernels without a matrix case: {sorted(built - named)}"
    assert not named - built, f"cases naming kernels the library does not build: {sorted(named - built)}"
    conv = KERNELS - {"rrdb_input_u8_kernel"}
    assert set(groups["shapes"]) == conv == set(groups["exact"]) == set(groups["values"]), "every template in each of the three groups"
    assert set(groups["ties"]) == {"rrdb_conv3x3_kernel<32>", "srvgg_conv3x3_kernel<48,true>"} and groups["input"] == ("rrdb_input_u8_kernel",)
    # every name a GPU test compares elvis_last_launch with is one the source notes
    text = "".join(open(os.path.join(CSRC, src)).read() for src in S.SOURCES)
    noted = {c.noted for c in S.CASES}
    assert noted == {"rrdb_conv3x3_kernel<32>", "rrdb_conv3x3_kernel<64>", "rrdb_input_u8_kernel<1>", "rrdb_input_u8_kernel<unshuffle2>",
                     "srvgg_conv3x3_kernel<64,prelu>", "srvgg_conv3x3_kernel<48,shuffle_f16>", "srvgg_conv3x3_kernel<48,shuffle_u8>"}
    for name in noted:
        assert re.search(r"elvis_note_launch\([^;]*\"" + re.escape(name) + "\"", text), name
    assert set(re.findall(r"elvis_note_launch\([^;]*?\"([^\"]+)\"", text)) | {"rrdb_input_u8_kernel<1>", "srvgg_conv3x3_kernel<48,shuffle_f16>"} == noted


def test_the_constants_are_the_headers():
    text = open(M.HEADER).read()
    assert "constexpr int SR_TY = 8, SR_TX = 32, SR_KC = 32;" in text and (S.SR_TY, S.SR_TX, S.SR_KC) == M.constants() == (8, 32, 32)
    assert "(t & 1) * 16 + l15" in text and "blockIdx.x * SR_TX" in text and "blockIdx.y * SR_TY" in text
    assert "__float2int_rn" in open(os.path.join(CSRC, "rrdb.hip")).read() and "__float2int_rn" in open(os.path.join(CSRC, "srvgg.hip")).read()


# ------------------------------------------------------------------------------------------------------- pins
def test_without_a_mutant_the_statements_are_what_they_were(golden_dir):
    """`mutant=` is an addition: the statements give the bytes recorded in tests/golden/sr_statement.npz, written by
    tools/make_sr_statement_golden.py from the statements as they were before they took it; an unknown name is refused."""
    spec = importlib.util.spec_from_file_location("make_sr_statement_golden", os.path.join(ROOT, "tools", "make_sr_statement_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    got, want = tool.arrays(), np.load(os.path.join(golden_dir, "sr_statement.npz"))
    assert set(got) == set(want.files) and len(got) == 12
    for key, v in got.items():
        assert v.shape == want[key].shape and v.dtype == want[key].dtype, key
        assert v.tobytes() == want[key].tobytes(), f"{key}: not the recorded bytes"
    x, w, b = tool._x(1, 32, 9, 33, 0), tool._w(32, 32, 0), tool._b(32, 0)
    a = RR.conv_ref(x, w, b)
    assert torch.equal(RR.conv_ref(x, w, b, mutant=None).ref, a.ref) and torch.equal(RR.u8_ref(a, mutant=None)[0], RR.u8_ref(a)[0])
    calls = (lambda m: RR.conv_ref(x, w, b, mutant=m), lambda m: RR.u8_ref(a, mutant=m),
             lambda m: SR.conv_ref(tool._x(1, 64, 9, 33, 0), tool._w(64, 64, 0), tool._b(64, 0), tool._b(64, 1), mutant=m),
             lambda m: SR.tail_ref(tool._x(1, 64, 9, 33, 0), tool._w(48, 64, 0), tool._b(48, 0), tool._x(1, 3, 9, 33, 1), mutant=m),
             lambda m: SR.u8_ref(a, mutant=m))
    for call in calls:
        with pytest.raises(ValueError, match="unknown mutant"):
            call("no_such")
    for call, other in ((calls[0], "slope_roll_1"), (calls[2], "s0_s1_swapped"), (calls[3], "slope_roll_1"), (calls[1], "store_f16_trunc")):
        with pytest.raises(ValueError, match="unknown mutant"):
            call(other)                               # a mutant of another statement is unknown to this one


# ------------------------------------------------------------------------------------------------------- coverage
def test_the_shape_cases_cover_the_tile_edges():
    shapes = S.of("shapes")
    assert {(c.h, c.w) for c in shapes} == set(S.EDGE_SIZES) | set(S.SEAM_FREE_SIZES)
    assert S.EDGE_SIZES == ((1, 65), (33, 1), (3, 15), (10, 16), (11, 17), (5, 47), (8, 48), (16, 49))
    for op, couts in (("rrdb", {32, 64}), ("layer", {64}), ("tail", {48}), ("tail_u8", {48}), ("rrdb_u8", {32})):
        for size in S.EDGE_SIZES:
            here = [c for c in shapes if c.op == op and (c.h, c.w) == size]
            assert {c.cout for c in here} == couts, (op, size)
            if op == "rrdb":
                assert sum(c.ups for c in here) == 1 and {c.cout for c in here if not c.ups} == {32, 64}, size
            if op == "layer":
                assert {(c.cin, c.cin_real) for c in here} == {(32, 3), (64, 0)}, size
    assert {c.w % S.SR_TX for c in shapes} == {1, 15, 16, 17, S.SR_TX - 1, 0}
    assert {c.h % S.SR_TY for c in shapes} >= {1, 2, 3, 5, 0}
    assert {c.w % S.SR_TX for c in shapes if (c.h, c.w) in S.EDGE_SIZES} == {1, 15, 16, 17} and S.SR_TX // 2 == 16
    tiles = {(c.h, c.w): c.tiles for c in shapes if not c.ups}
    assert any(ty > 2 and tx == 1 for ty, tx in tiles.values()) and any(ty == 1 and tx > 2 for ty, tx in tiles.values())
    assert any(c.h > S.SR_TY and c.w < S.SR_TX // 2 for c in shapes), "narrower than a fragment and taller than a tile"
    assert any(c.h == 1 and c.w > 2 * S.SR_TX for c in shapes), "one row, wider than two tiles"
    rrdb = [c for c in shapes if c.op == "rrdb"]
    assert {c.nkc for c in rrdb} == {1, 2, 3, 4, 5, 6} == {c.nkc for c in rrdb if not c.ups} and {c.cin for c in rrdb} == set(S.CINS)
    assert {c.nkc for c in shapes if c.op == "layer"} == {1, 2} and {c.nkc for c in shapes if c.op in ("tail", "tail_u8")} == {2}
    assert {(c.lrelu, "1" in c.res, "2" in c.res) for c in rrdb} == {(l, a, b) for l in (0, 1) for a in (False, True) for b in (False, True)}
    assert any(c.ups and c.tiles[0] * c.tiles[1] > 1 for c in rrdb) and any(c.alias for c in rrdb) and any(S.inputs(c.id)["r1_is_x"] for c in rrdb)
    for op in ("rrdb_u8", "tail_u8"):
        assert {c.swap for c in shapes if c.op == op} == {0, 1} == {c.swap for c in S.of("ties", op)}
    for kernel in KERNELS:
        assert {c.n for c in S.CASES if c.kernel == kernel} == {1, 2} or kernel == "rrdb_input_u8_kernel", kernel
    assert {c.n for c in S.of("input")} == {2} and {c.kind for c in S.of("input")} == {"1", "2"}
    assert {c.n for c in shapes if c.kernel == "rrdb_conv3x3_kernel<64>"} == {1, 2}
    for c in S.CASES:                                 # the largest tensor of the matrix: 2 x 16 x 49 x 200 f16, or its like
        assert all(v.numel() <= 2 * 16 * 49 * 200 for v in S.inputs(c.id).values() if torch.is_tensor(v)), c.id
        ho, wo = c.out_hw
        pitch = {"rrdb": S.inputs(c.id).get("out_pitch"), "layer": 72, "input": 32}.get(c.op, 3)
        assert c.n * ho * wo * pitch <= 2 * 16 * 49 * 200, c.id
    for c in shapes:                                  # different content per image, NaN in the channels past the ones read
        d = S.inputs(c.id)
        if c.n == 2:
            assert not torch.equal(d["x"][0], d["x"][1]), c.id
        if c.op in ("rrdb", "layer", "tail") and not c.alias:
            assert d["x"].shape[-1] > c.cin and bool(torch.isnan(d["x"][..., c.cin:]).all()), c.id
            for key in ("r1", "r2", "base"):
                t = d.get(key)
                if t is not None and t.shape[-1] > (3 if key == "base" else c.cout):
                    assert bool(torch.isnan(t[..., (3 if key == "base" else c.cout):]).all()), (c.id, key)


def test_the_u8_shape_cases_stay_under_the_share_cap():
    """The condition of the existing u8 tests, from the reference alone, on every new size: fewer than 2 % of the bytes
    within 255 e of a half-integer, both clamps reached.  A size over the cap gets another seed (S.U8_SEEDS), not another cap."""
    for c in S.of("shapes"):
        if c.op in ("rrdb_u8", "tail_u8"):
            r = S.expected(c.id)[0]
            share = S.near_share(c.id)
            print(f"{c.id}: near-half share {share:.4f}")
            assert share < 0.02, c.id
            assert bool((r.ref < 0).any()) and bool((r.ref > 1).any()), c.id


def test_the_exact_cases_are_exact_and_cover_the_combinations():
    exact = S.of("exact")
    rrdb = [c for c in exact if c.op == "rrdb"]
    assert {(c.cin, c.cout) for c in rrdb if c.alias} == {(a, b) for a in S.CINS for b in (32, 64)}
    assert {(c.cin, c.cout) for c in rrdb if c.ups} == {(a, b) for a in S.CINS if a <= 96 for b in (32, 64)}
    assert {(c.h, c.w) for c in exact} == set(S.EXACT_SIZES) == {(11, 17), (16, 49)} and {c.n for c in exact} == {2}
    for c in rrdb:
        d = S.inputs(c.id)
        assert (d["s0"], d["s1"], c.lrelu, c.res) == (0.5, 0.25, 0, "12") and (not c.alias or d["out_coff"] == c.cin)
        assert all(torch.equal(d[k], d[k].round()) for k in ("r1", "r2", "b")) and bool((d["r1"] != 0).any()) and bool((d["r2"] != 0).any())
    assert {(c.swap, c.base_pitch) for c in exact if c.op == "tail"} == {(0, 3), (0, 5), (1, 3), (1, 5)}
    assert {c.cin for c in exact if c.op == "layer"} == {32, 64}
    a = S.exact_slopes()
    assert all(not torch.equal(a.roll(r), a) for r in range(1, 64)) and bool((torch.log2(a.abs()) % 1 == 0).all()) and bool((a < 0).any())
    for c in exact:
        d, r = S.inputs(c.id), S.expected(c.id)
        assert torch.equal(r.ref, r.ref.half().double()) and float(r.ref.abs().max()) < 2048, c.id
        x = d["x"][..., :c.cin]
        assert set(x.unique().tolist()) == {0.0, 1.0, 2.0} and set(d["wt"].unique().tolist()) == {-1.0, 0.0, 1.0}
        assert not torch.equal(x[0], x[1])
        if c.op == "tail":
            assert not torch.equal(r.ref, r.ref.flip(1)), "the colours differ, so a swap shows"


def test_the_value_cases_reach_what_they_claim():
    facts = {c.id: S.value_facts(c.id) for c in S.of("values")}
    assert {c.kernel for c in S.of("values")} == KERNELS - {"rrdb_input_u8_kernel"} and {(c.h, c.w) for c in S.of("values")} == {(9, 33)}
    for c in S.of("values"):
        f = facts[c.id]
        print(c.id, {k: (round(v, 4) if isinstance(v, float) else v) for k, v in f.items()})
        d = S.inputs(c.id)
        if c.kind == "sub_x":
            assert f["sub_x"] == 1.0 and f["sub_out"] >= 0.10 and f["normal_out"] >= 0.10, "outputs in both ranges of f16"
            assert float(d["wt"].abs().mean()) > 0.25, "weights of order 1"
        elif c.kind == "sub_w":
            # activations of order 2^10 times weights of at least 2^-24: every product is a normal f16 or above, and so are the sums
            assert f["sub_w"] == 1.0 and 512 < float(d["x"][..., :c.cin].float().abs().mean()) < 2048 and f["normal_out"] > 0.9
        elif c.kind == "sat":
            assert f["x_at_max"] > 0 and f["x_max"] == S.F16_MAX and f["pos_inf"] > 0 and f["neg_inf"] > 0
            assert 1 <= len(f["inf_channels"]) <= 3 and f["finite"] > 10 * (f["pos_inf"] + f["neg_inf"]), "a few channels"
            r = S.expected(c.id)
            inf, _ = S.must_be_inf(r)
            assert bool(torch.isinf(r.ref[inf].half()).all())
        else:
            assert f["neg_zero_x"] > 0 and not bool(d["b"].any()) and f["zero_out"] > 0.25 and f["normal_out"] > 0.25
            if c.op == "layer":
                assert bool((d["slope"] == 0).any()) and bool((d["slope"] < 0).any())


def test_the_tie_cases_cover_every_m():
    m = np.arange(255)
    y = S.tie_y(m)
    assert y.dtype == np.float32 and S.TIES_EXACT == 255 and bool((y * np.float32(255) == (m + 0.5).astype(np.float32)).all())
    even = S.tie_byte(y)
    assert bool((even == m + (m % 2)).all()), "half to even"
    assert int((S.tie_byte(y, "u8_half_up") != even).sum()) == 128 and bool(((S.tie_byte(y, "u8_half_up") != even) == (m % 2 == 0)).all())
    assert bool(((S.tie_byte(y, "u8_truncate") != even) == (m % 2 == 1)).all())
    tail = S.of("ties", "tail_u8")
    assert len(tail) == 8 and {(c.h, c.w) for c in tail} == {(1, 1), (9, 33)} and sum(c.h == 1 for c in tail) == 4
    assert set(np.concatenate([S.tie_m(c) for c in tail]).tolist()) == set(range(255))
    for size in ((1, 1), (9, 33)):
        assert {c.swap for c in tail if (c.h, c.w) == size} == {0, 1}
    rrdb = [c for c in S.of("ties", "rrdb_u8") if c.kind == "bias"]
    ms = set(np.concatenate([S.tie_m(c) for c in rrdb]).tolist())
    assert all((c.h, c.w, c.res) == (1, 1, "") and S.inputs(c.id)["s0"] == 1.0 for c in rrdb)
    assert sum(v % 2 == 0 for v in ms) >= 16 and sum(v % 2 == 1 for v in ms) >= 16 and len(ms) >= 32
    mm, yy, r2, bias, valid = S._tie_r2_plan()
    assert bool(((bias[None, :] + r2.astype(np.float32) == yy) == valid).all()) and valid.sum() >= 3 and bool((bias != 0).all())
    assert (bias[None, :] + r2.astype(np.float32)).dtype == np.float32
    for c in S.of("ties"):
        d = S.inputs(c.id)
        assert not bool(d["x"].any()) and bool(d["wt"].any()) and ("base" not in d or not bool(d["base"][..., :3].any()))
    total = sum(int(S.expected(c.id)[1].sum()) for c in S.of("ties"))
    print(f"tie bytes compared: {total}; distinct m: tail 255, RRDB {len(ms)} by the bias and {len(set(mm[valid].tolist()))} through r2")


# ------------------------------------------------------------------------------------------------------- discrimination
STRUCTURAL = {k for k, v in S.MUTANTS.items() if v[2]}


def test_every_mutant_of_the_issue_is_mapped():
    assert set(S.MUTANTS) == {"tap_corner_00", "halo_col_32", "halo_row_8", "frag_col_16", "kchunk_last_nkc2", "kchunk_last_nkc6",
                              "taps_transposed", "bias_roll_1", "bias_roll_4", "bias_roll_16", "slope_roll_1", "slope_roll_4",
                              "slope_roll_16", "s0_s1_swapped", "r1_r2_swapped", "ups_source_round_up", "shuffle_dy_dx", "base_left",
                              "base_not_swapped", "store_f16_trunc", "weights_trunc"}
    assert set(S.MUTANTS) - STRUCTURAL == {"store_f16_trunc", "weights_trunc"} and S.U8_MUTANTS == ("u8_half_up", "u8_truncate")
    used = {v[0] for v in S.MUTANTS.values()}
    assert used == (set(RR.MUTANTS) | set(SR.CONV_MUTANTS) | set(SR.TAIL_MUTANTS)), "every mutant of the statements is held to a case"
    for label, (name, cid, _) in S.MUTANTS.items():
        c = S.BY_ID[cid]
        assert c.group == "shapes" and c.op in ("rrdb", "layer", "tail"), "a case the GPU file runs against the bound"
        assert name in {"rrdb": RR.MUTANTS, "layer": SR.CONV_MUTANTS, "tail": SR.TAIL_MUTANTS}[c.op]
    at = lambda label: S.BY_ID[S.MUTANTS[label][1]]
    assert at("halo_col_32").w > S.SR_TX and at("halo_row_8").h > S.SR_TY and at("frag_col_16").w % S.SR_TX == 16
    assert at("kchunk_last_nkc2").nkc == 2 and at("kchunk_last_nkc6").nkc == 6 and at("ups_source_round_up").ups == 1
    assert "1" in at("s0_s1_swapped").res and at("r1_r2_swapped").res == "12" and at("base_not_swapped").swap == 1
    assert at("tap_corner_00").h > 1 and at("tap_corner_00").w > 1


@pytest.mark.parametrize("label", sorted(S.MUTANTS))
def test_every_mutant_moves_its_case_past_the_bound(label):
    ratio = S.mutant_ratio(label)
    print(f"{label} on {S.MUTANTS[label][1]}: worst |mutant - statement| / bound = {ratio:.2f}")
    assert ratio >= (10.0 if label in STRUCTURAL else 1.0) and (label in STRUCTURAL or ratio > 1.0)


@pytest.mark.parametrize("mutant", S.U8_MUTANTS)
def test_the_rounding_mutants_change_the_tie_bytes(mutant):
    changed = S.tie_bytes_changed(mutant)
    print(f"{mutant}: {changed} tie bytes change")
    assert changed >= 100
    per_case = [int(((S.expected(c.id, mutant)[0] != S.expected(c.id)[0]) & S.expected(c.id)[1]).sum()) for c in S.of("ties", "tail_u8")]
    assert all(v > 0 for v in per_case), "every tail launch holds both parities of m"


def test_cases_that_cannot_see_a_mutant():
    """Why the cases are what they are.  Each mutant here is the statement itself, or within its bound."""
    # 8 x 32: no column 32, and the image does not end at the seam of the fragments
    cid = "shape_layer_8x32_cin64"
    for mutant in ("frag_col_16", "halo_col_32"):
        assert torch.equal(S.expected(cid, mutant).ref, S.expected(cid).ref), mutant
    # slopes of period 8 (tests/test_gpu_srvgg.py's integer case): a slope vector read 16 channels off is the same vector
    d = S.inputs("exact_layer_cin64_11x17")
    a8 = torch.tensor([0.5, 2.0, -0.25, 1.0, 0.125, -2.0, 0.0, 0.25]).repeat(8)
    x = S.nchw(d["x"])[:, :64]
    assert torch.equal(SR.conv_ref(x, d["wt"], d["b"], a8, mutant="slope_roll_16").ref, SR.conv_ref(x, d["wt"], d["b"], a8).ref)
    assert not torch.equal(S.expected("exact_layer_cin64_11x17", "slope_roll_16").ref, S.expected("exact_layer_cin64_11x17").ref)
    # the near-masked u8 cases: a half-up epilogue passes the check they make
    for cin, h, w, n, swap, res in RR.U8_CASES:
        wt, b, x_h, r1_h, r2_h = RR.u8_inputs(cin, h, w, n, swap, res)
        r = RR.conv_ref(RR.nchw(x_h), wt, b, s0=1.0, s1=0.5, r1=None if r1_h is None else RR.nchw(r1_h)[:, :3],
                        r2=None if r2_h is None else RR.nchw(r2_h)[:, :3])
        (byte, near), up = RR.u8_ref(r), RR.u8_ref(r, mutant="u8_half_up")[0]
        diff = (up - byte).abs()
        assert int(diff.max()) <= 1 and not (diff[~near] != 0).any()
    for h, w, n, swap, pitch in SR.U8_CASES:
        wt, b, x_h, base_h = SR.u8_inputs(h, w, n, swap, pitch)
        r = SR.tail_ref(SR.nchw(x_h), wt, b, SR.nchw(base_h)[:, :3])
        (byte, near), up = SR.u8_ref(r), SR.u8_ref(r, mutant="u8_half_up")[0]
        diff = (up - byte).abs()
        assert int(diff.max()) <= 1 and not (diff[~near] != 0).any()
    # 9 x 33: the second tile row is one row, and the row mutant moves nothing else
    d = S.inputs("value_zeros_rrdb32")
    g = torch.Generator().manual_seed(933)
    x = torch.randn((1, 64, 9, 33), generator=g).half().double()
    moved = (RR.conv_ref(x, d["wt"], d["b"], mutant="halo_row_8").ref != RR.conv_ref(x, d["wt"], d["b"]).ref)
    assert bool(moved[:, :, 8].any()) and not bool(moved[:, :, :8].any())
    # the integer weights of tests/test_gpu_rrdb.py are symmetric in (ky, kx): transposed taps are the same weights
    co, ci, ky, kx = torch.meshgrid(torch.arange(32), torch.arange(64), torch.arange(3), torch.arange(3), indexing="ij")
    old = ((co * 7 + ci * 3 + ky * 5 + kx * 11 + (co * ci) % 4) % 3 - 1).float()
    assert torch.equal(old, old.transpose(2, 3)) and not torch.equal(S.inputs("exact_rrdb_cin64_cout32")["wt"], S.inputs("exact_rrdb_cin64_cout32")["wt"].transpose(2, 3))


# ------------------------------------------------------------------------------------------------------- the packer
def _packer_values():
    """Every finite non-negative f16 value, the fp32 midpoint to its successor (65520 after 65504) and that midpoint's two
    fp32 neighbours, with both signs; then the named values."""
    v = np.arange(0x7c00, dtype=np.uint16).view(np.float16).astype(np.float64)
    nxt = np.append(v[1:], 65536.0)
    mid = ((v + nxt) / 2).astype(np.float32)
    assert bool((mid.astype(np.float64) == (v + nxt) / 2).all())
    four = np.concatenate([v.astype(np.float32), mid, np.nextafter(mid, np.float32(-np.inf)), np.nextafter(mid, np.float32(np.inf))])
    tiny = np.float32(2.0 ** -25)
    named = np.array([65504.0, 65519.99, 65520.0, tiny, np.nextafter(tiny, np.float32(0)), np.nextafter(tiny, np.float32(1)), np.inf, -np.inf,
                      np.nan, -65504.0, -65519.99, -65520.0, -tiny], np.float32)
    return np.concatenate([four, -four, named])


@pytest.mark.parametrize("net,cout", [("rrdb", 64), ("srvgg", 64), ("srvgg", 48)])
def test_the_packer_rounds_as_numpy(built_lib, net, cout):
    """elvis_<net>_pack_weights against numpy's astype(float16), bit for bit (NaN as NaN), and the padded channels zero."""
    lib = C.CDLL(built_lib)
    pack = getattr(lib, f"elvis_{net}_pack_weights")
    pack.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    vals = _packer_values()
    per = cout * 64 * 9
    calls = -(-len(vals) // per) if cout == 64 else 1          # the 48-channel layout: one call of it
    assert calls <= 8
    nans = 0
    for i in range(calls):
        chunk = np.resize(vals[i * per:], per)                  # the last call is filled up with its own first values
        w = np.ascontiguousarray(chunk.reshape(cout, 64, 3, 3).astype(np.float32))
        got = np.empty((2, 9, cout, 32), np.uint16)
        assert pack(w.ctypes.data, 64, cout, 64, cout, got.ctypes.data) == 0
        with np.errstate(over="ignore"):
            want = RR.pack_ref(w, 64, cout).view(np.uint16)
        nan = np.isnan(want.view(np.float16))
        assert bool(np.isnan(got.view(np.float16)[nan]).all()) and np.array_equal(got[~nan], want[~nan]), f"call {i}: the packer and numpy round differently"
        nans += int(nan.sum())
    assert nans >= 1 or cout == 48, "the NaN was among the values"
    # fewer real channels than packed ones: the rest is zero
    cin_real, cout_real = 50, cout - 7
    w = np.ascontiguousarray(np.resize(vals[1:], cout_real * cin_real * 9).reshape(cout_real, cin_real, 3, 3))
    w[np.isnan(w)] = 1.0
    got = np.full((2, 9, cout, 32), 0xFFFF, np.uint16)
    assert pack(w.ctypes.data, cin_real, cout_real, 64, cout, got.ctypes.data) == 0
    with np.errstate(over="ignore"):
        want = RR.pack_ref(w, 64, cout).view(np.uint16)
    assert np.array_equal(got, want)
    full = got.transpose(2, 0, 3, 1).reshape(cout, 64, 9)     # co, ci, tap
    assert not full[cout_real:].any() and not full[:, cin_real:].any() and full[:cout_real, :cin_real].any()


def test_the_packer_values_are_the_ones_asked_for():
    vals = _packer_values()
    assert len(vals) == 8 * 0x7c00 + 13 and len(vals) <= 7 * 64 * 64 * 9
    with np.errstate(over="ignore"):
        h = vals.astype(np.float16)
    assert int(np.isinf(h).sum()) > 4 and int(np.isnan(h).sum()) == 1 and int((h == 0).sum()) > 4
    assert len(np.unique(h[np.isfinite(h)].view(np.uint16))) == 2 * 0x7c00, "every finite f16 value of both signs is a result"


# ------------------------------------------------------------------------------------------------------- cost
def test_the_statement_values_of_the_new_cases_are_cheap():
    S.inputs.cache_clear(), S.expected.cache_clear()
    t = time.perf_counter()
    for c in S.CASES:
        S.expected(c.id)
    t = time.perf_counter() - t
    print(f"statement values of {len(S.CASES)} cases: {t:.2f} s")
    assert t < 60.0
