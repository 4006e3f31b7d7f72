"""CPU-side checks of the attention / Swin / DCNv2 matrix (tests/_modelref.py, tests/test_gpu_model_kernels_matrix.py):
the dispatch ledger (every window_attention_*, swin_fused_kernel and dcnv2_* instantiation in the built library is
reached by a matrix case) and a mutation self-test: each checker is fed CPU-made wrong outputs and
must reject every one of them."""
import math

import torch

import _modelref as R


def test_demangle():
    assert R.demangle_model("_ZN12_GLOBAL__N_117swin_fused_kernelILi192ELi2ELi1ELb1EEEvNS_8SwinArgsE") == \
        "swin_fused_kernel<192,2,1,true>"
    assert R.demangle_model("_ZN12_GLOBAL__N_126window_attention_tr_kernelEPKDF16_PS0_iiiiiiiPKff") == \
        "window_attention_tr_kernel"
    assert R.demangle_model("_ZN12_GLOBAL__N_123window_attention_kernelIDF16_EEvPKT_PS1_iiiiiiPKff") == \
        "window_attention_kernel<half>"
    assert R.demangle_model("_ZN12_GLOBAL__N_117dcnv2_tile_kernelILi7EEEvPKDF16_S2_S2_PKfPS0_iiiiiiiiiii") == \
        "dcnv2_tile_kernel<7>"
    assert R.demangle_model("_ZN12_GLOBAL__N_112dcnv2_kernelIfEEvPKT_S3_S3_PKfPS1_iiiiiiiiiiiii") == "dcnv2_kernel<float>"
    assert R.demangle_model("_ZN12_GLOBAL__N_121temporal_stack_kernelIfEEvPKhPT_iiiiiii") is None
    assert R.demangle_model("_ZN12_GLOBAL__N_119conv3x3_halo_kernelIDF16_Li128ELi256ELi8ELb1ELi3ELb0EEEvNS_8ConvArgsE") is None


def test_dispatch_ledger(built_lib):
    """The model-kernel instantiations of the built library == the ones the matrix's cases expect."""
    syms = R.model_kernel_symbols(built_lib)
    reached = {}
    for c in R.CASES:
        reached.setdefault(c.expect, c.id)
    missing = syms - set(reached)
    assert not missing, f"instantiations without a matrix case: {sorted(missing)}"
    stale = set(reached) - syms
    assert not stale, f"cases naming instantiations the library does not build: {sorted(stale)}"
    assert syms == set(reached)
    # every instantiation: attention tr + f32, the 12 (C, MODE) Swin pairs, DCNv2 tile<7>/<8> + generic
    assert len([s for s in reached if s.startswith("swin_fused_kernel")]) == 12
    assert {"window_attention_tr_kernel", "window_attention_kernel<float>", "dcnv2_tile_kernel<7>", "dcnv2_tile_kernel<8>",
            "dcnv2_kernel<half>", "dcnv2_kernel<float>"} <= set(reached)
    assert len(set(c.id for c in R.CASES)) == len(R.CASES)


def test_last_launch_is_bound(built_lib):
    from elvis_amd._lib import lib
    assert isinstance(lib().elvis_last_launch(), bytes)


# ------------------------------------------------------------------------------------------ mutation self-test
def _passes(y, b, floor=None):
    ok = R.tier1(y, b)[0]
    if floor is not None:
        ok = ok and R.tier2(y, b) >= floor
    return ok


# ---- window attention
def _attn_inputs(shift=4, h=16, w=24, heads=2):
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(1, h, w, 3 * heads * 32, generator=g).half().double()
    table = (torch.randn(225, heads, generator=g) * 1.5).float().double()
    return qkv, heads, shift, table, float(32 ** -0.5)


def test_attention_checks_accept_the_correct_output():
    qkv, heads, shift, table, scale = _attn_inputs()
    b = R.attention_ref(qkv, heads, shift, table, scale)
    ok, worst, _ = R.tier1(R.rne16(b.ref), b)
    assert ok and worst <= 0.5 + 1e-9
    bf = R.attention_ref(qkv, heads, shift, table, scale, f16=False)
    assert R.tier1(bf.ref.float().double(), bf)[0]


def _attn_rejects(**mut):
    qkv, heads, shift, table, scale = _attn_inputs()
    b = R.attention_ref(qkv, heads, shift, table, scale)
    y = R.rne16(R.attention_ref(qkv, heads, shift, table, scale, **mut).ref)
    assert not _passes(y, b), f"mutant {sorted(mut)} passes"
    bf = R.attention_ref(qkv, heads, shift, table, scale, f16=False)
    yf = R.attention_ref(qkv, heads, shift, table, scale, f16=False, **mut).ref.float().double()
    assert not _passes(yf, bf), f"mutant {sorted(mut)} passes the fp32 check"


def test_attention_rejects_a_transposed_relative_position_index():
    _attn_rejects(rpi=R.relative_position_index(8).T.contiguous())


def test_attention_rejects_a_missing_mask_on_the_last_window_column():
    m = R.shift_mask(16, 24, 8, 4).clone()
    nwx = 24 // 8
    m.view(16 // 8, nwx, 64, 64)[:, nwx - 1] = 0.0
    _attn_rejects(mask=m)


def test_attention_rejects_the_roll_with_the_wrong_sign():
    _attn_rejects(roll_sign=-1)


def test_attention_rejects_two_v_keys_swapped_inside_a_32_key_block():
    perm = torch.arange(64)
    perm[[37, 44]] = perm[[44, 37]]
    _attn_rejects(v_key_perm=perm)


def test_attention_rejects_the_next_heads_bias_column():
    _attn_rejects(head_of_bias=[1, 0])


# ---- fused Swin
def _swin_inputs(mode, C=64, n1=192, M=96):
    g = torch.Generator().manual_seed(12)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = (1.5 * rn(M, C) + 0.5 * rn(M, 1)).half().double()
    gam = (torch.rand(C, generator=g) + 0.5).float().double()
    bet = (rn(C) * 0.2).float().double()
    w1, b1 = (rn(n1, C) / math.sqrt(C)).half().double(), (rn(n1) * 0.1).float().double()
    w2 = (rn(C, n1) / math.sqrt(n1)).half().double()
    b2 = (rn(C) * 0.1).float().double()
    kw = {}
    if mode == 2:
        kw = dict(y=(1.5 * rn(M, C)).half().double(), wp=(rn(C, C) / math.sqrt(C)).half().double(),
                  bp=(rn(C) * 0.1).float().double())
    args = (mode, x, gam, bet, w1, b1) + ((w2, b2) if mode else ())
    return args, kw


def _swin_check(mode, y, **inputs):
    args, kw = _swin_inputs(mode)
    b = R.swin_ref(*args, **kw)
    return _passes(y, b, R.TIER2_FLOOR["swin"])


def _swin_mutant(mode, *, gamma_block=None, **mut):
    args, kw = _swin_inputs(mode)
    if gamma_block is not None:
        args = list(args)
        gm = args[2].clone()
        gm[gamma_block] = 1.0
        args[2] = gm
    return R.rne16(R.swin_ref(*args, **kw, **mut).ref)


def test_swin_checks_accept_the_correct_output():
    for mode in (0, 1, 2):
        args, kw = _swin_inputs(mode)
        b = R.swin_ref(*args, **kw)
        y = R.rne16(b.ref)
        assert R.tier1(y, b)[0] and R.tier2(y, b) == 1.0


def test_swin_rejects_a_dropped_last_hidden_chunk():
    for mode in (1, 2):
        assert not _swin_check(mode, _swin_mutant(mode, drop_last_chunk=True))


def test_swin_rejects_two_hidden_rows_of_fc2_swapped():
    perm = torch.arange(192)
    perm[[133, 138]] = perm[[138, 133]]      # two k values of one 32-deep fragment of the last chunk
    for mode in (1, 2):
        assert not _swin_check(mode, _swin_mutant(mode, w2_cols=perm))


def test_swin_rejects_gamma_missing_on_one_32_channel_block():
    for mode in (0, 1, 2):
        assert not _swin_check(mode, _swin_mutant(mode, gamma_block=slice(32, 64)))


def test_swin_rejects_a_missing_residual():
    for mode in (1, 2):
        assert not _swin_check(mode, _swin_mutant(mode, residual=False))


def test_swin_rejects_linear_rows_permuted_inside_a_16_channel_group():
    args, kw = _swin_inputs(0)
    b = R.swin_ref(*args, **kw)
    perm = torch.arange(192)
    perm[[16 * 5 + 3, 16 * 5 + 12]] = perm[[16 * 5 + 12, 16 * 5 + 3]]
    assert not _passes(R.rne16(b.ref)[:, perm], b, R.TIER2_FLOOR["swin"])


def test_swin_rejects_truncated_outputs_in_tier_2():
    for mode in (0, 1, 2):
        args, kw = _swin_inputs(mode)
        b = R.swin_ref(*args, **kw)
        y = R.trunc16(b.ref)
        assert R.tier2(y, b) < R.TIER2_FLOOR["swin"], f"mode {mode}: truncation passes tier 2"


# ---- DCNv2
def _dcn_inputs(positive=False, cin=7, cout=24, h=16, w=40):
    g = torch.Generator().manual_seed(13)
    x = torch.randn(1, h, w, cin, generator=g)
    off = (torch.randn(1, h, w, 18 * cin, generator=g) * 2.0).clamp(-5.0, 5.0)
    mk = torch.randn(1, h, w, 9 * cin, generator=g) * 2.0
    wt = torch.randn(cout, cin * 9, generator=g) / math.sqrt(cin * 9)
    if positive:
        x, wt = x.abs() + 0.5, wt.abs()
    b = (torch.randn(cout, generator=g) * 0.1).float().double()
    return x.half().double(), torch.cat([off, mk], -1).half().double(), wt.half().double(), b, cin


def _dcn_rejects(tile, positive=False, **mut):
    x, om, wt, b, dg = _dcn_inputs(positive)
    ref = R.dcn_ref(x, om, wt, b, dg, True, tile=tile, f16_out=True)
    mut_sig = mut.pop("mask_sigmoid", True)
    y = R.rne16(R.dcn_ref(x, om, wt, b, dg, mut_sig, tile=tile, f16_out=True, **mut).ref)
    return _passes(y, ref, R.TIER2_FLOOR["dcn"] if tile else None)


def test_dcn_checks_accept_the_correct_output():
    for tile in (False, True):
        x, om, wt, b, dg = _dcn_inputs()
        ref = R.dcn_ref(x, om, wt, b, dg, True, tile=tile, f16_out=True)
        assert R.tier1(R.rne16(ref.ref), ref)[0] and R.tier2(R.rne16(ref.ref), ref) == 1.0
        assert bool((ref.ref != 0).any())


def test_dcn_rejects_a_skipped_sigmoid():
    for tile in (False, True):
        assert not _dcn_rejects(tile, mask_sigmoid=False)


def test_dcn_rejects_dy_dx_swapped():
    for tile in (False, True):
        assert not _dcn_rejects(tile, swap_dydx=True)


def test_dcn_rejects_edge_clamped_corners():
    for tile in (False, True):
        assert not _dcn_rejects(tile, clamp_edges=True)


def test_dcn_rejects_the_next_groups_mask():
    for tile in (False, True):
        assert not _dcn_rejects(tile, mask_group_shift=1)


def test_dcn_rejects_truncated_samples_in_tier_2():
    x, om, wt, b, dg = _dcn_inputs(positive=True)
    ref = R.dcn_ref(x, om, wt, b, dg, True, tile=True, f16_out=True)
    y = R.rne16(R.dcn_ref(x, om, wt, b, dg, True, tile=True, f16_out=True, trunc_samples=True).ref)
    assert R.tier2(y, ref) < R.TIER2_FLOOR["dcn"]
