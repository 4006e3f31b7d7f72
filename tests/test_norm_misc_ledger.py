"""CPU-side checks of the norm / misc matrix (tests/_normref.py, tests/test_gpu_norm_misc_matrix.py): the ledger (every
kernel of csrc/norm.hip and csrc/misc.hip in the built library is named by a case or by an exact-equality test), the CPU
pins (bicubic against F.interpolate in float64, the gn_blocks restatement), and a mutation self-test: each checker is
fed CPU-made wrong outputs and must reject every one, and must accept the correctly rounded reference."""
import numpy as np
import torch
import torch.nn.functional as F

import _normref as R


# ------------------------------------------------------------------------------------------------------- ledger
def test_demangle():
    assert R.demangle_norm_misc("_ZN12_GLOBAL__N_117affine_act_kernelIDF16_Lb0EEEvPKT_PS1_iiiiPKfS6_ix") == \
        "affine_act_kernel<half,false>"
    assert R.demangle_norm_misc("_ZN12_GLOBAL__N_116layernorm_kernelIfEEvPKT_PS1_xiiiPKfS6_fii") == "layernorm_kernel<float>"
    assert R.demangle_norm_misc("_ZN12_GLOBAL__N_126gn_partials_reduce4_kernelEPKfiiPdii") == "gn_partials_reduce4_kernel"
    assert R.demangle_norm_misc("_ZN12_GLOBAL__N_118convert_act_kernelIDF16_fEEvPKT_PT0_x") == "convert_act_kernel<half,float>"
    assert R.demangle_norm_misc("_ZN12_GLOBAL__N_112dcnv2_kernelIfEEvPKT_S3_S3_PKfPS1_iiiiiiiiiiiii") is None


def test_kernel_ledger(built_lib):
    """The norm.hip / misc.hip kernels of the built library == the ones the cases and the exact tests name."""
    syms = R.norm_misc_kernel_symbols(built_lib)
    named = {c.expect for c in R.CASES} | R.EXACT_KERNELS | {
        "gn_channel_sums_kernel<half>", "gn_channel_sums_kernel<float>"}
    missing = syms - named
    assert not missing, f"kernels without a matrix case or an exact test: {sorted(missing)}"
    stale = named - syms
    assert not stale, f"cases naming kernels the library does not build: {sorted(stale)}"
    assert len(syms) == 23
    assert len({c.id for c in R.CASES}) == len(R.CASES)
    for op in ("gn_sums", "partials", "gn_affine", "gn_e2e", "affine_act", "layernorm", "bicubic"):
        assert any(c.op == op for c in R.CASES)


def test_the_cases_cover_the_branches():
    f = lambda **kw: [c for c in R.CASES if all(getattr(c, k) == v for k, v in kw.items())]
    # GN sums: one pixel, fewer pixels than pixel lanes, one slab, one slab + 1, the hw / 2048 branch, pl = 1
    for dt in ("f16", "f32"):
        _, ppb, pl = R.gn_blocks(dt == "f16", 1000, 64)
        assert {1, pl - 1, ppb, ppb + 1} <= {c.hw for c in f(op="gn_sums", dt=dt, c=64)}
    big = [c for c in f(op="gn_sums") if c.hw > 2048 * 16 * R.gn_blocks(c.dt == "f16", c.hw, c.c)[2]]
    assert big and all(R.gn_blocks(c.dt == "f16", c.hw, c.c)[1] == (c.hw + 2047) // 2048 for c in big)
    assert {8, 64, 100, 160, 320, 640, 2048} <= {c.c for c in f(op="gn_sums", dt="f16")}
    assert {8, 12, 64, 100, 160, 320, 640, 1024} <= {c.c for c in f(op="gn_sums", dt="f32")}
    assert {1, 255, 256, 257, 1000} == {c.tiles for c in f(op="partials", expect="gn_partials_reduce4_kernel")}
    assert any(c.misalign for c in f(op="partials")) and any(c.c % 4 for c in f(op="partials"))
    # LayerNorm: lpt 1 .. 64, the wave loop
    assert {R.ln_lpt(c.c, True) for c in f(op="layernorm", dt="f16")} == {1, 8, 16, 32, 64}
    assert {R.ln_lpt(c.c, False) for c in f(op="layernorm", dt="f32")} == {1, 4, 16, 64}
    assert any(c.hw > 256 * 16 * 4 * (64 // R.ln_lpt(c.c, c.dt == "f16")) for c in f(op="layernorm"))
    assert any(c.n * c.hw * ((c.c + 7) // 8) > 256 * 32 * 256 for c in f(op="affine_act", dt="f16"))
    assert {c.sf for c in f(op="bicubic")} == {1, 2, 3, 4} and {c.c for c in f(op="bicubic")} == {1, 3, 4, 8}


# ------------------------------------------------------------------------------------------------------- CPU pins
def test_gn_blocks_restatement():
    """ceil(hw / ppb) workgroups of max(ceil(hw / 2048), 16 pl) pixels: never more than 2048 + a few, every pixel covered."""
    for f16 in (True, False):
        for c in (1, 8, 12, 64, 100, 640, 1024, 2048 if f16 else 1000):
            for hw in (1, 15, 16, 17, 511, 512, 513, 4096, 2048 * 16 + 1, 2048 * 600 + 7):
                tiles, ppb, pl = R.gn_blocks(f16, hw, c)
                assert tiles * ppb >= hw > (tiles - 1) * ppb and ppb >= 16 * pl and pl >= 1
                assert pl * ((c + (8 if f16 else 4) - 1) // (8 if f16 else 4)) <= 256
                assert R.gn_workspace_floats(f16, 3, hw, c) == 3 * tiles * c * 2
                assert R.gn_sums_k(f16, hw, c) == -(-ppb // pl) + pl


def test_bicubic_ref_equals_interpolate_in_float64():
    g = torch.Generator().manual_seed(3)
    for sf in (1, 2, 3, 4):
        for h, w in ((1, 1), (2, 3), (3, 1), (13, 17)):
            x = torch.randn(2, h, w, 3, generator=g, dtype=torch.float64)
            ref = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=sf, mode="bicubic", align_corners=False)
            mine = R.bicubic_ref(x, sf, False).ref.permute(0, 3, 1, 2)
            assert float((mine - ref).abs().max()) <= 1e-12, (sf, h, w)


def test_half_ties_exist_for_even_and_odd_k():
    ties = R.half_ties(range(255))
    assert len(ties) > 20 and {k % 2 for k in ties} == {0, 1}
    for k, (lo, t, hi) in ties.items():
        q = lambda v: np.float32(v) * np.float32(255.0)
        assert q(t) == k + 0.5 and q(lo) < k + 0.5 < q(hi)


# ------------------------------------------------------------------------------------------------------- mutants
def _passes(y, b, tier2=False):
    ok = R.tier1(y, b)[0]
    if tier2 and ok:
        ok = R.tier2(y, b) >= R.TIER2_FLOOR and R.exact_share(y, b) >= R.exact_share_floor(b)[0]
    return ok


def _accepts_rounded(b, out_f16):
    y = R.rne16(b.ref) if out_f16 else b.ref.float().double()
    # the bound is 1/2 ulp + e1 and a correct rounding may sit a whole 1/2 ulp from the reference: with e1 far below an
    # ulp (every op here) the ratio of the correctly rounded reference approaches 1, and 0.5 where e1 >= 1/2 ulp
    ok, worst, _ = R.tier1(y, b)
    assert ok and worst <= 1.0, worst
    if out_f16:
        assert R.tier2(y, b) == 1.0 and R.exact_share(y, b) == 1.0


def _gn_x(n=2, hw=1500, c=64, mean=1.0, f16=True, seed=21, std=1.0):
    g = torch.Generator().manual_seed(seed)
    x = mean + std * (torch.randn(n, hw, c, generator=g) + 0.3 * torch.randn(1, 1, c, generator=g))
    return (x.half() if f16 else x.float()).double()


def _gn_params(c=64, seed=22):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(c, generator=g) + 0.5).float().double(), (torch.randn(c, generator=g) * 0.3).float().double()


def test_gn_sums_accepts_exact_and_rejects_a_dropped_slab():
    for f16 in (True, False):
        x = _gn_x(f16=f16)
        b = R.gn_sums_ref(x, f16)
        assert R.tier1(b.ref, b)[0]
        tiles = R.gn_blocks(f16, x.shape[1], x.shape[2])[0]
        assert tiles > 2
        for slab in (0, tiles - 1):
            assert not _passes(R.gn_sums_ref(x, f16, drop_slab=slab).ref, b)
        # an fp32 accumulation gone one digit wrong (a relative 1e-5 of sum |x|) is rejected too
        assert not _passes(b.ref + 1e-5 * torch.stack([x.abs().sum(1), (x * x).sum(1)], -1), b)


def test_partials_rejects_a_missing_row():
    p = (torch.randn(2, 300, 8, 2, generator=torch.Generator().manual_seed(5)) * 50 + 20).float().double()
    b = R.partials_ref(p)
    assert R.tier1(b.ref, b)[0]
    for row in (0, 255, 256, 299):
        assert not _passes(R.partials_ref(p, drop_row=row).ref, b)
    assert not _passes(b.ref * (1 + 1e-12), b)


def _affine_args(hw=400, c=160, seed=31):
    x = _gn_x(n=3, hw=hw, c=c, mean=2.0, f16=False, seed=seed)
    sums = torch.stack([x.sum(1), (x * x).sum(1)], -1)
    gam, bet = _gn_params(c, seed + 1)
    return sums, gam, bet, hw


def test_gn_affine_rejects_unbiased_variance_and_eps_outside_the_root():
    sums, gam, bet, hw = _affine_args()
    for sc, sh in ((None, None), (gam * 0.1, None), (None, bet), (gam * 0.1, bet)):
        b = R.gn_affine_ref(sums, gam, bet, sc, sh, hw, 32, 1e-5)
        _accepts_rounded(b, False)
        assert not _passes(R.gn_affine_ref(sums, gam, bet, sc, sh, hw, 32, 1e-5, biased=False).ref.float().double(), b)
        assert not _passes(R.gn_affine_ref(sums, gam, bet, sc, sh, hw, 32, 1e-5, eps_outside=True).ref.float().double(), b)
    # the weakest GN mutant: unbiased variance over cnt = 2000 elements moves rstd by 2.5e-4 relative


def test_groupnorm_rejects_wrong_variance_and_quick_gelu():
    for f16 in (True, False):
        for mean in (0.0, 3.0, 30.0):
            x = _gn_x(mean=mean, f16=f16)
            gam, bet = _gn_params()
            for act in (0, 2):
                b = R.groupnorm_ref([x], f16, gam, bet, None, None, 32, 1e-5, act)
                _accepts_rounded(b, f16)
                store = (lambda t: R.rne16(t)) if f16 else (lambda t: t.float().double())
                n, hw, c = x.shape
                sums = torch.stack([x.sum(1), (x * x).sum(1)], -1)
                # unbiased variance over cnt = 3000 moves rstd by 1.7e-4 relative.  At mean / std = 30 the variance the
                # kernel forms from fp32 partials is itself only good to gamma(48) 2 (mean^2 + var) / var = 5e-3, and the
                # bound - which has to carry that - cannot tell the two apart: the GroupNorm-affine check (exact sums) does
                ab = R.gn_affine_ref(sums, gam, bet, None, None, hw, 32, 1e-5, biased=False).ref
                if mean < 30.0:
                    assert not _passes(store(R.affine_act_ref(x, ab[0], ab[1], act, f16).ref), b, tier2=f16), (f16, mean, act)
                # eps outside the root: at var ~ 1 it moves rstd by 5e-6 relative - 1/200 of an f16 ulp and below the
                # variance's own error from fp32 partials once mean / std >= 3 (the weakest mutant: the GroupNorm-affine
                # check on exact sums rejects it there); on an image of std 0.01, where eps matters, every case sees it
                xs_ = _gn_x(mean=mean * 0.01, f16=f16, std=0.01)
                bs_ = R.groupnorm_ref([xs_], f16, gam, bet, None, None, 32, 1e-5, act)
                sm = torch.stack([xs_.sum(1), (xs_ * xs_).sum(1)], -1)
                ab = R.gn_affine_ref(sm, gam, bet, None, None, hw, 32, 1e-5, eps_outside=True).ref
                assert not _passes(store(R.affine_act_ref(xs_, ab[0], ab[1], act, f16).ref), bs_, tier2=f16), (f16, mean, act)
                if act == 2:
                    ab = R.gn_affine_ref(sums, gam, bet, None, None, hw, 32, 1e-5).ref
                    y = store(R.affine_act_ref(x, ab[0], ab[1], 2, f16, quick_gelu=True).ref)
                    assert not _passes(y, b, tier2=f16)


def test_affine_act_rejects_quick_gelu_and_accepts_saturation():
    g = torch.Generator().manual_seed(41)
    for f16 in (True, False):
        x = torch.randn(2, 300, 12, generator=g) * 2
        x = (x.half() if f16 else x.float()).double()
        pa, pb = torch.randn(2, 12, generator=g).float().double(), torch.randn(2, 12, generator=g).float().double()
        for act in (0, 2):
            _accepts_rounded(R.affine_act_ref(x, pa, pb, act, f16), f16)
        b = R.affine_act_ref(x, pa, pb, 2, f16)
        y = R.affine_act_ref(x, pa, pb, 2, f16, quick_gelu=True).ref
        assert not _passes(R.rne16(y) if f16 else y.float().double(), b, tier2=f16)
        # t = -100: the kernel's 1 + exp(100) is inf and the output -0; the reference (-3.7e-42) must accept that
        xs = torch.tensor([-100.0, -20.0, 0.0, 20.0, 100.0]).view(1, 5, 1).double()
        one, zero = torch.ones(1, 1, dtype=torch.float64), torch.zeros(1, 1, dtype=torch.float64)
        bs = R.affine_act_ref(xs, one, zero, 2, f16)
        ys = bs.ref.clone()
        ys[0, 0, 0] = -0.0
        assert _passes(R.rne16(ys) if f16 else ys.float().double(), bs)
        ys[0, 0, 0] = float("nan")
        assert not _passes(ys, bs)


def _ln_inputs(c, f16, seed=51, T=120):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, c, generator=g) * 1.5 + 0.5 * torch.randn(T, 1, generator=g)
    gam, bet = _gn_params(c, seed + 1)
    return (x.half() if f16 else x.float()).double(), gam, bet


def test_layernorm_rejects_a_dropped_lane_and_the_wrong_divisor():
    for f16, cs in ((True, (64, 96, 192, 512)), (False, (12, 64, 192, 256))):
        store = (lambda t: R.rne16(t)) if f16 else (lambda t: t.float().double())
        for c in cs:
            x, gam, bet = _ln_inputs(c, f16)
            b = R.layernorm_ref(x, gam, bet, 1e-5, f16)
            _accepts_rounded(b, f16)
            lanes = c // (8 if f16 else 4)
            for lane in (0, lanes - 1):
                assert not _passes(store(R.layernorm_ref(x, gam, bet, 1e-5, f16, drop_lane=lane).ref), b, tier2=f16), (c, lane)
            if R.ln_lpt(c, f16) != lanes:      # c = 64 etc.: lpt * VEC == c and the mutant is the kernel
                assert not _passes(store(R.layernorm_ref(x, gam, bet, 1e-5, f16, mean_over_lanes=True).ref), b, tier2=f16), c
    # a token of mean 100, std 0.1: the bound carries the cancellation and still rejects a dropped lane
    g = torch.Generator().manual_seed(52)
    x = (100.0 + 0.1 * torch.randn(50, 192, generator=g)).half().double()
    gam, bet = _gn_params(192, 53)
    b = R.layernorm_ref(x, gam, bet, 1e-5, True)
    _accepts_rounded(b, True)
    assert not _passes(R.rne16(R.layernorm_ref(x, gam, bet, 1e-5, True, drop_lane=3).ref), b)


def test_bicubic_rejects_the_wrong_kernel_border_and_centres():
    g = torch.Generator().manual_seed(61)
    for f16 in (True, False):
        store = (lambda t: R.rne16(t)) if f16 else (lambda t: t.float().double())
        x = torch.randn(1, 13, 17, 3, generator=g)
        x = (x.half() if f16 else x.float()).double()
        for sf in (2, 3, 4):
            b = R.bicubic_ref(x, sf, f16)
            _accepts_rounded(b, f16)
            for mut in (dict(A=-0.5), dict(clamp=False), dict(align_corners=True)):
                assert not _passes(store(R.bicubic_ref(x, sf, f16, **mut).ref), b, tier2=f16), (f16, sf, mut)


def test_vq_rejects_last_minimum_and_fused_distance():
    g = torch.Generator().manual_seed(71)
    cb = torch.randn(1024, 3, generator=g).float()
    lo = torch.randint(0, 128, (200,), generator=g)
    cb[lo + 519] = cb[lo]
    z = cb[lo].numpy()
    idx, zq = R.vq_ref(z, cb.numpy())
    assert (idx == lo.numpy()).all()
    idx_last, _ = R.vq_ref(z, cb.numpy(), last_wins=True)
    assert (idx_last != idx).any()
    # a fused multiply-add distance: codes (a, b) and (b, a) are exactly equidistant from 0 and tie without contraction
    # (the first wins); fma(b, b, fl(a a)) and fma(a, a, fl(b b)) round differently and break the tie the other way
    rng = np.random.default_rng(7)
    differ = 0
    for _ in range(64):
        a, b = rng.standard_normal(2).astype(np.float32)
        pair = np.array([[a, b], [b, a]], np.float32)
        zz = np.zeros((1, 2), np.float32)
        assert R.vq_ref(zz, pair)[0][0] == 0
        differ += int(R.vq_ref(zz, pair, fused=True)[0][0] != 0)
    assert differ > 5, "the fused-distance mutant is indistinguishable on these inputs"


def test_u8_float_reject_rounding_swap_and_truncation_mutants():
    v = np.arange(256, dtype=np.uint8)
    src = np.stack([v, np.roll(v, 85), np.roll(v, 170)], -1)
    ref = R.u8_to_float_ref(src, 2.0, -1.0, 1, 1, False, 8)
    assert not R.bits_equal(ref, R.u8_to_float_ref(src, 2.0, -1.0, 1, 1, False, 8, swap_back=False))
    # v / 255 * 2 - 1 as one float64 expression rounded once differs from the three float32 operations somewhere
    once = np.zeros_like(ref)
    once[:, :3] = (src[:, ::-1].astype(np.float64) / 255.0 * 2.0 - 1.0).astype(np.float32)
    assert not R.bits_equal(ref, once)
    ties = R.half_ties(range(255))
    t = np.array([x for k in sorted(ties) for x in ties[k]], np.float32)
    t = t[: t.size // 3 * 3].reshape(-1, 3)
    r0, _ = R.float_to_u8_ref(t, 1.0, 0.0, 0, 0)
    r1, _ = R.float_to_u8_ref(t, 1.0, 0.0, 1, 0)
    up, _ = R.float_to_u8_ref(t, 1.0, 0.0, 0, 0, half_up=True)
    assert (r0 != r1).any(), "truncation where rounding is specified must show"
    assert (r0 != up).any(), "round-half-up must differ from half-even on the even-k ties"
    assert (r1 != up).any()
    nan = np.array([[np.nan, -np.inf, np.inf]], np.float32)
    assert R.float_to_u8_ref(nan, 1.0, 0.0, 0, 0)[0].tolist() == [[0, 0, 255]]
    sw, _ = R.float_to_u8_ref(t, 1.0, 0.0, 0, 1)
    assert (sw != r0).any()


def test_convert_rejects_truncation_and_pad_rejects_symmetric():
    a = R.f32_to_f16_inputs()
    ref = R.convert_ref(a, True)
    tr = R.trunc_f16(a)
    assert not R.bits_equal(ref, tr, nan_as_nan=True)
    assert R.bits_equal(ref, ref.copy(), nan_as_nan=True)
    x = np.random.default_rng(1).standard_normal((1, 5, 6, 3)).astype(np.float32)
    r = R.pad_reflect_axpy_ref(x, 8, 9, 0.5, None, 0.0, False)
    assert R.bits_equal(r[:, :5, :6], (x * np.float32(0.5)))
    assert R.bits_equal(r[:, 5], r[:, 3]) and R.bits_equal(r[:, :, 6], r[:, :, 4])      # reflect: edge not repeated
    assert not R.bits_equal(r, R.pad_reflect_axpy_ref(x, 8, 9, 0.5, None, 0.0, False, symmetric=True))
