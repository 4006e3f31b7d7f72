"""CPU-side checks of the conv test matrix (tests/_convref.py, tests/test_gpu_conv_matrix.py): the dispatch
ledger (every conv kernel instantiation in the built library is reached by a matrix case),
the name query against the dispatch rule, the statistics grid against the tile height in the resolved kernel's name,
and a mutation self-test of the tier-1 / tier-2 / statistics checks."""
import ctypes as C
import math

import torch

import _convref as R


def _syms(path):
    return {n for n in (R.demangle_conv(s) for s in R.elf_symbols(path)) if n is not None}


def test_demangle():
    assert R.demangle_conv("_ZN12_GLOBAL__N_119conv3x3_halo_kernelIDF16_Li128ELi256ELi8ELb1ELi3ELb0EEEvNS_8ConvArgsE") == \
        "conv3x3_halo_kernel<half,128,256,8,true,3,false>"
    assert R.demangle_conv("_ZN12_GLOBAL__N_117conv_igemm_kernelIfLi4ELi2ELi1ELi4EEEvNS_8ConvArgsE") == \
        "conv_igemm_kernel<float,4,2,1,4>"
    assert R.demangle_conv("_ZN12_GLOBAL__N_117conv3x3_ws_kernelILi2ELi64ELb1EEEvNS_8ConvArgsEii") == "conv3x3_ws_kernel<2,64,true>"
    assert R.demangle_conv("_ZN12_GLOBAL__N_116layernorm_kernelIfEEvPKT_PS1_xiiiPKfS6_fi") is None
    assert R.normalize_kernel_name("void (anonymous namespace)::conv3x3_ws_kernel<2, 64, true>((anonymous namespace)::ConvArgs, int, int)") \
        == "conv3x3_ws_kernel<2,64,true>"
    assert R.normalize_kernel_name("(anonymous namespace)::conv3x3_halo_kernel<_Float16, 64, 256, 16, true, 3, false>(ConvArgs)") \
        == "conv3x3_halo_kernel<half,64,256,16,true,3,false>"
    assert R.normalize_kernel_name("_ZN12_GLOBAL__N_117conv_igemm_kernelIDF16_Li4ELi2ELi1ELi4EEEvNS_8ConvArgsE") == \
        "conv_igemm_kernel<half,4,2,1,4>"


def test_dispatch_ledger(built_lib):
    """The conv instantiations of the built library == the names the matrix's cases resolve to."""
    syms = _syms(built_lib)
    assert len(syms) >= 100, f"only {len(syms)} conv kernel symbols decoded"
    reached = {}
    for c in R.CASES:
        for name in R.resolve(c):
            assert name == c.expect, f"{c.id} resolves to {name}, expected {c.expect}"
            reached.setdefault(name, c.id)
    missing = syms - set(reached)
    assert not missing, f"instantiations without a matrix case: {sorted(missing)}"
    stale = set(reached) - syms
    assert not stale, f"cases naming instantiations the library does not build: {sorted(stale)}"
    assert syms == set(reached)
    assert len(set(c.id for c in R.CASES)) == len(R.CASES)


def _name(d, res=0, st=0):
    from elvis_amd._lib import lib, check
    buf = C.create_string_buffer(128)
    check(lib().elvis_conv_kernel_name_for_call(C.byref(d), res, st, buf, len(buf)), None)
    return buf.value.decode()


def test_name_query_follows_call_flags(built_lib):
    """A ws-eligible shape runs on the weight-stationary kernel only without residual and statistics."""
    from elvis_amd import ops
    from elvis_amd._lib import lib
    ws = R.Case(id="q", expect="", cin=32, cout=64, h=72, w=1920)
    d, _, _ = R.descs(ws)[0]
    assert _name(d).startswith("conv3x3_ws_kernel<1,64,")
    assert ops.conv_kernel_name(d) == _name(d)
    buf = C.create_string_buffer(128)
    assert lib().elvis_conv_kernel_name(C.byref(d), buf, len(buf)) == 0 and buf.value.decode() == _name(d, 0, 0)
    for res, st in ((1, 0), (0, 1), (1, 1)):
        assert _name(d, res, st) == "conv3x3_halo_kernel<half,64,256,16,false,3,false>"
        assert ops.conv_kernel_name(d, residual=bool(res), stats=bool(st)) == _name(d, res, st)
    # shapes off the ws path: the flags change nothing
    for c in (R.Case(id="a", expect="", cin=64, cout=128, h=16, w=40),
              R.Case(id="b", expect="", cin=64, cout=64, ksize=1, h=16, w=40),
              R.Case(id="c", expect="", dt="f32", cin=16, cout=32, h=9, w=9, stride=2),
              R.Case(id="d", expect="", cin=32, cout=32, h=8, w=8, kind="up")):
        for d, _, _ in R.descs(c):
            assert _name(d, 1, 1) == _name(d, 0, 0) == ops.conv_kernel_name(d)


def test_stats_grid_follows_the_named_kernels_tile_height(built_lib):
    """elvis_conv_stats_tiles sizes the statistics grid with the tile height in the launched kernel's own name."""
    from elvis_amd._lib import lib
    halo = ("conv3x3_halo_kernel", "conv3x3_halo_x3_kernel", "conv3x3_x3p_kernel")
    checked = 0
    for c in R.CASES:
        for (d, _, _), name in zip(R.descs(c), R.resolve(c)):
            if not name.startswith(tuple(h + "<" for h in halo)):
                continue
            parity = d.ksize == 2 and d.subpixel != 5   # the sub-pixel parity form: one launch per parity, low-res grid
            rows, cols = (d.h, d.w) if parity else (d.ho, d.wo)
            want = d.n * math.ceil(rows / R.kernel_ty(name)) * math.ceil(cols / 32)
            assert lib().elvis_conv_stats_tiles(C.byref(d)) == want, f"{c.id}: {name}"
            checked += 1
    assert checked >= 50


# ------------------------------------------------------------------------------------------ mutation self-test
def _small():
    g = torch.Generator().manual_seed(7)
    n, cin, cout, h, w = 1, 40, 8, 10, 40   # 40 input channels: one whole K chunk + a partial one; two tile columns
    x = torch.randn(n, cin, h, w, generator=g).half().double()
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).float()
    b = (torch.randn(cout, generator=g) * 0.1).float().double()
    return x, wt, b


def _ref(x, wt, b):
    return R.conv_ref(x, wt.half().double(), b, None, ksize=3)


def _passes(y, r):
    return R.tier1(y, r)[0] and R.tier2(y, r) >= R.TIER2_FLOOR


def test_checks_accept_the_correct_output():
    x, wt, b = _small()
    r = _ref(x, wt, b)
    y = R.rne16(r.ref)
    ok, worst, _ = R.tier1(y, r)
    assert ok and worst < 1.0
    assert R.tier2(y, r) == 1.0
    st = R.tile_stats_ref(y, 8)
    assert R.stats_check(st[..., :2].float(), st)[0]


def _mutant(x, wt, b, *, mask_x=None, w_hat=None, bias=None):
    r = R.conv_ref(x if mask_x is None else x * mask_x, wt.half().double() if w_hat is None else w_hat,
                   b if bias is None else bias, None, ksize=3)
    return R.rne16(r.ref)


def test_checks_reject_a_dropped_corner_tap():
    x, wt, b = _small()
    r = _ref(x, wt, b)
    y = R.rne16(r.ref)
    # pixel (0, 0) without its tap (dy, dx) = (2, 2), i.e. input pixel (1, 1)
    w_hat = wt.half().double()
    y[0, :, 0, 0] = R.rne16(r.ref[0, :, 0, 0] - (x[0, :, 1, 1][None, :] * w_hat[:, :, 2, 2]).sum(1))
    assert not _passes(y, r)


def test_checks_reject_a_shifted_halo_column():
    x, wt, b = _small()
    r = _ref(x, wt, b)
    y = R.rne16(r.ref)
    xs = x.clone()
    xs[..., 1:] = x[..., :-1]   # the input shifted right by one column ...
    ys = _mutant(xs, wt, b)
    y[..., 32] = ys[..., 32]    # ... as seen by the first column of the second tile
    assert not _passes(y, r)


def test_checks_reject_the_neighbouring_channels_bias():
    x, wt, b = _small()
    r = _ref(x, wt, b)
    assert not _passes(_mutant(x, wt, b, bias=torch.roll(b, -1)), r)


def test_checks_reject_an_omitted_last_k_chunk():
    x, wt, b = _small()
    r = _ref(x, wt, b)
    y = R.rne16(r.ref)
    m = torch.ones_like(x)
    m[:, 32:] = 0   # channels 32..39: the partial last K chunk
    yd = _mutant(x, wt, b, mask_x=m)
    y[..., 0:8, 0:32] = yd[..., 0:8, 0:32]   # omitted for one 8 x 32 tile
    assert not _passes(y, r)


def test_checks_reject_output_truncation():
    x, wt, b = _small()
    r = _ref(x, wt, b)
    assert not _passes(R.trunc16(r.ref), r)


def test_checks_reject_weight_truncation():
    x, wt, b = _small()
    r = _ref(x, wt, b)
    assert not _passes(_mutant(x, wt, b, w_hat=R.trunc16(wt.double())), r)


def test_stats_check_rejects_a_missing_pixel():
    x, wt, b = _small()
    y = R.rne16(_ref(x, wt, b).ref)
    st = R.tile_stats_ref(y, 8)
    got = st[..., :2].clone()
    # tile 0, channel 0 without its pixel (3, 5)
    v = float(y[0, 0, 3, 5])
    got[0, 0, 0] -= v
    got[0, 0, 1] -= v * v
    assert not R.stats_check(got.float(), st)[0]
