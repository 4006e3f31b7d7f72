"""elvis_gn_partials_affine (csrc/gn_fused.hip) against the two launches it replaces, elvis_gn_partials_to_sums followed
by elvis_groupnorm_affine: the bits of pa and pb are equal.  The tile counts sit on both sides of the 256 virtual lanes.

The first matrix keeps its inputs: a large mean and mixed signs.  Such fp32 values add exactly in float64 in any order
(tests/test_gn_fused_host.py shows it), so that matrix pins the arithmetic and the addressing, not the order of the sums.
The second matrix has an oracle of its own, the bit-exact numpy model tests/_gn_fused_model.py, inputs on which every
reordering of a sum moves pa and pb (the model's mutants), the spans, short last workgroups and tile counts the first one
never ran, and a variance that rounds below zero."""
import numpy as np
import pytest
import torch

import _gn_fused_model as M
from test_gpu_model_kernels_matrix import SENTINEL, _last_launch

pytestmark = pytest.mark.gpu

GROUPS, EPS = 32, 1e-6
_made = {}


def _partials(n, tiles, c):
    """[n * tiles, c, 2] per-tile (sum, sum of squares) of 256-pixel tiles: sums of either sign around +20 +- 50, squares
    consistent with them (a positive variance, so that nothing is hidden behind the clamp at 0)."""
    key = (n, tiles, c)
    if key not in _made:
        g = torch.Generator().manual_seed(1000 * tiles + 10 * c + n)
        s = torch.randn(n * tiles, c, generator=g) * 50.0 + 20.0
        ss = s * s / 256.0 + torch.randn(n * tiles, c, generator=g).abs() * 100.0 + 50.0
        _made[key] = torch.stack([s, ss], -1).float().contiguous()
    return _made[key]


def _params(c, on):
    g = torch.Generator().manual_seed(77 + c)
    gam, bet = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    sc, sh = torch.randn(c, generator=g) * 0.3, torch.randn(c, generator=g) * 0.3
    return gam, bet, (sc if on else None), (sh if on else None)


def _guarded(numel, dev):
    t = torch.full((numel + 8,), SENTINEL, dtype=torch.float32)
    t[:numel] = float("nan")
    return t.to(dev)


def _both(p, n, tiles, c, gam, bet, sc, sh, dev, groups=GROUPS):
    from elvis_amd._lib import lib, check, ptr, stream_handle
    d = lambda t: None if t is None else t.to(dev)
    pd, keep = p.to(dev), [d(gam), d(bet), d(sc), d(sh)]
    hw = tiles * 256
    s = stream_handle(dev)
    sums = torch.full((n, c, 2), float("nan"), dtype=torch.float64, device=dev)
    pa0, pb0, pa1, pb1 = (_guarded(n * c, dev) for _ in range(4))
    check(lib().elvis_gn_partials_to_sums(ptr(pd), tiles, n, c, ptr(sums), c, 0, s), dev)
    check(lib().elvis_groupnorm_affine(ptr(sums), *(ptr(t) for t in keep), ptr(pa0), ptr(pb0), n, hw, c, groups, EPS, s), dev)
    check(lib().elvis_gn_partials_affine(ptr(pd), tiles, *(ptr(t) for t in keep), ptr(pa1), ptr(pb1), n, hw, c, groups, EPS, s), dev)
    name = _last_launch()
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in (pa0, pb0, pa1, pb1)]
    for t in out:
        assert (t[n * c:] == SENTINEL).all() and not np.isnan(t[:n * c]).any()
    return name, [t[:n * c].view(np.int32) for t in out]


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "scale_shift"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("c", [32, 128, 160])
@pytest.mark.parametrize("tiles", [1, 255, 256, 257, 1000])
def test_one_launch_equals_the_two_it_replaces(gpu_device, tiles, c, n, affine):
    from elvis_amd._lib import lib
    gam, bet, sc, sh = _params(c, affine)
    name, (pa0, pb0, pa1, pb1) = _both(_partials(n, tiles, c), n, tiles, c, gam, bet, sc, sh, gpu_device)
    span = lib().elvis_gn_partials_affine_span(c, GROUPS)
    assert span == {32: 16, 128: 16, 160: 20}[c] and name == f"gn_partials_affine_kernel<{8 if span == 16 else 4}>"
    assert np.array_equal(pa0, pa1), f"pa: {int((pa0 != pa1).sum())} of {pa0.size} differ"
    assert np.array_equal(pb0, pb1), f"pb: {int((pb0 != pb1).sum())} of {pb0.size} differ"
    assert len(set(pa0.tolist())) > c // 2                     # the inputs were not degenerate


def _first_difference(name, got, want):
    bad = np.nonzero(got != want)[0]
    return f"{name}: {bad.size} of {got.size} differ, first at (image, channel) {divmod(int(bad[0]), got.size // M.N_IMAGES)}: " \
           f"{got[bad[0]]:#x} against {want[bad[0]]:#x}" if bad.size else ""


def _model_and_both(p, c, groups, tiles, affine, dev):
    """(kernel name, pa, pb of the two launches, of the one launch, of the model) as int32 words, for partials [n, tiles, c, 2]."""
    n = p.shape[0]
    gam, bet, sc, sh = M.params(c, affine)
    t = lambda a: None if a is None else torch.from_numpy(a)
    name, (pa0, pb0, pa1, pb1) = _both(torch.from_numpy(np.array(p)).reshape(n * tiles, c, 2), n, tiles, c, t(gam), t(bet), t(sc), t(sh),
                                       dev, groups)
    ma, mb = M.model(p, gam, bet, sc, sh, tiles * 256, groups, EPS)
    return name, (pa0, pb0), (pa1, pb1), (ma.reshape(-1).view(np.int32), mb.reshape(-1).view(np.int32))


@pytest.mark.parametrize("c,groups,tiles", M.gpu_cases(), ids=lambda v: str(v))
def test_new_spans_equal_the_model_and_the_two_launches(gpu_device, c, groups, tiles):
    from elvis_amd._lib import lib
    assert EPS == M.EPS and lib().elvis_gn_partials_affine_span(c, groups) == M.SHAPES[(c, groups)] == M.span_of(c, groups)
    p = M.partials(M.N_IMAGES, tiles, c, c // groups)
    name, two, one, model = _model_and_both(p, c, groups, tiles, (c + tiles) % 2 == 0, gpu_device)
    assert name == f"gn_partials_affine_kernel<{M.row_lanes(c, groups)}>"
    for what, got, want in (("pa", one[0], model[0]), ("pb", one[1], model[1])):
        assert np.array_equal(got, want), _first_difference(f"{what} against the model", got, want)
    for what, got, want in (("pa", one[0], two[0]), ("pb", one[1], two[1])):
        assert np.array_equal(got, want), _first_difference(f"{what} against the two launches", got, want)


@pytest.mark.parametrize("c,groups,tiles", M.CLAMP_CASES)
def test_a_variance_that_rounds_below_zero_is_clamped_the_same_way(gpu_device, c, groups, tiles):
    """Every tile of a channel holds (256 v, 256 fl32(v^2)) with fl32(v^2) < v^2: the variance is negative before the clamp
    (the host test asserts it on the model).  Both device paths and the model agree bit for bit."""
    p = M.clamp_partials(M.N_IMAGES, tiles, c, groups)
    info = {}
    gam, bet, sc, sh = M.params(c, True)
    M.model(p, gam, bet, sc, sh, tiles * 256, groups, EPS, info=info)
    assert (info["var"] < 0).all()
    name, two, one, model = _model_and_both(p, c, groups, tiles, True, gpu_device)
    for k, what in enumerate(("pa", "pb")):
        assert np.array_equal(one[k], model[k]), _first_difference(f"{what} against the model", one[k], model[k])
        assert np.array_equal(one[k], two[k]), _first_difference(f"{what} against the two launches", one[k], two[k])


def test_null_gamma_and_shift_without_scale(gpu_device):
    n, tiles, c = 2, 300, 128
    _, _, _, sh = _params(c, True)
    for args in ((None, None, None, None), (None, None, None, sh)):
        _, (pa0, pb0, pa1, pb1) = _both(_partials(n, tiles, c), n, tiles, c, *args, gpu_device)
        assert np.array_equal(pa0, pa1) and np.array_equal(pb0, pb1)


def test_groupnorm_affine_takes_the_one_launch_for_one_buffer(gpu_device):
    """ops.groupnorm_affine: one input with fused partials -> the new entry; a concat, or an input without partials, or a
    group wider than the kernel's span -> the old ones.  Same (pa, pb) either way."""
    from elvis_amd import ops
    from elvis_amd._lib import lib
    dev = gpu_device
    n, h, w, c = 2, 16, 64, 128
    tiles = 4
    g = torch.Generator().manual_seed(5)
    x = ops.Act(torch.randn(n, h, w, c, generator=g).half().to(dev), c, _partials(n, tiles, c).to(dev))
    gam, bet, _, _ = _params(c, False)
    gam, bet = gam.to(dev), bet.to(dev)
    pa, pb = ops.groupnorm_affine([x], gam, bet, GROUPS, EPS)
    assert _last_launch() == "gn_partials_affine_kernel<8>"
    sums = torch.zeros((n, c, 2), dtype=torch.float64, device=dev)
    pa0, pb0 = torch.zeros_like(pa), torch.zeros_like(pb)
    from elvis_amd._lib import check, ptr, stream_handle
    check(lib().elvis_gn_partials_to_sums(ptr(x.stats), tiles, n, c, ptr(sums), c, 0, stream_handle(dev)), dev)
    check(lib().elvis_groupnorm_affine(ptr(sums), ptr(gam), ptr(bet), 0, 0, ptr(pa0), ptr(pb0), n, h * w, c, GROUPS, EPS,
                                       stream_handle(dev)), dev)
    assert torch.equal(pa.view(torch.int32), pa0.view(torch.int32)) and torch.equal(pb.view(torch.int32), pb0.view(torch.int32))
    plain = ops.Act(x.t, c)
    ops.groupnorm_affine([plain], gam, bet, GROUPS, EPS)
    assert _last_launch() == "gn_affine_kernel"
    ops.groupnorm_affine([x, x], torch.cat([gam, gam]), torch.cat([bet, bet]), GROUPS, EPS)
    assert _last_launch() == "gn_affine_kernel"
    assert lib().elvis_gn_partials_affine_span(2112, GROUPS) == 0 and lib().elvis_gn_partials_affine_span(1024, GROUPS) == 32
    with pytest.raises(ValueError):
        check(lib().elvis_gn_partials_affine(ptr(x.stats), tiles, 0, 0, 0, 0, ptr(pa), ptr(pb), n, h * w, c, 1, EPS,
                                             stream_handle(dev)), dev)
