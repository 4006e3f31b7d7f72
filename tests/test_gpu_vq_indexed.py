"""elvis_vq_nearest_indexed (csrc/vq_index.hip) against the float32 first-minimum restatement `_normref.vq_ref` and, on
the same buffers, against the full scan elvis_vq_nearest: indices, zq bits, pad channels and guards - equality throughout.

The inputs are chosen where a grid search can go wrong and a scan cannot: duplicate codes (the lower index must win even
from another position of a cell's list), exact ties between different codes, every code in one cell, an outlier that
stretches the grid, pixels far outside the codebook's bounding box, pixels exactly on cell faces, signed zeros and
denormals.  c = 4 has no index: ops.vq_nearest falls back to the scan."""
import numpy as np
import pytest
import torch

import _normref as R
import _vq_grid_ref as V
from test_gpu_model_kernels_matrix import SENTINEL, _last_launch, _out_buffer, _pitched

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 5, 257, 8192)
PIXELS = (1, 3, 4, 5, 1025)


def _dt(dt):
    from elvis_amd._lib import F16, F32
    return (torch.float16, F16) if dt == "f16" else (torch.float32, F32)


def _index(cbd):
    from elvis_amd import ops
    index = ops.vq_index(cbd)
    assert index is not None and index.data_ptr() % 16 == 0
    return index


def _edges(index):
    """The grid's cells per axis and the three axes' edges [3, G + 1], as the kernel reads them (header of the index)."""
    words = index[:256].cpu().numpy().view(np.int32)
    g = int(words[0])
    return g, words[4:4 + 3 * 17].view(np.float32).reshape(3, 17)[:, :g + 1].copy()


def _check(cb, z, dt, dev, what, index=None, cbd=None, pin=16, pout=16, want_idx=True):
    """Both entries on the same buffers: the indexed one equals vq_ref and equals the scan.  `want_idx=False` gives the
    indexed entry a null index buffer, what ops.vq_nearest(want_idx=False) passes; its codes are then read off zq."""
    from elvis_amd._lib import lib, check, ptr, stream_handle
    dtype, code = _dt(dt)
    pixels, n_embed = z.shape[0], cb.shape[0]
    cbd = cb.contiguous().to(dev) if cbd is None else cbd
    index = _index(cbd) if index is None else index
    zd = _pitched(z, pin, dtype, dev)                          # NaN in the input's pad channels: never read
    ridx, rzq = R.vq_ref(z.to(dtype).float().numpy(), cb.numpy())
    got = {}
    for name in ("indexed", "scan"):
        out = _out_buffer(pixels, 3, pout, dtype, dev)
        idx = torch.full((pixels + 8,), -7, dtype=torch.int32, device=dev)
        if name == "indexed":
            check(lib().elvis_vq_nearest_indexed(ptr(zd), ptr(out), ptr(idx) if want_idx else 0, code, pixels, 3, pin, pout, ptr(cbd),
                                                 n_embed, ptr(index), stream_handle(dev)), dev)
            assert _last_launch() == f"vq_grid_nearest_kernel<{'half' if dt == 'f16' else 'float'}>"
        else:
            check(lib().elvis_vq_nearest(ptr(zd), ptr(out), ptr(idx), code, pixels, 3, pin, pout, ptr(cbd), n_embed,
                                         stream_handle(dev)), dev)
        torch.cuda.synchronize()
        o, i = out.cpu(), idx.cpu().numpy()
        assert bool((o[:pixels, 3:] == 0).all()), f"{what} / {name}: pad channels not zeroed"
        assert bool((o[pixels] == SENTINEL).all()) and (i[pixels:] == -7).all(), f"{what} / {name}: written past the end"
        got[name] = (i[:pixels], o[:pixels, :3].numpy())
    if not want_idx:
        assert (got["indexed"][0] == -7).all(), f"{what}: an index was written without an index buffer"
        got["indexed"] = (got["scan"][0], got["indexed"][1])               # zq below is compared on its own
    for name, (i, o) in got.items():
        bad = np.nonzero(i != ridx)[0]
        assert bad.size == 0, f"{what} / {name}: pixel {bad[0]} ({z[bad[0]].tolist()}) index {i[bad[0]]}, reference {ridx[bad[0]]}"
        assert R.bits_equal(o, R.np_store(rzq, dt == "f16")), f"{what} / {name}: zq differs from the stored codebook[idx]"
    assert np.array_equal(got["indexed"][0], got["scan"][0]) and R.bits_equal(got["indexed"][1], got["scan"][1])
    return ridx


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("n_embed", SIZES)
def test_random_codes_every_size(gpu_device, n_embed, dt):
    g = torch.Generator().manual_seed(9100 + n_embed)
    cb = torch.randn(n_embed, 3, generator=g).float()
    cbd = cb.contiguous().to(gpu_device)
    index = _index(cbd)
    for pixels in PIXELS:
        z = torch.randn(pixels, 3, generator=g) * 1.2
        _check(cb, z, dt, gpu_device, f"k{n_embed} p{pixels}", index, cbd)


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_duplicates_the_lower_index_wins(gpu_device, dt):
    """200 codes that exist twice, queried exactly (the construction of test_vq_rejects_last_minimum_and_fused_distance)."""
    g = torch.Generator().manual_seed(71)
    cb = torch.randn(1024, 3, generator=g).float()
    if dt == "f16":
        cb = cb.half().float()
    lo = torch.randint(0, 128, (200,), generator=g)
    cb[lo + 519] = cb[lo]
    ridx = _check(cb, cb[lo].clone(), dt, gpu_device, "duplicates")
    assert (ridx == lo.numpy()).all()
    # rotated by 519: the copy (now at lo) stands in front of the original (now at lo + 505) and wins
    cb2 = torch.cat([cb[519:], cb[:519]])
    ridx = _check(cb2, cb[lo].clone(), dt, gpu_device, "duplicates, copy first")
    assert (ridx == lo.numpy()).all()


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_exact_ties_between_mirrored_codes(gpu_device, dt):
    """Codes (a, b, t) and (b, a, t) are exactly equidistant from (0, 0, 0) - fl(a a + b b) is commutative - and from every
    pixel on the diagonal (s, s, u): the first of the pair must win, whatever cells the two fall into."""
    rng = np.random.default_rng(7)
    ab = rng.standard_normal((64, 3)).astype(np.float32)
    if dt == "f16":
        ab = ab.astype(np.float16).astype(np.float32)
    pairs = np.empty((128, 3), np.float32)
    pairs[0::2] = ab
    pairs[1::2] = ab[:, [1, 0, 2]]
    cb = torch.from_numpy(pairs)
    z = torch.zeros(1, 3)
    ridx = _check(cb, z, dt, gpu_device, "mirrored pairs at 0")
    assert ridx[0] % 2 == 0
    s = torch.from_numpy(rng.standard_normal((300, 2)).astype(np.float32))
    ridx = _check(cb, torch.stack([s[:, 0], s[:, 0], s[:, 1]], 1), dt, gpu_device, "mirrored pairs on the diagonal")
    assert (ridx % 2 == 0).all()
    # the mirrored code first: now the odd positions hold the originals, and the even ones still win
    ridx = _check(torch.from_numpy(pairs[::-1].copy()), z, dt, gpu_device, "mirrored pairs reversed")
    assert ridx[0] % 2 == 0


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_all_codes_in_one_cell_and_an_outlier(gpu_device, dt):
    g = torch.Generator().manual_seed(9200)
    # a cluster of 2046 codes 1e-3 wide and two corner codes that span the grid: one cell holds the cluster
    cluster = 0.3 + torch.randn(2046, 3, generator=g) * 1e-3
    cb = torch.cat([torch.tensor([[-4.0, -4.0, -4.0]]), cluster, torch.tensor([[4.0, 4.0, 4.0]])]).float()
    z = torch.cat([0.3 + torch.randn(500, 3, generator=g) * 2e-3, torch.randn(500, 3, generator=g) * 3])
    _check(cb, z, dt, gpu_device, "one cell")
    index = _index(cb.to(gpu_device))
    gsize, edges = _edges(index)
    cells = [np.searchsorted(edges[d][1:gsize], cluster[:, d].numpy(), side="right") for d in range(3)]
    assert gsize > 4 and all(len(set(c.tolist())) == 1 for c in cells), "the cluster was meant to sit in one cell"
    # one code 1e4 away from the rest: every other code falls into the first cells of every axis
    cb = torch.randn(8192, 3, generator=g).float()
    cb[4321] = torch.tensor([1.0e4, -1.0e4, 1.0e4])
    z = torch.cat([torch.randn(600, 3, generator=g) * 1.5, torch.tensor([[9.0e3, -9.0e3, 9.0e3], [5.0e3, -5.0e3, 5.0e3], [5.0e3, 0.0, 0.0]])])
    ridx = _check(cb, z, dt, gpu_device, "outlier")
    assert ridx[600] == 4321


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_pixels_far_outside_the_bounding_box(gpu_device, dt):
    g = torch.Generator().manual_seed(9300)
    cb = torch.randn(8192, 3, generator=g).float()
    far = torch.randn(700, 3, generator=g) * (1.0e3 if dt == "f16" else 1.0e6)
    one_axis = torch.randn(325, 3, generator=g)
    one_axis[:, 1] = 3.0e4 if dt == "f16" else -7.0e8             # outside on one axis only, inside on the others
    _check(cb, torch.cat([far, one_axis]), dt, gpu_device, "far outside")


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_pixels_exactly_on_cell_faces(gpu_device, dt):
    """Codes in [-2, 2]^3 with both corners present: 16 cells of width 0.25 per axis, edges exact in f16 and f32.  Pixels
    on faces, edges and corners of cells, the outer faces of the grid included."""
    g = torch.Generator().manual_seed(9400)
    cb = (torch.rand(8192, 3, generator=g) * 4 - 2).float()
    cb[0] = torch.tensor([-2.0, -2.0, -2.0])
    cb[8191] = torch.tensor([2.0, 2.0, 2.0])
    cb[100:400] = torch.round(cb[100:400] * 4) / 4                 # codes on faces too
    cbd = cb.contiguous().to(gpu_device)
    index = _index(cbd)
    gsize, edges = _edges(index)
    assert gsize == 16 and np.array_equal(edges, np.tile(np.arange(17, dtype=np.float32) * 0.25 - 2, (3, 1)))
    e = torch.from_numpy(edges[0])
    pick = lambda n: e[torch.randint(0, 17, (n,), generator=g)]
    inside = lambda n: torch.rand(n, generator=g) * 4 - 2
    z = torch.cat([torch.stack([pick(300), inside(300), inside(300)], 1), torch.stack([inside(300), pick(300), pick(300)], 1),
                   torch.stack([pick(425), pick(425), pick(425)], 1)])
    _check(cb, z, dt, gpu_device, "on faces", index, cbd)


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_signed_zeros_and_denormals(gpu_device, dt):
    g = torch.Generator().manual_seed(9500)
    tiny = 6.0e-8 if dt == "f16" else 1.0e-40                      # a denormal of the pixel's format
    cb = torch.randn(257, 3, generator=g).float() * 0.5
    cb[3] = torch.tensor([0.0, -0.0, 0.0])
    cb[9] = torch.tensor([-0.0, 0.0, -0.0])
    cb[20] = torch.tensor([1.0e-40, -1.0e-40, 3.0e-39])
    cb[21] = torch.tensor([-2.0e-41, 1.0e-45, 0.0])
    vals = torch.tensor([0.0, -0.0, tiny, -tiny, 2 * tiny, 1.0e-3])
    z = vals[torch.randint(0, len(vals), (400, 3), generator=g)]
    ridx = _check(cb, z, dt, gpu_device, "zeros and denormals")
    assert 3 in ridx                                               # (+-0, +-0, +-0) ties codes 3 and 9 at distance 0: 3 wins
    assert 9 not in ridx


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("case_id", [c.id for c in V.CASES])
def test_the_cases_of_the_host_model(gpu_device, case_id, dt):
    """tests/_vq_grid_ref.py: grids of one and two cells, the grid capped at 16, codebooks constant on one, two and three
    axes with pixels below, on and above the value, pixel counts around a workgroup, the mutants' cases - among them ties
    whose winner is visited after its rival (tests/test_vq_grid_host.py shows what each case contains)."""
    cb, z = V.BY_ID[case_id].arrays()
    assert cb.shape[0] <= V.MAX_CODES and z.shape[0] <= V.MAX_PIXELS
    ridx = _check(torch.from_numpy(cb.copy()), torch.from_numpy(z.copy()), dt, gpu_device, case_id)
    if case_id == "mirrored_winner_seen_later":
        assert (ridx % 2 == 0).all()


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("pin,pout", [(3, 3), (3, 16), (16, 3)])
def test_tight_pitches(gpu_device, pin, pout, dt):
    """Pitch 3 in: nothing pads z[px * 3 + d].  Pitch 3 out: the zero-fill loop runs no iteration, and the guard row behind
    the last pixel shows that nothing is written past it."""
    for case_id in ("p255", "p257", "k7_two_cells", "constant_yz"):
        cb, z = V.BY_ID[case_id].arrays()
        _check(torch.from_numpy(cb.copy()), torch.from_numpy(z.copy()), dt, gpu_device, f"{case_id} pitch {pin}/{pout}", pin=pin, pout=pout)


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("pin,pout", [(16, 16), (3, 3)])
def test_without_an_index_buffer(gpu_device, pin, pout, dt):
    for case_id in ("p256", "p257", "random_2000"):
        cb, z = V.BY_ID[case_id].arrays()
        _check(torch.from_numpy(cb.copy()), torch.from_numpy(z.copy()), dt, gpu_device, f"{case_id} no idx", pin=pin, pout=pout,
               want_idx=False)
    # and through the wrapper that passes the null pointer
    from elvis_amd import ops
    cb, z = V.BY_ID["p257"].arrays()
    dtype, _ = _dt(dt)
    cbd = torch.from_numpy(cb.copy()).to(gpu_device)
    zt = torch.from_numpy(z.copy()).reshape(1, 1, 257, 3)
    out = ops.vq_nearest(ops.Act(_pitched(zt, 8, dtype, gpu_device), 3), cbd, want_idx=False, index=_index(cbd))
    assert _last_launch() == f"vq_grid_nearest_kernel<{'half' if dt == 'f16' else 'float'}>"
    ridx, rzq = R.vq_ref(z, cb)
    assert R.bits_equal(out.t.cpu().numpy().reshape(-1, out.pitch)[:, :3], R.np_store(rzq, dt == "f16"))


def test_four_channels_fall_back_to_the_scan(gpu_device):
    from elvis_amd import ops
    from elvis_amd._lib import lib
    assert lib().elvis_vq_index_bytes(8192, 4) == 0 and lib().elvis_vq_index_bytes(8192, 3) > 0
    g = torch.Generator().manual_seed(9600)
    cb = torch.randn(300, 4, generator=g).float()
    cbd = cb.to(gpu_device)
    index = ops.vq_index(cbd)
    assert index is None
    z = torch.randn(1, 5, 7, 4, generator=g)
    zd = ops.Act(_pitched(z, 8, torch.float32, gpu_device), 4)
    out, idx = ops.vq_nearest(zd, cbd, want_idx=True, index=index)
    assert _last_launch() == "vq_nearest_kernel<float>"
    ridx, rzq = R.vq_ref(z.reshape(-1, 4).numpy(), cb.numpy())
    assert np.array_equal(idx.cpu().numpy().reshape(-1), ridx)
    assert R.bits_equal(out.t.cpu().numpy().reshape(-1, 8)[:, :4], rzq) and bool((out.t[..., 4:] == 0).all())
    # and three channels through the same wrapper take the grid
    cb3 = cb[:, :3].contiguous()
    out3, idx3 = ops.vq_nearest(ops.Act(_pitched(z[..., :3], 8, torch.float32, gpu_device), 3), cb3.to(gpu_device),
                                want_idx=True, index=ops.vq_index(cb3.to(gpu_device)))
    assert _last_launch() == "vq_grid_nearest_kernel<float>"
    assert np.array_equal(idx3.cpu().numpy().reshape(-1), R.vq_ref(z[..., :3].reshape(-1, 3).numpy(), cb3.numpy())[0])
