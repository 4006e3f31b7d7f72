"""CPU-side checks of the glue matrix (tests/_glueref.py, tests/test_gpu_glue_matrix.py): the ledger (the kernels of
csrc/glue.hip in the built library are exactly the ones the cases name), the branches the case list must reach, the
pins of the references against oracle.glue_ref and the goldens, the honesty conditions of the SSIM bound, and the
discrimination test: every mutant of a reference differs from the true one somewhere on the matrix - otherwise the
inputs could not tell a wrong kernel from a right one."""
import functools
import os

import numpy as np
import pytest

import _glueref as R
from oracle import glue_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLUE_HIP = os.path.join(ROOT, "elvis_amd", "csrc", "glue.hip")
SMALL = [c for c in R.CASES if not c.big]


def _of(op, cases=R.CASES):
    return [c for c in cases if c.op == op]


# ------------------------------------------------------------------------------------------------------- ledger
def test_demangle():
    stems = R.glue_kernel_stems(GLUE_HIP)
    assert len(stems) == 11 and "recompose_u8_kernel" in stems and "clamp_map_kernel" in stems
    assert R.demangle_glue("_Z19recompose_u8_kernelILb1EEvPKhS1_PKiPhiiiiiiiiix", stems) == "recompose_u8_kernel<true>"
    assert R.demangle_glue("_Z19recompose_u8_kernelILb0EEvPKhS1_PKiPhiiiiiiiiix", stems) == "recompose_u8_kernel<false>"
    assert R.demangle_glue("_Z15blend_u8_kernelPKhS0_PKiPhiiiiiiifx", stems) == "blend_u8_kernel"
    assert R.demangle_glue("_Z30__device_stub__blend_u8_kernelPKhS0_PKiPhiiiiiiifx", stems) is None
    assert R.demangle_glue("elvis_blend_u8", stems) is None


def test_kernel_ledger(built_lib):
    """The glue.hip kernels of the built library == the names the cases resolve to (+ clamp_map_kernel, which every
    recompose case with a map_out runs and checks)."""
    syms = R.glue_kernel_symbols(built_lib, GLUE_HIP)
    named = {c.expect for c in R.CASES} | R.ALSO_RUN
    assert not syms - named, f"kernels without a matrix case: {sorted(syms - named)}"
    assert not named - syms, f"cases naming kernels the library does not build: {sorted(named - syms)}"
    assert len(syms) == 12
    assert len({c.id for c in R.CASES}) == len(R.CASES)
    assert any(c.clamp_to is not None for c in _of("recompose")) and any(c.clamp_to is None for c in _of("recompose"))
    assert {c.op for c in R.CASES} == set(R.OPS)


def test_the_cases_cover_the_branches():
    total = lambda c: int(np.prod(c.shape))
    rec = _of("recompose")
    assert {c.expect for c in rec} == {"recompose_rows_u8_kernel", "recompose_u8_kernel<true>", "recompose_u8_kernel<false>"}
    for c in rec:       # the dispatch restated from the launch code
        n, h, w, ch = c.shape
        rows = (w * ch) % 16 == 0 and c.block * ch >= 16
        assert (c.expect == "recompose_rows_u8_kernel") == rows
        assert rows or (c.expect == "recompose_u8_kernel<true>") == (c.block in (1, 2, 4, 8, 16, 32, 64))
    rows = [c for c in rec if c.expect == "recompose_rows_u8_kernel"]
    assert {16, 18, 24} <= {c.block * c.shape[3] for c in rows}
    assert any(c.shape[2] % c.block and c.shape[1] % c.block for c in rows), "trailing pixels and rows on the rows path"
    small_map = [c for c in rec if c.grid and c.grid[0] < c.shape[1] // c.block and c.grid[1] < c.shape[2] // c.block]
    assert {c.expect for c in small_map} >= {"recompose_rows_u8_kernel", "recompose_u8_kernel<false>"}
    assert {c.kind for c in rec} == {"some", "all", "none"}
    for op in ("recompose", "blend", "select"):
        assert any(total(c) % 16 for c in _of(op)), f"{op}: no total that is not a multiple of 16"
    assert {c.expect for c in rec if total(c) % 16} == {"recompose_u8_kernel<true>", "recompose_u8_kernel<false>"}
    # one case above every grid cap (R.CAP_*: the launch code's grid limit times what a lane handles)
    assert {c.expect for c in rec if total(c) > R.CAP_RECOMPOSE_BYTES} == {c.expect for c in rec}
    assert any(total(c) > R.CAP_BLEND_BYTES for c in _of("blend")) and any(total(c) > R.CAP_BLEND_BYTES for c in _of("select"))
    outs = lambda c: total(c) // (c.factor * c.factor)
    area = _of("area")
    assert any(outs(c) > R.CAP_AREA_OUTPUTS for c in area if c.expect == "area_downscale_u8_kernel")
    assert any(outs(c) // 3 > R.CAP_AREA_OUTPUTS for c in area if c.expect == "area_downscale4_c3_kernel")
    assert any(c.shape[1] * c.shape[2] > R.CAP_NORMALIZE_PIXELS for c in _of("normalize"))
    assert all(c.big == (total(c) > 2 ** 20) for c in R.CASES if c.kind != "extreme"), "only the over-cap cases are large"
    # area: channels x factors x roundings x batch, the four byte offsets of the c3 / f4 image
    assert {(c.shape[3], c.factor, c.rounding, c.shape[0]) for c in area if c.kind == "random" and not c.big} == \
        {(ch, f, r, n) for ch in (1, 2, 3, 4) for f in (1, 2, 3, 4, 5, 7, 8, 16) for r in (0, 1) for n in (1, 3)}
    offs = [c for c in area if c.shape[3] == 3 and c.factor == 4 and c.kind == "every_sum"]
    assert {c.offset for c in offs} == {0, 1, 2, 3}
    assert all((c.expect == "area_downscale4_c3_kernel") == (c.offset == 0) for c in offs)
    assert {(c.factor, c.expect) for c in area if c.kind == "every_sum"} == {
        (2, "area_downscale_u8_kernel"), (3, "area_downscale_u8_kernel"), (4, "area_downscale_u8_kernel"),
        (4, "area_downscale4_c3_kernel")}
    # blend: every alpha on the pair image and on frames the block does not divide
    for kind in ("pairs", "random"):
        assert {np.float32(c.alpha) for c in _of("blend") if c.kind == kind and not c.big} == {np.float32(a) for a in R.ALPHAS}
    assert any(c.shape[1] % c.block and c.shape[2] % c.block for c in _of("blend"))
    sel = _of("select")
    assert {c.versions for c in sel} == {1, 2, 3, 4} and {c.shape[3] for c in sel} == {1, 3} and {c.block for c in sel} == {3, 8}
    assert any(-1 in c.slots for c in sel) and any(c.offset == 1 for c in sel)
    assert any(c.shape[1] % c.block and c.shape[2] % c.block for c in sel)
    acc = _of("accumulate")
    assert {c.shape[3] for c in acc} == {1, 3} and {t[4] for c in acc for t in c.tiles} == {1.0, 0.5, 0.3}
    assert any(len(c.tiles) == 2 for c in acc) and any((t[2] * t[3]) % 256 for c in acc for t in c.tiles)
    assert {c.shape[3] for c in _of("normalize")} == {1, 3, 4}
    sse = _of("sse")
    assert {int(np.prod(c.shape[1:])) for c in sse} >= {1, 63, 64, 65, 4095, 4096, 4097, 8197}
    assert {c.shape[3] for c in sse if c.mask == "random"} == {1, 3, 4} and {c.mask for c in sse} == {"", "zero", "full", "random"}
    assert {c.shape[0] for c in sse} == {1, 3}
    ssim = _of("ssim")
    assert {c.block for c in ssim} == set(R.SSIM_BLOCKS) >= {10, 11}
    assert {(c.block, c.shape[3], c.kind) for c in ssim} == {(b, ch, k) for b in R.SSIM_BLOCKS for ch in (1, 3) for k in R.SSIM_CONTENT}
    assert all(c.shape[1] % c.block and c.shape[2] % c.block for c in ssim if c.block > 1)


# ------------------------------------------------------------------------------------------------------- pins
def test_recompose_ref_equals_the_oracle():
    for c in _of("recompose"):
        a, b, m = R.inputs(c)
        ref, = R.expected(c)[:1]
        for i in range(a.shape[0]):
            assert np.array_equal(ref[i], glue_ref.recompose_select(a[i], b[i], m[i].astype(np.int64) <= c.thr, c.block)), c.id
        if c.clamp_to is not None:
            assert np.array_equal(R.expected(c)[1], np.where(m <= c.thr, m, c.clamp_to)), c.id


def test_area_ref_equals_the_oracle():
    for c in _of("area"):
        x, = R.inputs(c)
        ref, = R.expected(c)
        for i in range(x.shape[0]):
            assert np.array_equal(ref[i], glue_ref.area_downscale_u8(x[i], c.factor, "cv2" if c.rounding == 0 else "half_up")), c.id
    x = np.random.default_rng(1).integers(0, 256, (1, 32, 48, 3), dtype=np.uint8)
    for r in (0, 1):
        assert np.array_equal(R.area_ref_u16(x, 4, r), R.area_ref(x, 4, r))


def test_every_sum_image_is_complete():
    """Every block sum 0 .. 255 f^2 occurs, in every channel: every tie and every saturation point of the division."""
    for f in (2, 3, 4):
        for ch in (1, 3):
            img = R.every_sum_image(f, ch, f)
            assert img.shape == R.every_sum_shape(f, ch)
            s = img.reshape(1, img.shape[1] // f, f, img.shape[2] // f, f, ch).astype(np.int64).sum((2, 4))
            for k in range(ch):
                assert set(s[..., k].ravel().tolist()) == set(range(255 * f * f + 1)), (f, ch, k)


def test_blend_ref_equals_the_oracle():
    for c in _of("blend"):
        o, r, m = R.inputs(c)
        ref, = R.expected(c)
        for i in range(o.shape[0]):
            assert np.array_equal(ref[i], glue_ref.blend_by_map(o[i], r[i], m[i], c.block, c.alpha)), c.id


def test_select_ref_equals_the_oracle_pick():
    """restore_video_adaptively's pick applies where every level of the map has a version and frames have 3 channels:
    the cases' inputs with the map folded into the valid levels."""
    done = 0
    for c in _of("select", SMALL):
        *vs, m = R.inputs(c)
        if c.shape[3] != 3:
            continue
        valid = [lv for lv, s in enumerate(c.slots) if s >= 0]
        mv = np.asarray(valid)[np.mod(m, len(valid))].astype(np.int32)
        ref = R.select_ref(vs, np.asarray(c.slots, np.int32), mv, c.block)
        fn = lambda frames, degradation_level=0, **kw: [f for f in vs[c.slots[int(degradation_level)]]]
        got = glue_ref.restore_video_adaptively(fn, [f for f in vs[0]], [d for d in mv], block_size=c.block)
        assert np.array_equal(ref, np.stack(got)), c.id
        done += 1
    assert done >= 3


def test_sse_ref_equals_the_oracle_mse():
    for c in _of("sse"):
        a, b, mk = R.inputs(c)
        sse, cnt = R.expected(c)
        for i in range(a.shape[0]):
            want = glue_ref.masked_mse(a[i], b[i], None if mk is None else np.broadcast_to(mk[i][..., None], a[i].shape))
            got = 0.0 if cnt[i] == 0 else float(sse[i]) / float(cnt[i])
            # the oracle averages float32 squares in float32: good to 2e-6 on these small frames, 2e-5 on the 1080p one
            assert got == pytest.approx(want, rel=2e-5 if c.kind == "extreme" else 2e-6), c.id
    big = [c for c in _of("sse") if c.kind == "extreme"][0]
    assert R.expected(big)[0].tolist() == [404_507_520_000] and R.expected(big)[0][0] > 2 ** 32


def test_accumulate_and_normalize_refs_reproduce_the_tiler_goldens(golden_dir):
    """The reference's own resource_aware_restore outputs (tests/golden/tiler.npz), bit for bit, from the product's host
    logic (windows, ramps, temporal weights) with the accumulate / normalise references in place of the kernels."""
    from elvis_amd.tiler import _edge_ramp, _temporal_weight, _windows
    g = np.load(os.path.join(golden_dir, "tiler.npz"))
    fns = {"ident": lambda f, tc: f.copy(),
           "affine": lambda f, tc: np.clip(f.astype(np.float32) * 0.5 + 7.0, 0, 255).astype(np.uint8),
           "coord": lambda f, tc: np.clip(f.astype(np.int32) + (tc[2] * 3 + tc[4] * 5 + tc[0] * 11) % 37, 0, 255).astype(np.uint8)}
    ran = 0
    for k in range(int(g["count"])):
        n, h, w, tile, halo, chunk, ov = [int(v) for v in g[f"c{k}_cfg"]]
        if int(g[f"c{k}_raised"]):
            continue
        frames, fn = g[f"c{k}_in"], fns[str(g[f"c{k}_fn"])]
        tiled, chunked = tile > 0 and (h > tile or w > tile), chunk > 0 and n > chunk
        if not (tiled or chunked):        # the restorer is called once, directly: nothing is accumulated
            continue
        side = tile if tiled else max(h, w)
        rows = _windows(h, side, tile - halo) if tiled else [(0, h)]
        cols = _windows(w, side, tile - halo) if tiled else [(0, w)]
        spans = _windows(n, chunk, chunk - ov) if chunked else [(0, n)]
        acc, wsum = np.zeros((n, h, w, 3), np.float32), np.zeros((n, h, w), np.float32)
        fe = halo // 2 if tiled else 0
        for (t0, t1) in spans:
            for (y0, y1) in rows:
                for (x0, x1) in cols:
                    wy = _edge_ramp(y1 - y0, fe, y0 > 0, y1 < h, np.float32)
                    wl = _edge_ramp(x1 - x0, fe, x0 > 0, False, np.float64)
                    wr = _edge_ramp(x1 - x0, fe, False, x1 < w, np.float64)
                    for i in range(t1 - t0):
                        out = fn(frames[t0 + i][y0:y1, x0:x1], (t0, t1, y0, y1, x0, x1))
                        tw = _temporal_weight(i, t1 - t0, ov, t0 > 0, t1 < n) if chunked else 1.0
                        R.tile_accumulate_ref(acc[t0 + i], wsum[t0 + i], out, wy, wl, wr, y0, x0, float(np.float32(tw)))
        final = np.stack([R.tile_normalize_ref(acc[i], wsum[i]) for i in range(n)])
        assert np.array_equal(final, g[f"c{k}_out"]), f"golden case {k}"
        ran += 1
    assert ran >= 12


def test_normalize_edge_inputs_sit_on_the_integer_boundaries():
    for ch in (1, 3, 4):
        acc, wsum = R.normalize_edges(ch)
        out = R.tile_normalize_ref(acc, wsum)
        for r, ws in enumerate(R.NORMALIZE_WSUM):
            k = (np.arange(256)[:, None] + 85 * np.arange(ch)[None, :]) % 256
            exact, below, half, neg, beyond = (out[5 * r + j] for j in range(5))
            if ws != 1e-30:
                assert np.array_equal(exact, k) and np.array_equal(below, np.maximum(k - 1, 0)), ws
            assert np.array_equal(half, k) and not neg.any() and (beyond == 255).all(), ws
        assert not np.isnan(acc).any() and not np.isnan(wsum).any()


# ------------------------------------------------------------------------------------------------------- SSIM
@functools.lru_cache(maxsize=None)
def _ssim_all():
    out = {}
    for c in _of("ssim"):
        a, b = R.inputs(c)
        ref, bound = R.ssim_ref(a, b, c.block)
        out[c.id] = (ref, bound, R.ssim_f32_restatement(a, b, c.block).astype(np.float64))
    return out


def test_ssim_window_and_ref_equal_the_product_window_and_the_oracle():
    from elvis_amd.metrics import ssim_window
    assert R.ssim_window().dtype == np.float32 and np.array_equal(R.ssim_window(), ssim_window())
    for c in _of("ssim"):
        a, b = R.inputs(c)
        ref = _ssim_all()[c.id][0]
        o = np.stack([glue_ref.block_ssim(a[i], b[i], c.block) for i in range(a.shape[0])])
        assert np.abs(o - ref).max() <= 1.2e-7, c.id          # the oracle returns float32: half an ulp of 1, doubled
        if c.kind == "black":
            assert (ref == 1.0).all()
        if c.kind == "inverse" and c.block >= 11:
            assert ref.min() < 0
        if c.block < 11:                                       # unsmoothed: the structure term is identically 1
            x, y = a.astype(np.float64) / 255, b.astype(np.float64) / 255
            lum = (2 * x * y + 1e-4) / (x * x + y * y + 1e-4)
            by, bx = a.shape[1] // c.block, a.shape[2] // c.block
            want = lum[:, :by * c.block, :bx * c.block].reshape(a.shape[0], by, c.block, bx, c.block, -1).mean((2, 4, 5))
            assert np.abs(want - ref).max() < 1e-13, c.id


def test_ssim_bound_is_honest():
    """The float32 restatement of the kernel's order stays inside the bound on every case, is not far inside on all of
    them, and the bound of the noise cases stays below the tolerance the earlier test used."""
    worst = {}
    for c in _of("ssim"):
        ref, bound, y = _ssim_all()[c.id]
        ratio = float((np.abs(y - ref) / bound).max())
        assert ratio <= 1.0, f"{c.id}: the restatement leaves the bound (ratio {ratio:.3f})"
        worst[c.kind] = max(worst.get(c.kind, 0.0), ratio)
        if c.kind == "noise":
            assert float(bound.max()) < 2e-5, f"{c.id}: bound {float(bound.max()):.3g}"
        if c.kind == "black":
            assert (y == 1.0).all()
    print({k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) > 0.05
    # tight where the variance is large, loose (by the kernel's own sensitivity) where s1 + s2 << C2
    flat = max(float(_ssim_all()[c.id][1].max()) for c in _of("ssim") if c.kind == "bright_flat")
    assert flat > 1e-4


SSIM_MUTANTS = {"sigma_1.6": dict(win=R.ssim_window(1.6)), "window_not_normalised": dict(win=R.ssim_window(normalise=False)),
                "C2_0.03": dict(C2=0.03), "smoothing_at_b10": dict(smooth_from=10), "no_channel_mean": dict(channel_mean=False)}


@pytest.mark.parametrize("name", sorted(SSIM_MUTANTS))
def test_ssim_bound_rejects(name):
    broken = []
    for c in _of("ssim"):
        a, b = R.inputs(c)
        ref, bound, _ = _ssim_all()[c.id]
        y = R.ssim_ref(a, b, c.block, **SSIM_MUTANTS[name])[0].astype(np.float32).astype(np.float64)
        if (np.abs(y - ref) > bound).any():
            broken.append(c.id)
    assert broken, f"{name}: inside the bound on every case"
    if name == "smoothing_at_b10":
        assert all("_b10_" in i for i in broken)
    if name == "no_channel_mean":
        assert all("_c3_" in i for i in broken)


# ------------------------------------------------------------------------------------------------------- discrimination
def _differs(op, mutant, pick=lambda c: True, index=0):
    hits = []
    for c in _of(op, SMALL):
        if pick(c) and not np.array_equal(R.expected(c)[index], R.expected(c, mutant=mutant)[index]):
            hits.append(c)
    return hits


def test_recompose_inputs_tell_the_mutants_apart():
    assert _differs("recompose", "strict"), "no map entry equals thr"
    hits = _differs("recompose", "trailing_a")
    assert {c.expect for c in hits} == {"recompose_rows_u8_kernel", "recompose_u8_kernel<true>", "recompose_u8_kernel<false>"}
    assert _differs("recompose", "no_clamp", lambda c: c.clamp_to is not None, index=1)


def test_area_inputs_tell_the_roundings_apart():
    cv2 = lambda f: (lambda c: c.factor == f and c.rounding == R.ROUND_CV2 and c.kind == "every_sum")
    # half-up in place of half-even.  An odd area has no tie (2 r == 9 has no solution), so at f = 3 the two roundings
    # are the same function and nothing can tell them apart; at f = 4 both kernels' cases do
    assert not _differs("area", "half_up", cv2(3))
    assert {c.expect for c in _differs("area", "half_up", cv2(4))} == {"area_downscale_u8_kernel", "area_downscale4_c3_kernel"}
    assert _differs("area", "half_up", lambda c: c.factor in (8, 16) and c.rounding == R.ROUND_CV2)
    # half-even at f = 2, where both rounding codes mean (s + 2) >> 2
    assert _differs("area", "half_even", cv2(2))
    assert _differs("area", "half_even", lambda c: c.factor == 4 and c.rounding == R.ROUND_HALF_UP and c.kind == "every_sum")


def test_blend_inputs_tell_the_mutants_apart():
    hits = _differs("blend", "y_div_block")
    assert hits and all(c.shape[1] % c.block or c.shape[2] % c.block for c in hits)
    assert len(_differs("blend", "round", lambda c: c.kind == "pairs")) >= 5       # every fractional alpha
    for c in _of("blend", SMALL):     # both clip ends are reached by the two alphas outside [0, 1]
        if c.kind == "pairs_positive" and (c.alpha > 1 or c.alpha < 0):
            o, r, m = R.inputs(c)
            v = o.astype(np.float64) * (1 - c.alpha) + r.astype(np.float64) * c.alpha
            assert (v < -1).any() and (v > 256).any()
            ref, = R.expected(c)
            assert (ref[v < -1] == 0).all() and (ref[v > 256] == 255).all()


def test_tile_inputs_tell_the_mutants_apart():
    assert _differs("normalize", "round") and _differs("normalize", "wsum_ge_0")
    rng = np.random.default_rng(5)
    hit = 0
    for c in _of("accumulate"):
        _, h, w, ch = c.shape
        acc, wsum = rng.standard_normal((h, w, ch)).astype(np.float32), rng.random((h, w)).astype(np.float32)
        a0, w0 = R.accumulate_expected(c, acc, wsum)
        a1, w1 = R.accumulate_expected(c, acc, wsum, mutant="single_rounding")
        hit += int(R.first_difference(w0, w1) is not None and R.first_difference(a0, a1) is not None)
        outside = np.ones((h, w), bool)
        for (y0, x0, th, tw, _) in c.tiles:
            outside[y0:y0 + th, x0:x0 + tw] = False
        assert R.first_difference(a0[outside], acc[outside]) is None and R.first_difference(w0[outside], wsum[outside]) is None
    assert hit == len(_of("accumulate"))


def test_sse_inputs_tell_the_mask_indexing_apart():
    hits = _differs("sse", "mask_by_byte", lambda c: c.mask == "random") + \
        _differs("sse", "mask_by_byte", lambda c: c.mask == "random", index=1)
    assert {c.shape[3] for c in hits} == {3, 4}
    assert not _differs("sse", "mask_by_byte", lambda c: c.shape[3] == 1)


def test_select_inputs_reach_every_outcome():
    for c in _of("select", SMALL):
        *vs, m = R.inputs(c)
        ref, = R.expected(c)
        assert (m < 0).any() and (m >= len(c.slots)).any(), c.id
        for s, v in enumerate(vs):
            assert (ref == v).any(), f"{c.id}: version {s} never picked"
        h, w, b = c.shape[1], c.shape[2], c.block
        assert not ref[:, h // b * b:].any() and not ref[:, :, w // b * b:].any()
        assert (ref[:, :h // b * b, :w // b * b] == 0).any()
