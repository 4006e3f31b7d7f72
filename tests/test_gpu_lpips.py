"""LPIPS (AlexNet) on the device against the float64 statement of tests/_lpips_ref.py.

Per kernel, against float64 fed the device's own input: the stem and the 5x5 conv within the error model of
tests/_convref.py (1/2 ulp + (K + 2) 2^-24 sum|x||w|, K = 363 and 1600), the max-pool bit-exact, the distance per tap
within a bound derived below.  End to end the score is within DEVICE_BAR = 32 x the CPU float32 figure of the float64
restatement (relative to max(|ref|, 1e-6)):

    CPU float32 worst 1.986e-6   |   device bar 6.37e-5   |   worst device value observed 1.72e-6 (MI355X; the one-LSB case)

Every output lies between guard words that must come back untouched.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _convref as CR
import _lpips_ref as R
from elvis_amd import _lib, lpips, metrics, ops

pytestmark = pytest.mark.gpu
GUARD = 64                                    # floats (256 bytes) of guard on either side of an output
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def model(gpu_device):
    return lpips.LpipsAlex(None, gpu_device)


def guarded(shape, device, dtype=torch.float32):
    n = int(np.prod(shape))
    full = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=device)
    return full, full[GUARD:GUARD + n].view(shape)


def guards_intact(full):
    return bool((full[:GUARD] == SENTINEL).all()) and bool((full[-GUARD:] == SENTINEL).all())


def last_launch():
    return _lib.lib().elvis_last_launch().decode()


def nchw(t: torch.Tensor, c: int) -> torch.Tensor:
    return t[..., :c].permute(0, 3, 1, 2).double().cpu()


# ----------------------------------------------------------------------------- per kernel
@pytest.mark.parametrize("order", ["bgr", "rgb"])
def test_stem_within_the_conv_error_model(model, gpu_device, order):
    """70 x 90 frames, a rect with odd origin, a 60 % mask: 14 x 18 outputs, more than one tile, ragged on both sides."""
    case = R.BY_ID["rect_odd_masked"]
    a, _, m = R.inputs(case)
    y0, y1, x0, x1 = case.rect
    a_d, m_d = torch.from_numpy(a.copy()).to(gpu_device), torch.from_numpy(m.copy()).to(gpu_device)
    ho, wo = (y1 - y0 - 7) // 4 + 1, (x1 - x0 - 7) // 4 + 1
    full, view = guarded((a.shape[0], ho, wo, 64), gpu_device)
    lpips.stem_device(a_d, model, m_d, case.rect, order, out=ops.Act(view, 64))
    assert last_launch() == f"lpips_stem_kernel<{int(order == 'bgr')}>"
    got = nchw(view, 64)
    assert guards_intact(full)
    rgb = a[..., ::-1] if order == "bgr" else a
    seen = np.where(m[..., None] != 0, rgb, 0)[:, y0:y1, x0:x1]
    x_hat = torch.from_numpy(R.affine_f32(seen)).double().permute(0, 3, 1, 2)          # the operands the kernel multiplies
    sd = R.weights()
    ref = CR.conv_ref(x_hat, sd["features.0.weight"].double(), sd["features.0.bias"].double(), None, ksize=11, stride=4, pad=2, act=3,
                      out_f16=False)
    assert ref.kt == 363 and tuple(got.shape) == tuple(ref.z.shape)
    ok, worst, at = CR.tier1(got, ref)
    print(f"stem {order}: worst |err| / bound = {worst:.3g} at {at}")
    assert ok
    # the float64 contract itself (affine in float64) is as close: the fp32 affine costs a few ulp of one operand
    x64 = R.network_input(a, order, m, case.rect)
    ref64 = CR.conv_ref(x64, sd["features.0.weight"].double(), sd["features.0.bias"].double(), None, ksize=11, stride=4, pad=2, act=3,
                        out_f16=False)
    assert float((got - ref64.ref).abs().max()) <= 2 * float(ref64.bound().max())


@pytest.mark.parametrize("n,h,w", [(2, 9, 21), (1, 3, 3), (1, 4, 16), (1, 15, 33)])
def test_conv5_within_the_conv_error_model(model, gpu_device, n, h, w):
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn(n, h, w, 64, generator=g)
    full, view = guarded((n, h, w, 192), gpu_device)
    lib = _lib.lib()
    x_d = x.to(gpu_device)
    _lib.check(lib.elvis_lpips_conv5_f32(x_d.data_ptr(), model.conv5_w.data_ptr(), model.conv5_b.data_ptr(), view.data_ptr(), n, h, w, 64, 192,
                                         torch.cuda.current_stream(gpu_device).cuda_stream), gpu_device)
    assert last_launch() == "lpips_conv5_kernel"
    got = nchw(view, 192)
    assert guards_intact(full)
    sd = R.weights()
    ref = CR.conv_ref(x.permute(0, 3, 1, 2).double(), sd["features.3.weight"].double(), sd["features.3.bias"].double(), None, ksize=5, pad=2,
                      act=3, out_f16=False)
    assert ref.kt == 1600
    ok, worst, at = CR.tier1(got, ref)
    print(f"conv5 {n}x{h}x{w}: worst |err| / bound = {worst:.3g} at {at}")
    assert ok


@pytest.mark.parametrize("n,h,w,c", [(2, 9, 12, 64), (1, 7, 7, 192), (1, 3, 3, 64), (3, 8, 11, 192)])
def test_maxpool_is_bit_exact(gpu_device, n, h, w, c):
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn(n, h, w, c, generator=g)
    ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    full, view = guarded((n, ho, wo, c), gpu_device)
    x_d = x.to(gpu_device)
    _lib.check(_lib.lib().elvis_lpips_maxpool_f32(x_d.data_ptr(), view.data_ptr(), n, h, w, c, c, c,
                                                  torch.cuda.current_stream(gpu_device).cuda_stream), gpu_device)
    assert last_launch() == "lpips_maxpool_kernel"
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1)
    assert torch.equal(view.cpu(), want) and guards_intact(full)


def distance_tolerance(xd, yd, lin):
    """The bound of test_distance_per_tap (its docstring derives it) for float64 NCHW features and one tap's weights."""
    xh = xd / (torch.sqrt((xd * xd).sum(1, keepdim=True)) + 1e-10)
    yh = yd / (torch.sqrt((yd * yd).sum(1, keepdim=True)) + 1e-10)
    d = (xh - yh).abs()
    return (32 * CR.U24 * ((d * (xh.abs() + yh.abs()) + d * d) * lin.double()[None, :, None, None]).sum(1).mean((1, 2))).numpy()


@pytest.mark.parametrize("tap", range(5))
def test_distance_per_tap(model, gpu_device, tap):
    """Bound: xh carries at most ~9 roundings of 2^-24 (the sum of squares: a chain of up to 6 and 6 butterfly steps, halved
    by the sqrt; the sqrt, the + 1e-10 and the divide), so d = xh - yh is off by 9 u (|xh| + |yh|) + u |d| / 2, d^2 by twice
    |d| times that, and the weighted sum adds at most 12 u v: in all under 18 u sum_c w_c (|d| (|xh| + |yh|) + d^2) per
    pixel.  The test allows 32 u of that sum, averaged over the pixels; the float64 sum over pixels adds nothing."""
    c = R.TAP_CHANNELS[tap]
    n, h, w = 2, 5, 27                                                       # 135 pixels: three workgroups, the last one ragged
    g = torch.Generator().manual_seed(tap)
    x, y = torch.relu(torch.randn(n, h, w, c, generator=g)), torch.relu(torch.randn(n, h, w, c, generator=g))
    x[0, 2, 3] = 0.0                                                         # a pixel without any feature: 0 / 1e-10
    y[1, 4, 26] = x[1, 4, 26]
    lin = R.weights()[f"lin{tap}.model.1.weight"].reshape(-1)
    full, view = guarded((n,), gpu_device, torch.float64)
    view.fill_(7.0)
    lpips.distance_device(x.to(gpu_device), y.to(gpu_device), c, model.lin[tap], view, accumulate=False)
    assert last_launch() == "lpips_finish_kernel"
    got = view.cpu().numpy().copy()
    xd, yd = x.permute(0, 3, 1, 2).double(), y.permute(0, 3, 1, 2).double()
    want = R.tap_distance(xd, yd, lin).numpy()
    tol = distance_tolerance(xd, yd, lin)
    print(f"tap {tap}: got {got}, want {want}, |err| / tol = {np.abs(got - want) / tol}")
    assert (np.abs(got - want) <= tol).all()
    lpips.distance_device(x.to(gpu_device), y.to(gpu_device), c, model.lin[tap], view, accumulate=True)
    assert np.array_equal(view.cpu().numpy(), got + got) and guards_intact(full)


def test_distance_partials_are_the_distance_kernels_own_output(model, gpu_device):
    """elvis_lpips_distance_f64 with a workspace of the test's own: lpips_distance_kernel writes one float64 partial sum a
    workgroup and nothing else, lpips_finish_kernel reads nothing else.  The partials of a frame add up to the float64
    reference times the pixel count within test_distance_per_tap's bound, and the result is their sum in index order
    divided by the pixel count, bit for bit."""
    from elvis_amd._lib import check, lib, ptr, stream_handle
    tap, (n, h, w) = 1, (2, 5, 27)
    c = R.TAP_CHANNELS[tap]
    g = torch.Generator().manual_seed(50)
    x, y = torch.relu(torch.randn(n, h, w, c, generator=g)), torch.relu(torch.randn(n, h, w, c, generator=g))
    lin = R.weights()[f"lin{tap}.model.1.weight"].reshape(-1)
    blocks = lib().elvis_lpips_distance_workspace_bytes(n, h, w) // 8 // n
    assert blocks == 3 and lib().elvis_lpips_distance_workspace_bytes(n, h, w) == n * blocks * 8
    wfull, ws = guarded((n * blocks,), gpu_device, torch.float64)
    ws.fill_(float("nan"))
    ofull, out = guarded((n,), gpu_device, torch.float64)
    xd_, yd_ = x.to(gpu_device), y.to(gpu_device)
    check(lib().elvis_lpips_distance_f64(ptr(xd_), ptr(yd_), ptr(model.lin[tap]), ptr(ws), ptr(out), n, h, w, c, c, 0,
                                         stream_handle(gpu_device)), gpu_device)
    partial, got = ws.cpu().numpy().reshape(n, blocks), out.cpu().numpy()
    xd, yd = x.permute(0, 3, 1, 2).double(), y.permute(0, 3, 1, 2).double()
    want, tol = R.tap_distance(xd, yd, lin).numpy(), distance_tolerance(xd, yd, lin)
    assert np.isfinite(partial).all() and (partial > 0).all()
    assert (np.abs(partial.sum(1) / (h * w) - want) <= tol).all()
    serial = np.zeros(n)
    for b in range(blocks):
        serial = serial + partial[:, b]
    assert np.array_equal(got, serial / float(h * w)) and guards_intact(wfull) and guards_intact(ofull)


# ----------------------------------------------------------------------------- end to end
def run(case, model, device, **kw):
    a, b, m = R.inputs(case)
    up = lambda t: None if t is None else torch.from_numpy(t.copy()).to(device)
    return lpips.lpips_device(up(a), up(b), model, masks=up(m), rect=case.rect, order=case.order, **kw).cpu().numpy()


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_score_against_float64(model, gpu_device, case):
    got = run(case, model, gpu_device)
    want = R.expected(case.id)
    err = R.rel(got, want)
    print(f"{case.id}: device {got}, float64 {want}, rel {err:.3g} (bar {R.DEVICE_BAR:.3g})")
    assert got.dtype == np.float64 and got.shape == want.shape
    assert err <= R.DEVICE_BAR
    if case.pair == "identical":
        assert (got == 0.0).all()
    if case.pair == "one_lsb":
        assert 0.0 < got[0] < 1e-6
    for mutant, cid in R.MUTANTS.items():                                     # the device sides with the contract, not the mutant
        if cid == case.id:
            assert R.rel(got, R.expected(cid, mutant)) >= (R.MUTANT_MIN_BARS - 1) * R.DEVICE_BAR


def test_a_frame_scores_the_same_alone_and_in_a_batch(model, gpu_device):
    case = R.BY_ID["n3_33x38"]
    a, b, _ = R.inputs(case)
    both = run(case, model, gpu_device)
    for f in range(3):
        alone = lpips.lpips_device(torch.from_numpy(a[f:f + 1].copy()).to(gpu_device), torch.from_numpy(b[f:f + 1].copy()).to(gpu_device), model)
        assert alone.cpu().numpy().tobytes() == both[f:f + 1].tobytes()
    seven = np.concatenate([a, a, a[:1]]), np.concatenate([b, b, b[:1]])      # more pairs than one pass keeps resident
    got = lpips.lpips_device(torch.from_numpy(seven[0]).to(gpu_device), torch.from_numpy(seven[1]).to(gpu_device), model).cpu().numpy()
    assert got.tobytes() == np.concatenate([both, both, both[:1]]).tobytes()


def test_host_surface_chunks_none_and_mixed_sizes(model, gpu_device):
    case = R.BY_ID["n3_33x38"]
    a, b, _ = R.inputs(case)
    want = run(case, model, gpu_device)
    refs, decs = [a[0], None, a[1], a[2]], [b[0], b[1], b[1], b[2], b[0]]
    for chunk in (1, 2, None):
        got = lpips.calculate_lpips_per_frame(refs, decs, device=gpu_device, model=model, chunk_frames=chunk)
        assert isinstance(got, list) and np.asarray(got).tobytes() == want.tobytes()
    assert lpips.calculate_lpips(refs, decs, model) == got
    assert lpips.calculate_lpips_per_frame(refs[:1], decs[:1], device=gpu_device) == got[:1]      # the cached seed-0 model
    assert lpips.get_lpips_model(gpu_device) is lpips.get_lpips_model("cuda")
    small, _, _ = R.inputs(R.BY_ID["min_31x31"])
    mixed = lpips.calculate_lpips_per_frame([a[0], small[0], a[1]], [b[0], small[0], b[1]], device=gpu_device, model=model)
    assert mixed[1] == 0.0 and mixed[0] == got[0] and mixed[2] == got[1]
    with pytest.raises(ValueError, match="chunk_frames"):
        lpips.calculate_lpips_per_frame(refs, decs, device=gpu_device, model=model, chunk_frames=0)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_views_off_a_dword_give_the_same_bytes(model, gpu_device, off):
    case = R.BY_ID["rect_odd_masked"]
    a, b, m = R.inputs(case)
    want = run(case, model, gpu_device)

    def shifted(arr):
        buf = torch.zeros(arr.size + 8, dtype=torch.uint8, device=gpu_device)
        view = buf[off:off + arr.size].view(arr.shape)
        view.copy_(torch.from_numpy(arr.copy()))
        assert view.data_ptr() % 4 == off and view.is_contiguous()
        return view
    got = lpips.lpips_device(shifted(a), shifted(b), model, masks=shifted(m), rect=case.rect).cpu().numpy()
    assert got.tobytes() == want.tobytes()


def test_argument_errors(model, gpu_device):
    a = torch.zeros((1, 40, 50, 3), dtype=torch.uint8, device=gpu_device)
    for kw, msg in [(dict(rect=(0, 30, 0, 50)), "at least 31"), (dict(rect=(0, 40, 10, 40)), "at least 31"), (dict(rect=(0, 41, 0, 50)), "inside"),
                    (dict(rect=(-1, 40, 0, 50)), "inside"), (dict(order="gbr"), "order"),
                    (dict(masks=torch.zeros((1, 40, 49), dtype=torch.uint8, device=gpu_device)), "masks")]:
        with pytest.raises(ValueError, match=msg):
            lpips.lpips_device(a, a, model, **kw)
    with pytest.raises(ValueError, match="at least 31"):
        lpips.lpips_device(a[:, :30].contiguous(), a[:, :30].contiguous(), model)
    with pytest.raises(ValueError, match="one shape"):
        lpips.lpips_device(a, a[:, :35].contiguous(), model)
    with pytest.raises(ValueError, match="uint8"):
        lpips.lpips_device(a.float(), a.float(), model)
    assert lpips.lpips_device(a[:0], a[:0], model).shape == (0,)


# ----------------------------------------------------------------------------- the evaluator
def test_evaluator_with_a_model_adds_the_lpips_keys_and_nothing_else(model, gpu_device):
    rng = np.random.default_rng(7)
    h, w, count = 48, 64, 5
    yy, xx = np.mgrid[:h, :w]
    refs, decs, fgs = [], [], []
    for i in range(count):
        base = np.stack([110 + 70 * np.sin((yy + 2 * i) / 6.0 + c) * np.cos((xx - i) / 9.0) for c in range(3)], axis=-1)
        r = np.clip(base + rng.normal(0, 5, base.shape), 0, 255).astype(np.uint8)
        fg = ((yy - 22 - i) ** 2 + (xx - 28 - 2 * i) ** 2) < 260
        refs.append(r)
        decs.append(np.clip(r.astype(np.float64) + rng.normal(0, 1, r.shape) * np.where(fg[..., None], 3.0, 12.0), 0, 255).astype(np.uint8))
        fgs.append(fg)
    plain = metrics.evaluate_fg_bg_metrics(refs, decs, fgs, metric_stride=2, device=gpu_device)
    with_model = metrics.evaluate_fg_bg_metrics(refs, decs, fgs, metric_stride=2, device=gpu_device, lpips_model=model)
    idx = metrics.metric_frame_indices(count, 2)
    bx, by, bw, bh = metrics.compute_mask_union_bbox(fgs, w, h, device=gpu_device)
    ys, xs = slice(by, min(h, by + max(1, bh))), slice(bx, min(w, bx + max(1, bw)))
    assert ys.stop - ys.start >= 31 and xs.stop - xs.start >= 31 and (ys.start, xs.start) != (0, 0)
    mask = lambda f, m: np.where(m[..., None], f, 0).astype(np.uint8)
    by_hand = {
        "foreground": lpips.calculate_lpips_per_frame([np.ascontiguousarray(mask(refs[i], fgs[i])[ys, xs]) for i in idx],
                                                      [np.ascontiguousarray(mask(decs[i], fgs[i])[ys, xs]) for i in idx], device=gpu_device, model=model),
        "background": lpips.calculate_lpips_per_frame([mask(refs[i], ~fgs[i]) for i in idx], [mask(decs[i], ~fgs[i]) for i in idx],
                                                      device=gpu_device, model=model),
    }
    for region in ("foreground", "background"):
        assert set(with_model[region]) == set(plain[region]) | {"lpips_mean", "lpips_std"}
        for key, value in plain[region].items():
            assert np.float64(value).tobytes() == np.float64(with_model[region][key]).tobytes(), key
        assert with_model[region]["lpips_mean"] == float(np.mean(by_hand[region])) > 0.0
        assert with_model[region]["lpips_std"] == float(np.std(by_hand[region]))
