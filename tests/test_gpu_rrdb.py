"""csrc/rrdb.hip and elvis_amd/realesrgan.py on the device against the float64 statements of tests/_rrdb_ref.py.

The kernel matrix goes through the C ABI at the smallest shapes that reach every branch of an 8 x 32 pixel tile and a
32-channel K chunk (the kernel's constants): 1x1 (one pixel, all halo), 7x31 and 8x32 (one tile, ragged and exact),
9x33 (a second tile in both directions, one pixel wide), 17x70 (three tiles, ragged); n in {1, 2}; every cin (1..6
chunks), both cout.  The factors are covered in three sweeps rather than as a full product (7680 cases): every
(cin, cout), every (size, upsample, n), every (residuals, lrelu, cout); the other factors rotate inside each sweep.
"""
import math

import numpy as np
import pytest
import torch

import _rrdb_ref as R
from elvis_amd import _lib, realesrgan, restore, weights
from elvis_amd.recompose import frames_to_device, frames_to_host, maps_to_device, upscale_adaptive_device

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (7, 31), (8, 32), (9, 33), (17, 70))
CINS = (32, 64, 96, 128, 160, 192)
RES = ("", "1", "2", "12")


def _nchw(t):          # [n,h,w,c] device/host tensor -> float64 NCHW on the host
    return t.detach().cpu().permute(0, 3, 1, 2).double()


def _call(dev, x, cin, wp, bias, out, out_coff, cout, n, h, w, *, ups=0, lrelu=0, s0=1.0, s1=0.0, r1=None, r2=None, out_u8=0, swap=0):
    rc = _lib.lib().elvis_rrdb_conv3x3(x.data_ptr(), x.shape[-1], wp.data_ptr(), bias.data_ptr(), out.data_ptr(), out.shape[-1],
                                       out_coff, _lib.ptr(r1), 0 if r1 is None else r1.shape[-1], _lib.ptr(r2),
                                       0 if r2 is None else r2.shape[-1], n, h, w, cin, cout, ups, lrelu, s0, s1, out_u8, swap,
                                       _lib.stream_handle(dev))
    _lib.check(rc, dev)


def _packed(w, b, dev):
    packed, bias, cin, cout = realesrgan.pack_conv(w, b)
    return torch.from_numpy(packed.view(np.int16)).to(dev), torch.from_numpy(bias).to(dev), cin, cout


def _cases():
    out = []
    k = 0
    for cin in CINS:                                   # sweep 1: every (cin, cout)
        for cout in (32, 64):
            h, w = SIZES[1 + k % 4]
            ups = (k // 2) % 2 if h * w < 600 else 0
            out.append(dict(cin=cin, cout=cout, h=h, w=w, n=1 + k % 2, ups=ups, lrelu=k % 2, res=RES[k % 4], alias=not ups and k % 3 != 0))
            k += 1
    for h, w in SIZES:                                 # sweep 2: every (size, upsample, n)
        for ups in (0, 1):
            for n in (1, 2):
                cin = CINS[k % 6] if h * w < 600 or not ups else CINS[k % 3]
                out.append(dict(cin=cin, cout=(32, 64)[(k // 2) % 2], h=h, w=w, n=n, ups=ups, lrelu=(k // 3) % 2, res=RES[(k + 1) % 4],
                                alias=not ups and k % 2 == 0))
                k += 1
    for res in RES:                                    # sweep 3: every (residuals, lrelu, cout)
        for lrelu in (0, 1):
            for cout in (32, 64):
                out.append(dict(cin=64, cout=cout, h=9, w=33, n=1, ups=0, lrelu=lrelu, res=res, alias=k % 2 == 0))
                k += 1
    return out


def _case_id(c):
    return "cin{cin}_cout{cout}_{h}x{w}_n{n}_u{ups}_l{lrelu}_r{res}_a{alias:d}".format(**c)


@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_conv_matrix(gpu_device, case):
    cin, cout, h, w, n, ups, lrelu, res, alias = (case[k] for k in ("cin", "cout", "h", "w", "n", "ups", "lrelu", "res", "alias"))
    g = torch.Generator().manual_seed(sum(map(ord, _case_id(case))))
    ho, wo = (2 * h, 2 * w) if ups else (h, w)
    wt = torch.randn((cout, cin, 3, 3), generator=g) / math.sqrt(9 * cin)
    b = torch.randn(cout, generator=g) * 0.5
    wp, bias, _, _ = _packed(wt, b, gpu_device)
    if alias:          # the in-place concat: x and out are one buffer, channels [0, cin) read and [cin, cin + cout) written
        pitch = cin + cout + 8
        buf = torch.randn((n, h, w, pitch), generator=g).half()
        x_h, out_coff = buf, cin
    else:              # x_pitch > cin with channels the kernel must not read (NaN); out wider than cout
        x_h = torch.full((n, h, w, cin + 8), float("nan"), dtype=torch.float16)
        x_h[..., :cin] = torch.randn((n, h, w, cin), generator=g).half()
        out_coff = 0
    x_d = x_h.to(gpu_device)
    out_d = x_d if alias else torch.full((n, ho, wo, cout + 8), 7.0, dtype=torch.float16, device=gpu_device)
    r1_d = r2_d = None
    if "1" in res:
        # r1 may alias x: use x itself where its shape allows, else a tensor of its own with a pitch above cout
        r1_d = x_d if (not ups and cin >= cout) else (torch.randn((n, ho, wo, cout + 4), generator=g).half()).to(gpu_device)
    if "2" in res:
        r2_d = torch.randn((n, ho, wo, cout + 12), generator=g).half().to(gpu_device)
    r1_ref = None if r1_d is None else _nchw(r1_d)[:, :cout]
    r2_ref = None if r2_d is None else _nchw(r2_d)[:, :cout]
    s0, s1 = (0.2, 0.5) if res else (1.0, 0.0)
    before = x_d.clone()
    _call(gpu_device, x_d, cin, wp, bias, out_d, out_coff, cout, n, h, w, ups=ups, lrelu=lrelu, s0=s0, s1=s1, r1=r1_d, r2=r2_d)
    torch.cuda.synchronize()
    assert _lib.lib().elvis_last_launch() == f"rrdb_conv3x3_kernel<{cout}>".encode()
    ref = R.conv_ref(_nchw(x_h)[:, :cin], wt, b, upsample=bool(ups), lrelu=bool(lrelu), s0=s0, s1=s1, r1=r1_ref, r2=r2_ref)
    got = _nchw(out_d)
    y = got[:, out_coff:out_coff + cout]
    assert not torch.isnan(y).any()
    ratio = ((y - ref.ref).abs() / ref.bound()).max()
    print(f"{_case_id(case)}: worst |y - ref| / bound = {float(ratio):.3f}")
    assert float(ratio) <= 1.0
    # nothing but channels [out_coff, out_coff + cout) was written
    raw, raw0 = out_d.cpu().view(torch.int16), (before if alias else torch.full_like(out_d, 7.0)).cpu().view(torch.int16)
    assert torch.equal(raw[..., :out_coff], raw0[..., :out_coff]) and torch.equal(raw[..., out_coff + cout:], raw0[..., out_coff + cout:])
    if not alias:
        assert torch.equal(x_d.cpu().view(torch.int16), before.cpu().view(torch.int16))


@pytest.mark.parametrize("cin,h,w,n,swap,res", R.U8_CASES)
def test_conv_out_u8(gpu_device, cin, h, w, n, swap, res):
    wt, b, x_h, r1_h, r2_h = R.u8_inputs(cin, h, w, n, swap, res)
    wp, bias, cin_k, cout_k = _packed(wt, b, gpu_device)
    assert (cin_k, cout_k) == (cin, 32)
    ref = R.conv_ref(_nchw(x_h), wt, b, s0=1.0, s1=0.5, r1=None if r1_h is None else _nchw(r1_h)[:, :3],
                     r2=None if r2_h is None else _nchw(r2_h)[:, :3])
    byte, near = R.u8_ref(ref)
    share = float(near.double().mean())
    assert share < 0.02, f"{share:.4f} of the elements lie within 255 e of a half-integer"       # from the reference alone
    assert float((ref.ref < 0).double().mean()) > 0.01 and float((ref.ref > 1).double().mean()) > 0.01   # both clamps are reached
    out_d = torch.full((n, h, w, 3), 99, dtype=torch.uint8, device=gpu_device)
    dev = lambda t: None if t is None else t.to(gpu_device)
    _call(gpu_device, x_h.to(gpu_device), cin, wp, bias, out_d, 0, 32, n, h, w, s0=1.0, s1=0.5, r1=dev(r1_h), r2=dev(r2_h), out_u8=1, swap=swap)
    got = out_d.cpu().to(torch.int64).permute(0, 3, 1, 2)
    if swap:
        got = got.flip(1)
    diff = (got - byte).abs()
    print(f"out_u8 cin={cin} {h}x{w}: near-half share {share:.4f}, bytes off by one {int((diff == 1).sum())}")
    assert int(diff.max()) <= 1 and not (diff[~near] != 0).any()


@pytest.mark.parametrize("cin,cout,ups", [(64, 32, 0), (64, 64, 0), (96, 64, 1)])
def test_conv_exact_integers(gpu_device, cin, cout, ups):
    """Activations in {0, 1, 2} and an asymmetric pattern of weights in {-1, 0, 1}: every partial sum is a small
    integer, exact in fp32, and the results (|.| <= 2 * 9 * 96) are exact in f16, so a transposed or permuted fragment
    map cannot hide behind a tolerance."""
    n, h, w = 2, 9, 33
    co, ci, ky, kx = torch.meshgrid(torch.arange(cout), torch.arange(cin), torch.arange(3), torch.arange(3), indexing="ij")
    wt = ((co * 7 + ci * 3 + ky * 5 + kx * 11 + (co * ci) % 4) % 3 - 1).float()
    assert not torch.equal(wt, wt.flip(2)) and not torch.equal(wt, wt.flip(3)) and not torch.equal(wt[:32, :32], wt[:32, :32].transpose(0, 1))
    b = (torch.arange(cout) % 5 - 2).float()
    yy, xx, cc = torch.meshgrid(torch.arange(h), torch.arange(w), torch.arange(cin), indexing="ij")
    x_h = torch.stack([((yy * 3 + xx * 5 + cc * 7 + i) % 3) for i in range(n)]).half()
    wp, bias, _, _ = _packed(wt, b, gpu_device)
    ho, wo = (2 * h, 2 * w) if ups else (h, w)
    out_d = torch.zeros((n, ho, wo, cout), dtype=torch.float16, device=gpu_device)
    _call(gpu_device, x_h.to(gpu_device), cin, wp, bias, out_d, 0, cout, n, h, w, ups=ups)
    ref = R.conv_ref(_nchw(x_h), wt, b, upsample=bool(ups)).ref
    assert float(ref.abs().max()) <= 2048
    assert torch.equal(_nchw(out_d), ref)


def test_conv_one_real_channel(gpu_device):
    """One real input and one real output channel packed into 32 x 32: the padded weights are zero, so the other input
    channels (arbitrary values) do not reach the output and the other output channels are exactly the zero bias."""
    n, h, w = 1, 9, 33
    g = torch.Generator().manual_seed(9)
    wt = torch.randn((1, 1, 3, 3), generator=g)
    b = torch.tensor([0.25])
    wp, bias, cin, cout = _packed(wt, b, gpu_device)
    assert (cin, cout) == (32, 32)
    x_h = (torch.randn((n, h, w, 32), generator=g) * 100).half()
    out_d = torch.full((n, h, w, 32), 7.0, dtype=torch.float16, device=gpu_device)
    _call(gpu_device, x_h.to(gpu_device), 32, wp, bias, out_d, 0, 32, n, h, w)
    ref = R.conv_ref(_nchw(x_h)[:, :1], wt, b)
    y = _nchw(out_d)
    assert float(((y[:, :1] - ref.ref).abs() / ref.bound()).max()) <= 1.0
    assert not y[:, 1:].any()


def test_conv_offsets_past_2_31(gpu_device):
    """2 x 4100 x 8192 pixels of 32 channels: 2^31 + 2.1 M elements a tensor, so the last rows of the second image sit
    past a 32-bit element offset on the input and on the output side.  Those rows are checked against the reference."""
    n, h, w, c = 2, 4100, 8192, 32
    assert n * h * w * c > 2 ** 31
    g = torch.Generator().manual_seed(31)
    wt = torch.randn((c, c, 3, 3), generator=g) / math.sqrt(9 * c)
    b = torch.randn(c, generator=g) * 0.5
    wp, bias, _, _ = _packed(wt, b, gpu_device)
    x_d = torch.empty((n, h, w, c), dtype=torch.float16, device=gpu_device)
    x_d.view(-1)[:1 << 20].normal_()
    tail = (torch.randn((6, w, c), generator=g)).half()
    x_d[1, -6:] = tail.to(gpu_device)
    out_d = torch.empty((n, h, w, c), dtype=torch.float16, device=gpu_device)
    out_d[1, -4:] = 7.0
    _call(gpu_device, x_d, c, wp, bias, out_d, 0, c, n, h, w, lrelu=1)
    ref = R.conv_ref(tail.permute(2, 0, 1)[None].double(), wt, b, lrelu=True)
    y = _nchw(out_d[1:2, -4:])
    ratio = ((y - ref.ref[:, :, 2:]).abs() / ref.bound()[:, :, 2:]).max()
    assert float(ratio) <= 1.0


@pytest.mark.parametrize("s,h,w", [(1, 1, 1), (1, 5, 7), (1, 8, 32), (2, 4, 6), (2, 5, 7), (2, 3, 3), (2, 8, 33), (2, 17, 70)])
def test_input_u8(gpu_device, s, h, w):
    g = torch.Generator().manual_seed(h * 100 + w)
    frames = torch.randint(0, 256, (2, h, w, 3), generator=g, dtype=torch.uint8)
    frames[0, 0, 0] = torch.tensor([0, 255, 128], dtype=torch.uint8)
    for swap in (0, 1):
        ho, wo = -(-h // s), -(-w // s)
        out = torch.full((2, ho, wo, 32), 7.0, dtype=torch.float16, device=gpu_device)
        _lib.check(_lib.lib().elvis_rrdb_input_u8(frames.to(gpu_device).data_ptr(), out.data_ptr(), 2, h, w, s, swap,
                                                  _lib.stream_handle(gpu_device)), gpu_device)
        want = R.input_ref(frames, s, bool(swap))
        assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


# ----------------------------------------------------------------------------- the model
MODEL_CASES = {"x4_b2": (4, 2), "x2_b1": (2, 1)}


@pytest.fixture(scope="module")
def model_refs():
    """Per configuration: the seeded 24 x 40 frame, the weights, the float64 statement, and d - the max-abs distance
    between it and the same statement with f16 storage (fp32 arithmetic): what f16 storage alone costs on this input."""
    out = {}
    for name, (scale, blocks) in MODEL_CASES.items():
        cfg = weights.RRDBNetConfig(scale=scale, num_block=blocks)
        sd = weights.make_rrdbnet_weights(cfg, 0)
        frame = torch.randint(0, 256, (1, 24, 40, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8)
        ref64 = R.rrdbnet_ref(sd, scale, blocks, frame)
        ref16 = R.rrdbnet_ref(sd, scale, blocks, frame, storage_f16=True)
        out[name] = dict(cfg=cfg, sd=sd, frame=frame, ref=ref64, d=float((ref64 - ref16).abs().max()))
    return out


@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_model_against_the_float64_statement(gpu_device, model_refs, name):
    """The device output before quantisation is within 2 d of the float64 statement (d: what f16 storage alone costs,
    `model_refs`; the factor 2 covers the different summation order), the bytes within ceil(255 * 2 d) + 1.
    Measured on an MI355X: x4_b2 d = 6.81e-8, device 6.04e-8; x2_b1 d = 6.38e-8, device 6.30e-8; bytes equal in both."""
    m = model_refs[name]
    model = realesrgan.RRDBNetModel(m["cfg"], m["sd"], gpu_device)
    frame_d = m["frame"].to(gpu_device)
    y = model.forward(frame_d, swap_rb=False, as_float=True)
    s = m["cfg"].scale
    assert y.shape == (1, 24 * s, 40 * s, 3) and y.dtype == torch.float16
    dist = float((_nchw(y) - m["ref"]).abs().max())
    print(f"{name}: d = {m['d']:.3e}, device distance = {dist:.3e}, output max |.| = {float(m['ref'].abs().max()):.3e}")
    assert m["d"] > 0 and dist <= 2 * m["d"]
    u8 = model.forward(frame_d, swap_rb=False)
    assert u8.shape == (1, 24 * s, 40 * s, 3) and u8.dtype == torch.uint8
    off = int((u8.cpu().to(torch.int64) - R.to_bytes(m["ref"])).abs().max())
    print(f"{name}: bytes off by at most {off}")
    assert off <= math.ceil(255 * 2 * m["d"]) + 1
    # BGR in and out is the same network on the reversed channels
    bgr = model.forward(frame_d.flip(-1).contiguous(), swap_rb=True)
    assert torch.equal(bgr.flip(-1), u8)


def test_model_bytes_on_a_visible_output(gpu_device):
    """The synthetic default weights give outputs near zero; here the last conv is rescaled so that the bytes cover
    the whole range, and the same two bounds are asked of them."""
    cfg = weights.RRDBNetConfig(scale=4, num_block=1)
    sd = weights.make_rrdbnet_weights(cfg, 5)
    frame = torch.randint(0, 256, (1, 24, 40, 3), generator=torch.Generator().manual_seed(12), dtype=torch.uint8)
    probe = R.rrdbnet_ref(sd, 4, 1, frame)
    sd["conv_last.weight"] = sd["conv_last.weight"] * float(0.3 / probe.std())
    sd["conv_last.bias"] = torch.full((3,), 0.5)
    ref64 = R.rrdbnet_ref(sd, 4, 1, frame)
    d = float((ref64 - R.rrdbnet_ref(sd, 4, 1, frame, storage_f16=True)).abs().max())
    model = realesrgan.RRDBNetModel(cfg, sd, gpu_device)
    y = model.forward(frame.to(gpu_device), swap_rb=False, as_float=True)
    dist = float((_nchw(y) - ref64).abs().max())
    want = R.to_bytes(ref64)
    assert int(want.min()) == 0 and int(want.max()) == 255
    off = int((model.forward(frame.to(gpu_device), swap_rb=False).cpu().to(torch.int64) - want).abs().max())
    print(f"visible output: d = {d:.3e}, device distance = {dist:.3e}, bytes off by at most {off}")
    assert dist <= 2 * d and off <= math.ceil(255 * 2 * d) + 1


def test_model_batch_independence_and_odd_sizes(gpu_device, monkeypatch):
    g = torch.Generator().manual_seed(3)
    for scale, (h, w) in ((4, (9, 33)), (2, (10, 34)), (2, (9, 33))):
        model = realesrgan.RRDBNetModel(weights.RRDBNetConfig(scale=scale, num_block=1), None, gpu_device)
        frames = torch.randint(0, 256, (3, h, w, 3), generator=g, dtype=torch.uint8).to(gpu_device)
        all3 = model.forward(frames)
        assert all3.shape == (3, scale * h, scale * w, 3)
        for i in range(3):
            assert torch.equal(model.forward(frames[i:i + 1]), all3[i:i + 1])
        monkeypatch.setattr(realesrgan, "MAX_INVOCATION_BYTES", 1)         # one frame per invocation
        assert model.max_batch(h, w) == 1 and torch.equal(model.forward(frames), all3)
        monkeypatch.undo()
    # an odd x2 size is the even one with a reflected row and column, cropped
    odd = torch.randint(0, 256, (1, 9, 33, 3), generator=g, dtype=torch.uint8)
    padded = torch.cat((odd, odd[:, -2:-1]), 1)
    padded = torch.cat((padded, padded[:, :, -2:-1]), 2)
    assert torch.equal(model.forward(odd.to(gpu_device)), model.forward(padded.to(gpu_device))[:, :18, :66])


# ----------------------------------------------------------------------------- the public surface
@pytest.mark.parametrize("model_name", ["RealESRGAN_x4plus_anime_6B", "RealESRGAN_x2plus"])
def test_restore_frames_realesrgan_is_the_composition(gpu_device, model_name):
    rng = np.random.default_rng(21)
    frames = [rng.integers(0, 256, size=(32, 48, 3), dtype=np.uint8) for _ in range(4)]
    maps = np.zeros((4, 2, 3), np.int32)
    maps[0] = [[2, 0, 1], [0, 2, 0]]
    maps[1] = [[1, 0, 0], [0, 1, 1]]
    maps[3] = [[0, 2, 2], [1, 0, 0]]                   # frame 2: all zero
    out = restore.restore_frames_realesrgan(frames, maps, 16, gpu_device, model_name=model_name, tile=256, tile_pad=4)
    model = restore.get_realesrgan_upsampler(gpu_device, model_name=model_name)
    assert model.scale == weights.realesrgan_config(model_name).scale
    assert restore.get_realesrgan_upsampler(gpu_device, model_name=model_name + ".pth") is model
    for i, f in enumerate(frames):
        if not maps[i].any():
            want = f                                    # an all-zero map returns the frame
        else:
            want = frames_to_host(upscale_adaptive_device(frames_to_device([f], gpu_device), maps_to_device(maps[i:i + 1], 1, gpu_device),
                                                          16, lambda cur: model.forward(cur, swap_rb=True), sr_scale=model.scale))[0]
        assert np.array_equal(out[i], want), i
    assert not np.array_equal(out[0], frames[0])
    zero = restore.restore_frames_realesrgan(frames, np.zeros_like(maps), 16, gpu_device, model_name=model_name)
    assert all(np.array_equal(a, b) for a, b in zip(zero, frames))
    if model.scale == 4:
        single = restore.restore_frames_realesrgan(frames[:1], maps[:1], 16, gpu_device, model_name=model_name, schedule="single4x")
        from elvis_amd import ops
        fd = frames_to_device(frames[:1], gpu_device)
        want = ops.recompose_u8(fd, model.forward(ops.area_downscale_u8(fd, 4)), maps_to_device(maps[:1], 1, gpu_device), 16, 0)
        assert np.array_equal(single[0], frames_to_host(want)[0])
    else:
        with pytest.raises(ValueError, match="single4x"):
            restore.restore_frames_realesrgan(frames[:1], maps[:1], 16, gpu_device, model_name=model_name, schedule="single4x")
    # P1 and P3
    up = restore.get_realesrgan_upsample_fn(gpu_device, model_name=model_name, scale=2)(frames[0])
    assert up.shape == (64, 96, 3) and up.dtype == np.uint8
    naive = restore.restore_with_realesrgan_naive(frames=[frames[0][:, :, ::-1].copy()], device=gpu_device, model_name=model_name,
                                                  tile_coords=(0, 0))
    assert naive[0].shape == (32, 48, 3)


def test_checkpoint_file_reproduces_the_seeded_model(gpu_device, tmp_path):
    name = "RealESRGAN_x4plus_anime_6B"
    rng = np.random.default_rng(22)
    frames = [rng.integers(0, 256, size=(16, 32, 3), dtype=np.uint8) for _ in range(2)]
    maps = np.array([[[2, 1]], [[0, 2]]], np.int32)
    seeded = restore.restore_frames_realesrgan(frames, maps, 16, gpu_device, model_name=name)
    path = tmp_path / "RealESRGAN_x4plus_anime_6B.pth"
    torch.save({"params_ema": weights.make_rrdbnet_weights(weights.realesrgan_config(name), 0)}, path)
    loaded = restore.restore_frames_realesrgan(frames, maps, 16, gpu_device, model_name=name, model_path=str(path))
    assert restore.get_realesrgan_upsampler(gpu_device, model_name=name, model_path=str(path)) is not \
        restore.get_realesrgan_upsampler(gpu_device, model_name=name)
    assert all(np.array_equal(a, b) for a, b in zip(seeded, loaded))
    bad = tmp_path / "bad.pth"
    torch.save({"params": {"conv_first.weight": torch.zeros(64, 3, 3, 3)}}, bad)
    with pytest.raises(ValueError, match="missing key"):
        restore.restore_frames_realesrgan(frames, maps, 16, gpu_device, model_name=name, model_path=str(bad))


def test_restore_yuv_clip_realesrgan(gpu_device, tmp_path):
    """The clip-file driver's "realesrgan" kind: the resident restorer between the two I420 conversions."""
    from elvis_amd import drivers, handoff
    rng = np.random.default_rng(23)
    frames = [rng.integers(0, 256, size=(32, 48, 3), dtype=np.uint8) for _ in range(3)]
    maps = np.array([[[1, 0, 1], [0, 1, 0]], [[0, 0, 0], [0, 0, 0]], [[0, 1, 1], [1, 0, 0]]], np.int32)
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    handoff.write_y4m(frames, src, 25, gpu_device)
    drivers.restore_yuv_clip("realesrgan", src, dst, maps, 16, devices=[gpu_device], model_name="RealESRGAN_x2plus")
    clip = handoff.load_y4m_device(src, gpu_device, "bgr")
    want = handoff.rgb_to_i420_device(restore.restore_frames_realesrgan_device(clip, maps, 16, model_name="RealESRGAN_x2plus"), "bgr")
    head = len(handoff.y4m_header(48, 32, 25))
    got = np.frombuffer(open(dst, "rb").read()[head:], np.uint8).reshape(3, 6 + 32 * 48 * 3 // 2)
    assert bytes(got[0, :6]) == b"FRAME\n"
    assert np.array_equal(got[:, 6:].reshape(3, 48, 48), want.cpu().numpy())
    assert not np.array_equal(got[0, 6:], handoff.rgb_to_i420_device(clip, "bgr").cpu().numpy()[0].reshape(-1))
    with pytest.raises(ValueError, match="fp32"):
        drivers.restore_yuv_clip("realesrgan", src, dst, maps, 16, devices=[gpu_device], fp32=True)
