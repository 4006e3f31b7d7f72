"""The SRVGGNetCompact models of the Real-ESRGAN slot without a GPU: the name table, the layout, state-dict validation,
deep network interpolation, what the getter refuses before it needs a device, the host packing against its numpy
statement, the argument checks of the entry points, the pixel-shuffle order of the reference statement and the inputs of
the u8 device cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _srvgg_ref as R
from elvis_amd import _build, _lib, drivers, restore, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"realesr-animevideov3": 16, "realesr-general-x4v3": 32}


# ----------------------------------------------------------------------------- names, layout, weights
def test_name_table_and_layout():
    assert weights.REALESRGAN_SRVGG_MODELS == tuple(NAMES)
    for name, num_conv in NAMES.items():
        cfg = weights.srvgg_config(name)
        assert (cfg.num_conv, cfg.num_feat, cfg.upscale, cfg.scale) == (num_conv, 64, 4, 4)
        assert weights.srvgg_config(name + ".pth") == cfg                 # cut at the first '.'
        with pytest.raises(ValueError, match="SRVGG"):                    # not an RRDBNet: the other table
            weights.realesrgan_config(name)
        layout = weights.srvgg_layout(cfg)
        assert len(layout) == 3 * num_conv + 5
        assert layout[0] == ("body.0.weight", (64, 3, 3, 3)) and layout[1] == ("body.0.bias", (64,))
        assert layout[2] == ("body.1.weight", (64,)) and layout[3] == ("body.2.weight", (64, 64, 3, 3))
        last = 2 * num_conv + 2
        assert layout[-2] == (f"body.{last}.weight", (48, 64, 3, 3)) and layout[-1] == (f"body.{last}.bias", (48,))
        assert last == {16: 34, 32: 66}[num_conv]
        assert f"body.{last + 1}.weight" not in dict(layout)              # no PReLU after the last conv
        sd = weights.make_srvgg_weights(cfg, 0)
        assert weights._srvgg_config_of(sd) == cfg                        # num_conv read from the keys
        assert weights.load_srvgg_state_dict({"params": sd}).keys() == sd.keys()
    for bad in ("RealESRGAN_x4plus", "nope"):
        with pytest.raises(ValueError, match="Unknown Real-ESRGAN SRVGG model"):
            weights.srvgg_config(bad)
    for bad in (dict(num_feat=32), dict(upscale=2), dict(num_conv=0), dict(num_conv=1.5)):
        with pytest.raises(ValueError):
            weights.SRVGGConfig(**{**dict(num_conv=2), **bad})


def test_synthetic_weights_are_seeded_and_survive_the_depth():
    cfg = weights.SRVGGConfig(num_conv=32)
    a, b, other = weights.make_srvgg_weights(cfg, 0), weights.make_srvgg_weights(cfg, 0), weights.make_srvgg_weights(cfg, 1)
    assert list(a) == [k for k, _ in weights.srvgg_layout(cfg)]
    for key, shape in weights.srvgg_layout(cfg):
        assert tuple(a[key].shape) == shape and a[key].dtype == torch.float32
        assert torch.equal(a[key], b[key]) and not torch.equal(a[key], other[key])
        if key.endswith(".bias"):
            assert a[key].abs().min() > 0
        if len(shape) == 1 and not key.endswith(".bias"):     # slopes: per channel, negative and above one among them
            assert a[key].unique().numel() > 32 and float(a[key].min()) < 0 and float(a[key].max()) > 1
    # activations neither die nor blow up on the way through 33 layers
    frame = torch.randint(0, 256, (1, 12, 16, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    x = frame.permute(0, 3, 1, 2).double() / 255.0
    for i in range(33):
        z = F.conv2d(x, a[f"body.{2 * i}.weight"].double(), a[f"body.{2 * i}.bias"].double(), padding=1)
        x = torch.where(z > 0, z, a[f"body.{2 * i + 1}.weight"].double()[None, :, None, None] * z)
    assert 0.1 < float(x.pow(2).mean().sqrt()) < 10.0
    out = R.srvgg_ref(a, 32, frame)
    assert out.shape == (1, 3, 48, 64) and 0.01 < float((out - R.nearest4(frame.permute(0, 3, 1, 2).double() / 255.0)).std()) < 1.0


def test_state_dict_unwrapping_and_validation(tmp_path):
    cfg = weights.SRVGGConfig(num_conv=2)
    sd = weights.make_srvgg_weights(cfg, 3)
    for wrapped in (sd, {"params": sd}, {"params_ema": sd}, {"params": {"junk": torch.zeros(1)}, "params_ema": sd}):
        got = weights.load_srvgg_state_dict(wrapped)
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    got = weights.load_srvgg_state_dict({"params_ema": {k: v.half() for k, v in sd.items()}}, cfg)
    assert all(v.dtype == torch.float32 for v in got.values())
    path = tmp_path / "m.pth"
    torch.save({"params": sd}, path)
    got = weights.load_srvgg_state_dict(str(path), cfg)
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    with pytest.raises(ValueError, match=r"missing key 'body\.3\.weight'"):
        weights.load_srvgg_state_dict({k: v for k, v in sd.items() if k != "body.3.weight"}, cfg)
    with pytest.raises(ValueError, match=r"unexpected key 'body\.7\.weight'"):
        weights.load_srvgg_state_dict({**sd, "body.7.weight": torch.zeros(64)}, cfg)
    with pytest.raises(ValueError, match=r"'body\.6\.weight' has shape \(3, 64, 3, 3\), expected \(48, 64, 3, 3\)"):
        weights.load_srvgg_state_dict({**sd, "body.6.weight": torch.zeros(3, 64, 3, 3)}, cfg)
    with pytest.raises(ValueError, match=r"'body\.6\.weight' has shape \(48, 64, 3, 3\), expected \(64, 64, 3, 3\)"):   # a 3-conv model asked for
        weights.load_srvgg_state_dict(sd, weights.SRVGGConfig(num_conv=3))
    with pytest.raises(ValueError, match="not an SRVGGNetCompact"):
        weights.load_srvgg_state_dict(weights.make_rrdbnet_weights(weights.RRDBNetConfig(4, 1), 0))
    with pytest.raises(ValueError, match="expected a dict"):
        weights.load_srvgg_state_dict([1, 2])


def test_deep_network_interpolation():
    cfg = weights.SRVGGConfig(num_conv=2)
    a, b = weights.make_srvgg_weights(cfg, 0), weights.make_srvgg_weights(cfg, 1)
    one, zero, mid = (weights.dni_state_dicts(a, b, s) for s in (1.0, 0.0, 0.3))
    for k in a:
        assert torch.equal(one[k], a[k]) and torch.equal(zero[k], b[k])
        want = 0.3 * a[k] + (1 - 0.3) * b[k]                              # the fp32 expression, bit for bit
        assert mid[k].dtype == torch.float32 and torch.equal(mid[k].view(torch.int32), want.view(torch.int32))
        assert not torch.equal(mid[k], a[k]) and not torch.equal(mid[k], b[k])
    with pytest.raises(ValueError, match="differ in their keys"):
        weights.dni_state_dicts(a, {k: v for k, v in b.items() if k != "body.1.weight"}, 0.3)
    for s in (1.5, -0.1):
        with pytest.raises(ValueError, match="outside"):
            weights.dni_state_dicts(a, b, s)


# ----------------------------------------------------------------------------- the getter, before any device
def test_getter_refusals_need_no_gpu(tmp_path):
    with pytest.raises(ValueError, match="denoise_strength"):
        restore.get_realesrgan_upsampler("cuda:0", model_name="RealESRGAN_x4plus", denoise_strength=0.5)
    with pytest.raises(ValueError, match="denoise_strength"):
        restore.get_realesrgan_upsampler("cuda:0", model_name="realesr-animevideov3", denoise_strength=0.5)
    with pytest.raises(ValueError, match="outside"):
        restore.get_realesrgan_upsampler("cuda:0", model_name="realesr-general-x4v3", denoise_strength=1.5)
    for name in NAMES:
        with pytest.raises(ValueError, match="fp32"):
            restore.get_realesrgan_upsampler("cuda:0", model_name=name, fp32=True)
        with pytest.raises(ValueError, match="pre_pad"):
            restore.get_realesrgan_upsampler("cuda:0", model_name=name, pre_pad=10)
    # one path, and no wdn file beside it: the reference's error and text, raised before a device is asked for
    path = tmp_path / "realesr-general-x4v3.pth"
    torch.save({"params": weights.make_srvgg_weights(weights.SRVGGConfig(32), 0)}, path)
    with pytest.raises(RuntimeError, match=r"^Unable to locate realesr-general-wdn-x4v3 weights for DNI upsampling\.$"):
        restore.get_realesrgan_upsampler("cuda:0", model_name="realesr-general-x4v3.pth", denoise_strength=0.3, model_path=str(path))
    with pytest.raises(ValueError, match="pair"):
        restore.get_realesrgan_upsampler("cuda:0", model_name="realesr-general-x4v3", denoise_strength=0.3, state_dict={})
    # the checker the drivers call: compatible without a name, and with one it returns the configuration
    assert restore._check_realesrgan_args(1.0, 0, False) is None
    with pytest.raises(ValueError, match="denoise_strength"):
        restore._check_realesrgan_args(0.5, 0, False)
    assert restore._check_realesrgan_args(0.3, 0, False, "realesr-general-x4v3") == weights.SRVGGConfig(32)
    assert restore._check_realesrgan_args(1.0 + 1e-12, 0, False, "RealESRGAN_x2plus.pth") == weights.RRDBNetConfig(2, 23)
    src = tmp_path / "in"
    src.mkdir()
    with pytest.raises(ValueError, match="denoise_strength"):
        drivers.restore_downsampled_with_realesrgan(str(src), str(tmp_path / "o"), np.zeros((1, 1, 1)), 8,
                                                    model_name="realesr-animevideov3", denoise_strength=0.5)
    with pytest.raises(ValueError, match="No frames found"):             # the name and the strength pass the checks
        drivers.restore_downsampled_with_realesrgan(str(src), str(tmp_path / "o"), np.zeros((1, 1, 1)), 8,
                                                    model_name="realesr-general-x4v3", denoise_strength=0.5)


# ----------------------------------------------------------------------------- packing
@pytest.mark.parametrize("cin_real,cout_real,cin,cout", [(3, 64, 32, 64), (64, 64, 64, 64), (64, 48, 64, 48), (1, 1, 32, 48),
                                                         (33, 47, 64, 48)])
def test_pack_weights_against_the_numpy_statement(built_lib, cin_real, cout_real, cin, cout):
    h = _lib.lib()
    rng = np.random.default_rng(cin_real * 100 + cout_real)
    w = rng.standard_normal((cout_real, cin_real, 3, 3)).astype(np.float32)
    w.flat[:8] = [65504.0, 65520.0, -1e-8, 2.0 ** -25, 2.0 ** -25 * 1.0001, 6.0e-5, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11][:min(8, w.size)]
    assert h.elvis_srvgg_packed_weight_bytes(cin, cout) == 9 * cin * cout * 2
    packed = np.full(9 * cin * cout, 0x7e00, dtype=np.uint16)
    assert h.elvis_srvgg_pack_weights(w.ctypes.data_as(C.c_void_p), cin_real, cout_real, cin, cout, packed.ctypes.data_as(C.c_void_p)) == 0
    with np.errstate(over="ignore"):
        want = R.pack_ref(w, cin, cout)
    got = packed.view(np.float16).reshape(want.shape)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    # the padding is zero: input channels past cin_real, output channels past cout_real
    full = got.transpose(2, 0, 3, 1).reshape(cout, cin, 9)
    assert not full[cout_real:].any() and not full[:, cin_real:].any()


def test_entry_point_argument_checks(built_lib):
    h = _lib.lib()
    assert "srvgg.hip" in _build.SOURCES
    header = open(os.path.join(ROOT, "include", "elvis_amd.h")).read()
    for name, nargs in (("elvis_srvgg_packed_weight_bytes", 2), ("elvis_srvgg_pack_weights", 6), ("elvis_srvgg_conv3x3", 12),
                        ("elvis_srvgg_tail", 13)):
        m = re.search(r"(?:int|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]) and hasattr(h, name)
        comment = header[header.rfind("/*", 0, m.start()):m.start()]
        assert "elvis.py:2431-2441" in comment and "2515" in comment
    assert h.elvis_srvgg_packed_weight_bytes(96, 64) == 0 and h.elvis_srvgg_packed_weight_bytes(64, 32) == 0
    buf = np.zeros(9 * 32 * 48, np.uint16)
    w = np.zeros((48, 32, 3, 3), np.float32)
    wp, bp = w.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)
    assert h.elvis_srvgg_pack_weights(wp, 32, 48, 40, 48, bp) == -1 and b"cin=40" in h.elvis_last_error()
    assert h.elvis_srvgg_pack_weights(wp, 32, 48, 32, 32, bp) == -1 and b"cout=32" in h.elvis_last_error()
    assert h.elvis_srvgg_pack_weights(wp, 33, 48, 32, 48, bp) == -1 and b"do not fit" in h.elvis_last_error()
    assert h.elvis_srvgg_pack_weights(wp, 32, 0, 32, 48, bp) == -1 and b"do not fit" in h.elvis_last_error()
    assert h.elvis_srvgg_pack_weights(None, 32, 48, 32, 48, bp) == -1 and b"null" in h.elvis_last_error()
    before = h.elvis_last_launch()

    def conv(x=4096, x_pitch=64, wgt=8192, bias=8192, slope=8192, out=1 << 20, out_pitch=64, n=1, hh=4, ww=4, cin=64):
        return h.elvis_srvgg_conv3x3(x, x_pitch, wgt, bias, slope, out, out_pitch, n, hh, ww, cin, None)

    # every check comes before any launch: the pointers above are never touched
    assert conv(cin=48) == -1 and b"cin=48" in h.elvis_last_error()
    assert h.elvis_last_error().startswith(b"elvis_srvgg_conv3x3")
    assert conv(cin=96) == -1 and b"cin=96" in h.elvis_last_error()
    assert conv(x_pitch=60) == -1 and b"x_pitch" in h.elvis_last_error()
    assert conv(x_pitch=32) == -1 and b"x_pitch" in h.elvis_last_error()
    assert conv(out_pitch=48) == -1 and b"out_pitch" in h.elvis_last_error()
    assert conv(out_pitch=68) == -1 and b"out_pitch" in h.elvis_last_error()
    assert conv(n=-1) == -1 and b"bad shape" in h.elvis_last_error()
    assert conv(hh=(1 << 29) + 1) == -1 and b"too large" in h.elvis_last_error()
    for null in ("x", "wgt", "bias", "slope", "out"):
        assert conv(**{null: None}) == -1 and b"null" in h.elvis_last_error()
    assert conv(x=4100) == -1 and b"aligned" in h.elvis_last_error()
    assert conv(slope=8196) == -1 and b"aligned" in h.elvis_last_error()
    assert conv(out=(1 << 20) + 4) == -1 and b"aligned" in h.elvis_last_error()
    assert conv(out=4096) == -1 and b"overlaps x" in h.elvis_last_error()                    # in place
    assert conv(out=4096 + 16 * 64 * 2 - 8) == -1 and b"overlaps x" in h.elvis_last_error()  # the last 8 bytes of x
    assert conv(x=(1 << 20) + 16 * 64 * 2 - 16) == -1 and b"overlaps x" in h.elvis_last_error()
    assert conv(n=70000, out=1 << 40) == -1 and b"more than one launch" in h.elvis_last_error()
    assert conv(n=0, x=None, out=None) == 0 and conv(hh=0, x=None) == 0 and conv(ww=0, slope=None) == 0

    def tail(x=4096, x_pitch=64, wgt=8192, bias=8192, base=1 << 16, base_pitch=32, out=1 << 20, n=1, hh=4, ww=4, u8=1):
        return h.elvis_srvgg_tail(x, x_pitch, wgt, bias, base, base_pitch, out, n, hh, ww, u8, 0, None)

    assert tail(x_pitch=60) == -1 and b"x_pitch" in h.elvis_last_error()
    assert h.elvis_last_error().startswith(b"elvis_srvgg_tail")
    assert tail(x_pitch=32) == -1 and b"x_pitch" in h.elvis_last_error()
    assert tail(base_pitch=2) == -1 and b"base_pitch" in h.elvis_last_error()
    assert tail(ww=-1) == -1 and b"bad shape" in h.elvis_last_error()
    assert tail(ww=(1 << 27) + 1) == -1 and b"too large" in h.elvis_last_error()
    for null in ("x", "wgt", "bias", "base", "out"):
        assert tail(**{null: None}) == -1 and b"null" in h.elvis_last_error()
    assert tail(wgt=8200) == -1 and b"aligned" in h.elvis_last_error()
    assert tail(base=(1 << 16) + 1) == -1 and b"aligned" in h.elvis_last_error()
    assert tail(out=(1 << 20) + 2) == -1 and b"aligned" in h.elvis_last_error()
    assert tail(out=(1 << 20) + 4, u8=0) == -1 and b"aligned" in h.elvis_last_error()       # f16 out: 8 bytes
    assert tail(out=4096 + 16) == -1 and b"overlaps x" in h.elvis_last_error()
    assert tail(out=(1 << 16) + 16 * 32 * 2 - 4) == -1 and b"overlaps base" in h.elvis_last_error()
    assert tail(base=(1 << 20) + 16 * 48 - 2) == -1 and b"overlaps base" in h.elvis_last_error()   # the last byte pair of a u8 out
    assert tail(n=0, x=None, out=None) == 0 and tail(hh=0, base=None) == 0
    assert h.elvis_last_launch() == before                               # nothing was launched by any of the above


# ----------------------------------------------------------------------------- the statement itself
def test_pixel_shuffle_order_of_the_statement():
    """`shuffle4` puts channel 16c + 4dy + dx at (c, 4y + dy, 4x + dx): torch's pixel_shuffle, checked by position."""
    n, h, w = 2, 3, 5
    z = torch.zeros((n, 48, h, w), dtype=torch.float64)
    for ch in range(48):
        for y in range(h):
            for x in range(w):
                z[:, ch, y, x] = 10000 * ch + 100 * y + x                 # encodes (channel, y, x)
    z[1] += 0.5
    out = R.shuffle4(z)
    assert out.shape == (n, 3, 4 * h, 4 * w)
    for c in range(3):
        for Y in range(4 * h):
            for X in range(4 * w):
                assert float(out[0, c, Y, X]) == 10000 * (16 * c + 4 * (Y % 4) + X % 4) + 100 * (Y // 4) + X // 4
    assert torch.equal(out, F.pixel_shuffle(z, 4))
    base = torch.arange(n * 3 * h * w, dtype=torch.float64).reshape(n, 3, h, w)
    assert torch.equal(R.nearest4(base), F.interpolate(base, scale_factor=4, mode="nearest"))
    # the tail statement is the conv, this shuffle and this base
    g = torch.Generator().manual_seed(4)
    wt, b = torch.randn((48, 64, 3, 3), generator=g) * 0.05, torch.randn(48, generator=g)
    x = torch.randn((n, 64, h, w), generator=g).half().double()
    want = F.pixel_shuffle(F.conv2d(x, wt.half().double(), b.double(), padding=1), 4) + F.interpolate(base, scale_factor=4, mode="nearest")
    assert torch.allclose(R.tail_ref(x, wt, b, base).ref, want, rtol=0, atol=1e-12)


def test_u8_cases_are_mostly_decided_by_the_reference():
    """The inputs of the u8 device cases (tests/test_gpu_srvgg.py), from the float64 reference alone: under 2 % of a
    case lies within 255 e8 of a half-integer (where the byte may differ by one), both clamps are reached and the bytes
    0 and 255 occur."""
    for h, w, n, swap, base_pitch in R.U8_CASES:
        wt, b, x_h, base_h = R.u8_inputs(h, w, n, swap, base_pitch)
        assert base_h.shape[-1] == base_pitch
        ref = R.tail_ref(R.nchw(x_h), wt, b, R.nchw(base_h)[:, :3])
        byte, near = R.u8_ref(ref)
        share = float(near.double().mean())
        assert share < 0.02, (h, w, share)
        assert bool((ref.ref < 0).any()) and bool((ref.ref > 1).any())
        if h * w > 1:
            assert float((ref.ref < 0).double().mean()) > 0.01 and float((ref.ref > 1).double().mean()) > 0.01
        assert int(byte.min()) == 0 and int(byte.max()) == 255
