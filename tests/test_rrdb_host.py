"""The Real-ESRGAN slot without a GPU: the model-name table, state-dict validation, the host packing against its
numpy statement, the unshuffle order of the reference statement, the argument checks of the two entry points and the
directory driver through a stand-in worker."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _hooks
import _rrdb_ref as R
from elvis_amd import _build, _lib, drivers, frameio, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- names and configurations
def test_model_name_table_and_errors():
    want = {"RealESRGAN_x4plus": (23, 4), "RealESRNet_x4plus": (23, 4), "RealESRGAN_x4plus_anime_6B": (6, 4),
            "RealESRGAN_x2plus": (23, 2)}
    for name, (blocks, scale) in want.items():
        cfg = weights.realesrgan_config(name)
        assert (cfg.num_block, cfg.scale, cfg.num_feat, cfg.num_grow_ch) == (blocks, scale, 64, 32)
        assert weights.realesrgan_config(name + ".pth") == cfg            # cut at the first '.'
    for name in ("realesr-animevideov3", "realesr-general-x4v3"):
        with pytest.raises(ValueError, match="SRVGG"):
            weights.realesrgan_config(name)
    with pytest.raises(ValueError, match="Unknown Real-ESRGAN model: nope"):
        weights.realesrgan_config("nope")
    for bad in (dict(scale=1), dict(scale=8), dict(num_feat=32), dict(num_grow_ch=16), dict(num_block=0)):
        with pytest.raises(ValueError):
            weights.RRDBNetConfig(**{**dict(scale=4, num_block=2), **bad})
    assert weights.RRDBNetConfig(scale=2, num_block=1).in_channels == 12
    assert weights.RRDBNetConfig(scale=4, num_block=1).in_channels == 3


def test_departures_are_value_errors(tmp_path):
    from elvis_amd import restore
    for kw, msg in ((dict(fp32=True), "fp32"), (dict(pre_pad=10), "pre_pad"), (dict(denoise_strength=0.5), "denoise_strength")):
        with pytest.raises(ValueError, match=msg):
            restore.get_realesrgan_upsampler("cuda:0", **kw)
        src = tmp_path / "in"
        src.mkdir(exist_ok=True)
        with pytest.raises(ValueError, match=msg):
            drivers.restore_downsampled_with_realesrgan(str(src), str(tmp_path / "o"), np.zeros((1, 1, 1)), 8, **kw)
    with pytest.raises(ValueError, match="Unknown Real-ESRGAN model"):
        restore.get_realesrgan_upsampler("cuda:0", model_name="ESRGAN_x8")
    import elvis_amd
    for name in ("get_realesrgan_upsampler", "get_realesrgan_upsample_fn", "restore_frames_realesrgan",
                 "restore_frames_realesrgan_device", "restore_with_realesrgan_naive"):
        assert getattr(elvis_amd, name) is getattr(restore, name)
    assert elvis_amd.restore_downsampled_with_realesrgan is drivers.restore_downsampled_with_realesrgan
    assert "realesrgan" in drivers.YUV_CLIP_KINDS


# ----------------------------------------------------------------------------- state dicts
def test_synthetic_weights_are_seeded_and_scaled():
    cfg = weights.RRDBNetConfig(scale=2, num_block=1)
    a, b = weights.make_rrdbnet_weights(cfg, 0), weights.make_rrdbnet_weights(cfg, 0)
    other = weights.make_rrdbnet_weights(cfg, 1)
    layout = weights.rrdbnet_layout(cfg)
    assert len(layout) == 1 + 15 + 5 and layout[0] == ("conv_first", 64, 12) and layout[-1] == ("conv_last", 3, 64)
    assert [c for k, _, c in layout if k.startswith("body.0.rdb2")] == [64, 96, 128, 160, 192]
    assert len(weights.rrdbnet_layout(weights.RRDBNetConfig(4, 23))) == 351
    for key, cout, cin in layout:
        w = a[key + ".weight"]
        assert tuple(w.shape) == (cout, cin, 3, 3) and torch.equal(w, b[key + ".weight"])
        assert not torch.equal(w, other[key + ".weight"])
        assert not a[key + ".bias"].any()
        if w.numel() >= 9 * 64 * 32:       # std 0.1 * sqrt(2 / fan_in), within sampling error
            assert abs(float(w.std()) / (0.1 * (2.0 / (cin * 9)) ** 0.5) - 1.0) < 0.05


def test_state_dict_unwrapping_and_validation(tmp_path):
    cfg = weights.RRDBNetConfig(scale=4, num_block=2)
    sd = weights.make_rrdbnet_weights(cfg, 3)
    for wrapped in (sd, {"params": sd}, {"params_ema": sd}, {"params": {"junk": torch.zeros(1)}, "params_ema": sd}):
        got = weights.load_realesrgan_state_dict(wrapped)
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    got = weights.load_realesrgan_state_dict({"params_ema": {k: v.half() for k, v in sd.items()}}, cfg)
    assert all(v.dtype == torch.float32 for v in got.values())
    path = tmp_path / "m.pth"
    torch.save({"params_ema": sd}, path)
    got = weights.load_realesrgan_state_dict(str(path), cfg)
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    x2 = weights.make_rrdbnet_weights(weights.RRDBNetConfig(scale=2, num_block=1), 0)
    assert weights.load_realesrgan_state_dict(x2)["conv_first.weight"].shape[1] == 12       # scale read from the keys
    missing = {k: v for k, v in sd.items() if k != "body.1.rdb2.conv3.bias"}
    with pytest.raises(ValueError, match=r"missing key 'body\.1\.rdb2\.conv3\.bias'"):
        weights.load_realesrgan_state_dict(missing, cfg)
    with pytest.raises(ValueError, match=r"unexpected key 'conv_extra\.weight'"):
        weights.load_realesrgan_state_dict({**sd, "conv_extra.weight": torch.zeros(1)}, cfg)
    with pytest.raises(ValueError, match=r"'conv_up1\.weight' has shape \(64, 32, 3, 3\), expected \(64, 64, 3, 3\)"):
        weights.load_realesrgan_state_dict({**sd, "conv_up1.weight": torch.zeros(64, 32, 3, 3)}, cfg)
    with pytest.raises(ValueError, match=r"missing key 'body\.2\.rdb1\.conv1\.weight'"):       # a 3-block model asked for
        weights.load_realesrgan_state_dict(sd, weights.RRDBNetConfig(scale=4, num_block=3))
    with pytest.raises(ValueError, match="conv_first.weight"):
        weights.load_realesrgan_state_dict({**sd, "conv_first.weight": torch.zeros(64, 48, 3, 3)})
    with pytest.raises(ValueError, match="expected a dict"):
        weights.load_realesrgan_state_dict([1, 2])


# ----------------------------------------------------------------------------- packing
@pytest.mark.parametrize("cin_real,cout_real,cin,cout", [(3, 64, 32, 64), (12, 64, 32, 64), (64, 3, 64, 32), (96, 32, 96, 32),
                                                         (192, 64, 192, 64), (1, 1, 32, 32)])
def test_pack_weights_against_the_numpy_statement(built_lib, cin_real, cout_real, cin, cout):
    h = _lib.lib()
    rng = np.random.default_rng(cin_real * 100 + cout_real)
    w = rng.standard_normal((cout_real, cin_real, 3, 3)).astype(np.float32)
    w.flat[:8] = [65504.0, 65520.0, -1e-8, 2.0 ** -25, 2.0 ** -25 * 1.0001, 6.0e-5, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11][:min(8, w.size)]
    assert h.elvis_rrdb_packed_weight_bytes(cin, cout) == 9 * cin * cout * 2
    packed = np.full(9 * cin * cout, 0x7e00, dtype=np.uint16)
    assert h.elvis_rrdb_pack_weights(w.ctypes.data_as(C.c_void_p), cin_real, cout_real, cin, cout, packed.ctypes.data_as(C.c_void_p)) == 0
    with np.errstate(over="ignore"):
        want = R.pack_ref(w, cin, cout)
    got = packed.view(np.float16).reshape(want.shape)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    # the padding is zero: input channels past cin_real, output channels past cout_real
    full = got.transpose(2, 0, 3, 1).reshape(cout, cin, 9)
    assert not full[cout_real:].any() and not full[:, cin_real:].any()


def test_pack_and_entry_point_argument_checks(built_lib):
    h = _lib.lib()
    assert "rrdb.hip" in _build.SOURCES
    header = open(os.path.join(ROOT, "include", "elvis_amd.h")).read()
    for name, nargs in (("elvis_rrdb_packed_weight_bytes", 2), ("elvis_rrdb_pack_weights", 6), ("elvis_rrdb_conv3x3", 23),
                        ("elvis_rrdb_input_u8", 8)):
        m = re.search(r"(?:int|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]) and hasattr(h, name)
        assert "elvis.py:2515" in header[header.rfind("/*", 0, m.start()):m.start()]
    assert h.elvis_rrdb_packed_weight_bytes(48, 32) == 0 and h.elvis_rrdb_packed_weight_bytes(64, 16) == 0
    buf = np.zeros(9 * 32 * 32, np.uint16)
    w = np.zeros((32, 32, 3, 3), np.float32)
    wp, bp = w.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)
    assert h.elvis_rrdb_pack_weights(wp, 32, 32, 40, 32, bp) == -1 and b"cin=40" in h.elvis_last_error()
    assert h.elvis_rrdb_pack_weights(wp, 33, 32, 32, 32, bp) == -1 and b"do not fit" in h.elvis_last_error()
    assert h.elvis_rrdb_pack_weights(None, 32, 32, 32, 32, bp) == -1 and b"null" in h.elvis_last_error()

    def conv(x=4096, x_pitch=64, wgt=8192, bias=8192, out=1 << 20, out_pitch=64, out_coff=0, r1=None, r1_pitch=0, r2=None,
             r2_pitch=0, n=1, hh=4, ww=4, cin=64, cout=32, ups=0, lrelu=0, out_u8=0):
        return h.elvis_rrdb_conv3x3(x, x_pitch, wgt, bias, out, out_pitch, out_coff, r1, r1_pitch, r2, r2_pitch, n, hh, ww,
                                    cin, cout, ups, lrelu, 1.0, 0.0, out_u8, 0, None)

    # every check comes before any launch: the pointers above are never touched
    assert conv(cin=48) == -1 and b"cin=48" in h.elvis_last_error()
    assert h.elvis_last_error().startswith(b"elvis_rrdb_conv3x3")
    assert conv(cout=16) == -1 and b"cout=16" in h.elvis_last_error()
    assert conv(x_pitch=60) == -1 and b"x_pitch" in h.elvis_last_error()
    assert conv(out_pitch=48, out_coff=32) == -1 and b"do not fit" in h.elvis_last_error()
    assert conv(cout=64, out_u8=1) == -1 and b"out_u8" in h.elvis_last_error()
    assert conv(n=-1) == -1 and b"bad shape" in h.elvis_last_error()
    assert conv(x=None) == -1 and b"null" in h.elvis_last_error()
    assert conv(x=4100) == -1 and b"aligned" in h.elvis_last_error()
    assert conv(r1=1 << 21, r1_pitch=16) == -1 and b"r1_pitch" in h.elvis_last_error()
    # the in-place concat: the same buffer, channels [64, 96) written and [0, 64) read is accepted up to the launch;
    # an overlapping range is refused
    assert conv(out=4096, x_pitch=96, out_pitch=96, out_coff=32) == -1 and b"overlaps x" in h.elvis_last_error()
    assert conv(out=4096, x_pitch=96, out_pitch=96, out_coff=64, ups=1) == -1 and b"overlaps x" in h.elvis_last_error()
    assert conv(out=4096 + 64, x_pitch=96, out_pitch=96, out_coff=64) == -1 and b"overlaps x" in h.elvis_last_error()
    assert conv(out=4096, out_pitch=3, out_u8=1) == -1 and b"overlaps x" in h.elvis_last_error()
    # a residual inside out: element for element or on other channels only
    assert conv(out_pitch=96, out_coff=16, r2=1 << 20, r2_pitch=96) == -1 and b"r2 overlaps out" in h.elvis_last_error()
    assert conv(r1=(1 << 20) + 8, r1_pitch=64) == -1 and b"r1 overlaps out" in h.elvis_last_error()
    assert conv(n=0, x=None, out=None) == 0 and conv(hh=0, x=None) == 0

    def inp(src=4096, dst=8192, n=1, hh=4, ww=4, s=1):
        return h.elvis_rrdb_input_u8(src, dst, n, hh, ww, s, 0, None)

    assert inp(s=3) == -1 and b"s=3" in h.elvis_last_error()
    assert inp(hh=-1) == -1 and b"bad shape" in h.elvis_last_error()
    assert inp(hh=1, s=2) == -1 and b"reflected" in h.elvis_last_error()
    assert inp(src=None) == -1 and b"null" in h.elvis_last_error()
    assert inp(dst=8200) == -1 and b"aligned" in h.elvis_last_error()
    assert inp(n=0, src=None, dst=None) == 0


def test_unshuffle_order_of_the_statement():
    """`input_ref` puts input (c, 2y+sy, 2x+sx) at channel 4c + 2sy + sx: torch's pixel_unshuffle, checked by position."""
    n, h, w = 1, 4, 6
    img = torch.zeros((n, h, w, 3), dtype=torch.uint8)
    for c in range(3):
        for y in range(h):
            for x in range(w):
                img[0, y, x, c] = 10 * c + 4 * (y % 2) + 2 * (x % 2) + 1      # encodes (c, sy, sx)
    out = R.input_ref(img, 2, False)
    assert out.shape == (1, 2, 3, 32)
    for c in range(3):
        for sy in range(2):
            for sx in range(2):
                want = np.float16(np.float32(10 * c + 4 * sy + 2 * sx + 1) / np.float32(255.0))
                assert (out[0, :, :, 4 * c + 2 * sy + sx].numpy() == want).all()
    assert not out[..., 12:].any()
    ref = F.pixel_unshuffle(img.permute(0, 3, 1, 2).float(), 2)
    assert torch.equal(out[..., :12].permute(0, 3, 1, 2).float(), (ref / np.float32(255.0)).half().float())
    # an odd size: one reflected row and column (index h reads h - 2)
    odd = torch.arange(5 * 7 * 3, dtype=torch.uint8).reshape(1, 5, 7, 3)
    o = R.input_ref(odd, 2, True)
    assert o.shape == (1, 3, 4, 32)
    assert float(o[0, 2, 3, 4 * 0 + 2 * 1 + 1]) == float(np.float16(np.float32(int(odd[0, 3, 5, 2])) / np.float32(255.0)))


def test_out_u8_cases_are_mostly_decided_by_the_reference():
    """The inputs of the out_u8 device cases (tests/test_gpu_rrdb.py), from the float64 reference alone: under 2 % of a
    case lies within 255 e of a half-integer (where the byte may differ by one), and both clamps are reached."""
    for cin, h, w, n, swap, res in R.U8_CASES:
        wt, b, x_h, r1_h, r2_h = R.u8_inputs(cin, h, w, n, swap, res)
        ref = R.conv_ref(R.nchw(x_h), wt, b, s0=1.0, s1=0.5, r1=None if r1_h is None else R.nchw(r1_h)[:, :3],
                         r2=None if r2_h is None else R.nchw(r2_h)[:, :3])
        byte, near = R.u8_ref(ref)
        assert float(near.double().mean()) < 0.02
        assert float((ref.ref < 0).double().mean()) > 0.01 and float((ref.ref > 1).double().mean()) > 0.01
        assert int(byte.min()) == 0 and int(byte.max()) == 255


# ----------------------------------------------------------------------------- the directory driver
def test_realesrgan_driver_files_and_errors(tmp_path):
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, size=(16, 24, 3), dtype=np.uint8) for _ in range(4)]
    for i, f in enumerate(frames):
        frameio.save_frame(f, src / f"{i + 1:05d}.png")
    maps = np.zeros((4, 2, 3), np.uint8)
    maps[[1, 2]] = 1
    (dst / "stale").mkdir(parents=True)
    frameio.save_frame(frames[0], dst / "99999.png")          # cleared before writing (elvis.py:2716)
    drivers.restore_downsampled_with_realesrgan(str(src), str(dst), maps, 8, devices=["cpu"], model_name="RealESRGAN_x2plus",
                                                tile=400, tile_pad=5, _shard_fn=_hooks.plus_device_tag)
    assert sorted(p.name for p in frameio.get_frame_paths(dst)) == [f"{i + 1:05d}.png" for i in range(4)]
    for i, f in enumerate(frames):
        want = _hooks.plus_device_tag([f], maps[i:i + 1], 8, None, i)[0]
        assert np.array_equal(frameio.load_frame(dst / f"{i + 1:05d}.png"), want)
        assert np.array_equal(frameio.load_frame(src / f"{i + 1:05d}.png"), f)
    with pytest.raises(ValueError, match="does not match frame count"):
        drivers.restore_downsampled_with_realesrgan(str(src), str(dst), maps[:3], 8, devices=["cpu"], _shard_fn=_hooks.plus_device_tag)
    with pytest.raises(ValueError, match="does not match frame count"):
        drivers.restore_downsampled_with_realesrgan(str(src), str(dst), maps[0], 8, devices=["cpu"], _shard_fn=_hooks.plus_device_tag)
    with pytest.raises(ValueError, match="No frames found"):
        drivers.restore_downsampled_with_realesrgan(str(tmp_path / "empty"), str(dst), maps, 8, devices=["cpu"],
                                                    _shard_fn=_hooks.plus_device_tag)
    with pytest.raises(ValueError, match="png_writer"):
        drivers.restore_downsampled_with_realesrgan(str(src), str(dst), maps, 8, png_writer="cv2", _shard_fn=_hooks.plus_device_tag)
    if not torch.cuda.is_available():                  # the product path has no CPU fallback
        with pytest.raises((RuntimeError, ValueError)):
            drivers.restore_downsampled_with_realesrgan(str(src), str(dst), maps, 8)
