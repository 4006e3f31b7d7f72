"""The encoder hand-off on the device (csrc/handoff.hip, elvis_amd/handoff.py) against tests/_handoff_ref.py: exact equality
everywhere.  A lane takes a strip of 8 pixels of a row pair, so the widths are: 2, 6, 10, 18, 62, 66, 130 (`w % 4 == 2`: no
dword rows, the byte path), 8, 16, 64 (whole dword strips), 504, 512, 520 (one strip less than a wave's 64, exactly 64,
one more), and - added to the requested matrix - 4, 12, 20, 36 (`w % 8 == 4`: dword rows whose chroma rows start off a
dword, and a 4-pixel tail strip beside dword strips).  Every frame here is narrower than a workgroup's 256 strips, so a
wave wraps from one row pair to the next and from one frame to the next; 2 x 18 x 130 needs more than one workgroup."""
import os

import numpy as np
import pytest
import torch

import _handoff_ref as R
import _presley_degrade_ref as PR

pytestmark = pytest.mark.gpu

HEIGHTS = (2, 4, 6, 18)
WIDTHS = (2, 6, 8, 10, 16, 18, 62, 64, 66, 130, 504, 512, 520, 4, 12, 20, 36)
SENTINEL, GUARD = 0xA5, 64


def _frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _guarded(dev, shape, lead=GUARD):
    """A sentinel-filled `out` of `shape` inside a larger buffer, `lead` bytes in."""
    size = int(np.prod(shape))
    buf = torch.full((lead + size + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    return buf, buf[lead:lead + size].view(shape)


def _guards_intact(buf, lead=GUARD):
    host = buf.cpu().numpy()
    return bool((host[:lead] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all())


@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("h", HEIGHTS)
def test_shape_matrix(gpu_device, h, order):
    from elvis_amd import handoff
    for w in WIDTHS:
        frames = _frames(2, h, w, 1000 * h + w)
        want = R.rgb_to_i420(frames, order)
        src = torch.from_numpy(frames).to(gpu_device)
        got = handoff.rgb_to_i420_device(src, order)
        assert got.shape == (2, h * 3 // 2, w) and got.dtype == torch.uint8 and got.is_contiguous()
        assert np.array_equal(got.cpu().numpy(), want), (h, w, order)
        buf, out = _guarded(gpu_device, (2, h * 3 // 2, w))
        back = handoff.rgb_to_i420_device(src, order, out=out)
        assert back is out and np.array_equal(out.cpu().numpy(), want), (h, w, order, "out=")
        assert _guards_intact(buf), (h, w, order)
        assert np.array_equal(src.cpu().numpy(), frames)


@pytest.mark.parametrize("w", [8, 16, 36, 130])
def test_unaligned_pointers_take_the_byte_path(gpu_device, w):
    """A source or an output that does not start on a dword (a view into a larger tensor) is converted byte by byte."""
    from elvis_amd import handoff
    h = 6
    frames = _frames(2, h, w, w)
    want = R.rgb_to_i420(frames)
    for src_lead, out_lead in ((0, 61), (3, 64), (1, 62)):
        sbuf = torch.full((src_lead + frames.size + GUARD,), SENTINEL, dtype=torch.uint8, device=gpu_device)
        src = sbuf[src_lead:src_lead + frames.size].view(frames.shape)
        src.copy_(torch.from_numpy(frames).to(gpu_device))
        buf, out = _guarded(gpu_device, want.shape, out_lead)
        handoff.rgb_to_i420_device(src, out=out)
        assert np.array_equal(out.cpu().numpy(), want), (w, src_lead, out_lead)
        assert _guards_intact(buf, out_lead) and np.array_equal(src.cpu().numpy(), frames)


def test_every_colour(gpu_device):
    """The 4096 x 4096 frame whose pixel i is colour i, rolled by (ky, kx) in {0, 1}^2, one frame per launch: Y, U and V
    of all four, so every colour is converted to Y four times and sits on an even / even site exactly once."""
    from elvis_amd import handoff
    side = 4096
    c = np.arange(side * side, dtype=np.int32).reshape(side, side)
    base = np.stack([c >> 16, (c >> 8) & 255, c & 255], axis=-1).astype(np.uint8)
    y, u, v = (p.astype(np.uint8) for p in R.yuv_of(base))
    out = torch.empty((1, side * 3 // 2, side), dtype=torch.uint8, device=gpu_device)
    for ky in (0, 1):
        for kx in (0, 1):
            frame = np.roll(base, (ky, kx), axis=(0, 1))
            got = handoff.rgb_to_i420_device(torch.from_numpy(frame[None]).to(gpu_device), out=out)[0].cpu().numpy()
            ry, ru, rv = (np.roll(p, (ky, kx), axis=(0, 1)) for p in (y, u, v))
            assert np.array_equal(got[:side], ry), (ky, kx, "Y")
            assert np.array_equal(got[side:side * 5 // 4].reshape(side // 2, side // 2), ru[::2, ::2]), (ky, kx, "U")
            assert np.array_equal(got[side * 5 // 4:].reshape(side // 2, side // 2), rv[::2, ::2]), (ky, kx, "V")
    # pixel (r, q) moves to (r + ky, q + kx): it is on an even / even site for exactly one of the four (ky, kx)
    # the restatement's own word on one rolled frame, planes and layout included
    small = np.roll(base, (1, 1), axis=(0, 1))[:64, :130]
    assert np.array_equal(handoff.rgb_to_i420_device(torch.from_numpy(np.ascontiguousarray(small[None])).to(gpu_device))[0].cpu().numpy(),
                          R.rgb_to_i420(np.ascontiguousarray(small[None]))[0])


def test_chroma_is_not_averaged(gpu_device):
    from elvis_amd import handoff
    h, w = 18, 66
    frames = _frames(2, h, w, 5)
    other = _frames(2, h, w, 6)
    other[:, ::2, ::2] = frames[:, ::2, ::2]                    # only the three non-sampled pixels of every quad differ
    a = handoff.rgb_to_i420_device(torch.from_numpy(frames).to(gpu_device)).cpu().numpy()
    b = handoff.rgb_to_i420_device(torch.from_numpy(other).to(gpu_device)).cpu().numpy()
    assert np.array_equal(a[:, h:], b[:, h:])
    assert not np.array_equal(a[:, :h], b[:, :h]) and np.array_equal(a[:, :h:2, ::2], b[:, :h:2, ::2])


def test_surface_bytes_do_not_depend_on_the_chunk(gpu_device, tmp_path, golden_dir):
    from elvis_amd import handoff
    frames = list(_frames(5, 18, 34, 7))
    want_raw, want_y4m = R.yuv420p_bytes(frames), R.y4m_bytes(frames, 29.97)
    for chunk in (1, 2, len(frames), None):
        assert handoff.convert_frames_to_yuv420p(frames, gpu_device, chunk_frames=chunk) == want_raw, chunk
        path = str(tmp_path / f"clip_{chunk}.y4m")
        handoff.write_y4m(frames, path, 29.97, gpu_device, chunk_frames=chunk)
        assert open(path, "rb").read() == want_y4m, chunk
    assert handoff.convert_frames_to_yuv420p([], gpu_device) == b""
    # a batch equals its frames one by one
    batch = handoff.rgb_to_i420_device(torch.from_numpy(np.stack(frames)).to(gpu_device)).cpu().numpy()
    for i, f in enumerate(frames):
        assert np.array_equal(handoff.rgb_to_i420_device(torch.from_numpy(f[None]).to(gpu_device))[0].cpu().numpy(), batch[i])
    # and the reference's own write_y4m framing (tests/golden/handoff.npz), default device
    g = np.load(os.path.join(golden_dir, "handoff.npz"))
    path, pos = str(tmp_path / "golden.y4m"), 0
    for rate, size in zip(g["y4m_framerates"], g["y4m_sizes"]):
        handoff.write_y4m(list(g["y4m_frames"]), path, float(rate))
        assert open(path, "rb").read() == g["y4m_files"][pos:pos + size].tobytes()
        pos += size


def test_degraded_clip_goes_straight_to_i420(gpu_device):
    """`degrade_scale_device`'s output handed to `rgb_to_i420_device` with no host copy equals the restatement of both."""
    from elvis_amd import degrade, handoff
    b, h, w = 8, 34, 52                                          # a ragged edge on both axes
    frames = _frames(3, h, w, 11)
    scales = np.random.default_rng(12).choice(np.asarray([0, 2, 3, 4], np.int32), size=(3, h // b, w // b)).astype(np.int32)
    degraded = degrade.degrade_scale_device(torch.from_numpy(frames).to(gpu_device), torch.from_numpy(scales).to(gpu_device), b)
    got = handoff.rgb_to_i420_device(degraded).cpu().numpy()
    assert np.array_equal(got, R.rgb_to_i420(PR.scale_clip(frames, scales, b)))


def test_errors_come_before_any_launch(gpu_device):
    from elvis_amd import _lib, handoff
    dev = gpu_device

    def t(*shape, dtype=torch.uint8):
        return torch.zeros(shape, dtype=dtype, device=dev)

    good = t(2, 4, 6, 3)
    handoff.rgb_to_i420_device(good, "bgr")                      # every call below would launch the rgb instantiation
    assert _lib.lib().elvis_last_launch() == b"rgb_to_i420_kernel<bgr>"
    bad_calls = [
        lambda: handoff.rgb_to_i420_device(t(1, 3, 4, 3)), lambda: handoff.rgb_to_i420_device(t(1, 4, 5, 3)),
        lambda: handoff.rgb_to_i420_device(t(1, 4, 4, 1)), lambda: handoff.rgb_to_i420_device(t(1, 4, 4, 4)),
        lambda: handoff.rgb_to_i420_device(t(1, 4, 4, 3, dtype=torch.float32)), lambda: handoff.rgb_to_i420_device(good, "yuv"),
        lambda: handoff.rgb_to_i420_device(good, out=t(2, 6, 4)), lambda: handoff.rgb_to_i420_device(good, out=t(2, 6, 6, dtype=torch.int8)),
        lambda: handoff.rgb_to_i420_device(good, out=torch.zeros((2, 6, 6), dtype=torch.uint8)),
        lambda: handoff.rgb_to_i420_device(good, out=t(2, 6, 12)[:, :, ::2]), lambda: handoff.rgb_to_i420_device(t(4, 6, 3)),
        lambda: handoff.rgb_to_i420_device(good.cpu()), lambda: handoff.rgb_to_i420_device(t(2, 4, 12, 3)[:, :, ::2]),
    ]
    torch.cuda.synchronize()
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    assert _lib.lib().elvis_last_launch() == b"rgb_to_i420_kernel<bgr>"
    with pytest.raises(ValueError):
        handoff.write_y4m([np.zeros((3, 4, 3), np.uint8)], os.devnull, 30, dev)
    with pytest.raises(ValueError):
        handoff.convert_frames_to_yuv420p([np.zeros((4, 4, 4), np.uint8)], dev)
    empty = handoff.rgb_to_i420_device(t(0, 4, 6, 3))
    assert empty.shape == (0, 6, 6) and empty.dtype == torch.uint8 and empty.device == good.device
