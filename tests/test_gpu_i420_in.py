"""The decoder hand-off on the device (csrc/i420_in.hip, elvis_amd/handoff.py, drivers.restore_yuv_clip) against
tests/_i420_in_ref.py: exact equality everywhere.  A lane takes a strip of 8 pixels of a row pair, so the widths are 2, 6,
10, 18, 66 (`w % 4 == 2`: no dword rows, the byte path), 8 (whole dword strips, chroma rows on a dword), 4, 12
(`w % 8 == 4`: dword rows whose chroma rows start off a dword, and a 4-pixel tail strip beside dword strips) and 16, which
on 16-byte pointers is the kernel of 16-pixel strips (`test_sixteen_pixel_strips` has its matrix) and off them dword
strips again.  Frames of 2 x 2 and 6 x 2 are 6 and 18 bytes: at n = 3 the later frames start off a dword."""
import os

import numpy as np
import pytest
import torch

import _handoff_ref as F
import _i420_in_ref as R

pytestmark = pytest.mark.gpu

WIDTHS = (2, 4, 6, 8, 10, 12, 16, 18, 66)
HEIGHTS = (2, 4, 6)
SENTINEL, GUARD = 0xA5, 64


def _planes(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)


def _frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _guarded(dev, data=None, shape=None, lead=GUARD):
    """A tensor of `shape` (or holding `data`) inside a sentinel-filled buffer, `lead` bytes in."""
    shape = tuple(data.shape) if data is not None else tuple(shape)
    size = int(np.prod(shape))
    buf = torch.full((lead + size + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    view = buf[lead:lead + size].view(shape)
    if data is not None:
        view.copy_(torch.from_numpy(data).to(dev))
    return buf, view


def _guards_intact(buf, lead=GUARD):
    host = buf.cpu().numpy()
    return bool((host[:lead] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all())


# ----------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("n", [1, 3])
def test_shape_matrix(gpu_device, n, order):
    from elvis_amd import _lib, handoff
    for h in HEIGHTS:
        for w in WIDTHS:
            planes = _planes(n, h, w, 1000 * h + w + n)
            want = R.i420_to_rgb(planes, order)
            sbuf, src = _guarded(gpu_device, planes)
            got = handoff.i420_to_rgb_device(src, order)
            assert got.shape == (n, h, w, 3) and got.dtype == torch.uint8 and got.is_contiguous()
            assert np.array_equal(got.cpu().numpy(), want), (n, h, w, order)
            dbuf, out = _guarded(gpu_device, shape=(n, h, w, 3))
            back = handoff.i420_to_rgb_device(src, order, out=out)
            assert back is out and np.array_equal(out.cpu().numpy(), want), (n, h, w, order, "out=")
            assert _guards_intact(dbuf) and _guards_intact(sbuf), (n, h, w, order)
            assert np.array_equal(src.cpu().numpy(), planes)
    assert _lib.lib().elvis_last_launch() == f"i420_to_rgb_kernel<{order}>".encode()


@pytest.mark.parametrize("w", [8, 12, 16, 66])
def test_unaligned_pointers_take_the_byte_path(gpu_device, w):
    """A source or an output that does not start on a dword (a view into a larger tensor) is converted byte by byte."""
    from elvis_amd import handoff
    h = 6
    planes = _planes(2, h, w, w)
    want = R.i420_to_rgb(planes)
    for src_lead, out_lead in ((64, 61), (3, 64), (1, 62), (2, 63)):
        sbuf, src = _guarded(gpu_device, planes, lead=src_lead)
        dbuf, out = _guarded(gpu_device, shape=want.shape, lead=out_lead)
        handoff.i420_to_rgb_device(src, out=out)
        assert np.array_equal(out.cpu().numpy(), want), (w, src_lead, out_lead)
        assert _guards_intact(dbuf, out_lead) and _guards_intact(sbuf, src_lead) and np.array_equal(src.cpu().numpy(), planes)


@pytest.mark.parametrize("order", ["rgb", "bgr"])
def test_sixteen_pixel_strips(gpu_device, order):
    """`w % 16 == 0` with both pointers on 16 bytes is a kernel of its own (two strips a lane, 16-byte loads and stores,
    no tail); 4 or 8 bytes off, the same widths go back to the dword strips.  One strip, several, more than a workgroup's
    256 (80 x 130 x 3 is 975), frames that follow each other."""
    from elvis_amd import _lib, handoff
    for n, h, w in ((1, 2, 16), (3, 2, 16), (1, 6, 32), (3, 4, 48), (2, 6, 80), (3, 130, 80)):
        planes = _planes(n, h, w, 7 * h + w + n)
        want = R.i420_to_rgb(planes, order)
        for src_lead, out_lead, kernel in ((64, 64, "i420_to_rgb_x16_kernel"), (16, 48, "i420_to_rgb_x16_kernel"),
                                           (4, 64, "i420_to_rgb_kernel"), (64, 8, "i420_to_rgb_kernel"), (8, 12, "i420_to_rgb_kernel")):
            sbuf, src = _guarded(gpu_device, planes, lead=src_lead)
            dbuf, out = _guarded(gpu_device, shape=want.shape, lead=out_lead)
            handoff.i420_to_rgb_device(src, order, out=out)
            assert _lib.lib().elvis_last_launch() == f"{kernel}<{order}>".encode(), (n, h, w, src_lead, out_lead)
            assert np.array_equal(out.cpu().numpy(), want), (n, h, w, order, src_lead, out_lead)
            assert _guards_intact(dbuf, out_lead) and _guards_intact(sbuf, src_lead) and np.array_equal(src.cpu().numpy(), planes)


def test_every_yuv(gpu_device):
    """One 4096 x 4096 frame holding all 2^24 (Y, U, V) triples, bit for bit; both clamps are well exercised."""
    from elvis_amd import handoff
    frame = R.every_yuv_frame()
    want = R.i420_to_rgb(frame)
    low, high = float((want == 0).mean()), float((want == 255).mean())
    print(f"outputs at 0: {low:.3f}, at 255: {high:.3f}")
    assert low > 0.1 and high > 0.1
    got = handoff.i420_to_rgb_device(torch.from_numpy(frame).to(gpu_device)).cpu().numpy()
    assert np.array_equal(got, want)                                # the 16-pixel strips
    _, src = _guarded(gpu_device, frame, lead=4)                       # and, 4 bytes off, the dword strips
    assert np.array_equal(handoff.i420_to_rgb_device(src).cpu().numpy(), want)
    got = handoff.i420_to_rgb_device(torch.from_numpy(frame[:, :96 * 3 // 2]).to(gpu_device), "bgr").cpu().numpy()
    assert np.array_equal(got, R.i420_to_rgb(frame[:, :96 * 3 // 2], "bgr"))


def test_chroma_is_replicated_not_interpolated(gpu_device):
    """A U plane that is a checkerboard of 0 and 255 under flat Y and V: every quad is one colour, and there are two."""
    from elvis_amd import handoff
    h, w = 12, 20
    y = np.full((h, w), 128, np.uint8)
    u = (((np.arange(h // 2)[:, None] + np.arange(w // 2)[None]) & 1) * 255).astype(np.uint8)
    v = np.full((h // 2, w // 2), 128, np.uint8)
    planes = np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).reshape(1, h * 3 // 2, w)
    got = handoff.i420_to_rgb_device(torch.from_numpy(planes).to(gpu_device)).cpu().numpy()
    assert np.array_equal(got, R.i420_to_rgb(planes))
    corner = got[0, ::2, ::2]
    assert np.array_equal(got[0], np.repeat(np.repeat(corner, 2, axis=0), 2, axis=1))
    assert len(np.unique(got.reshape(-1, 3), axis=0)) == 2
    assert np.array_equal(corner[..., 2] > 128, u == 255)


def test_forward_then_inverse_is_the_two_statements(gpu_device):
    from elvis_amd import handoff
    frames = _frames(3, 6, 18, 21)
    for order in ("rgb", "bgr"):
        clip = torch.from_numpy(frames).to(gpu_device)
        got = handoff.i420_to_rgb_device(handoff.rgb_to_i420_device(clip, order), order).cpu().numpy()
        assert np.array_equal(got, R.i420_to_rgb(F.rgb_to_i420(frames, order), order)), order


def test_out_and_errors_come_before_any_launch(gpu_device):
    from elvis_amd import _lib, handoff
    dev = gpu_device

    def t(*shape, dtype=torch.uint8):
        return torch.zeros(shape, dtype=dtype, device=dev)

    good = t(2, 6, 6)                                              # two 4 x 6 frames
    out = t(2, 4, 6, 3)
    assert handoff.i420_to_rgb_device(good, "bgr", out=out) is out
    assert _lib.lib().elvis_last_launch() == b"i420_to_rgb_kernel<bgr>"
    bad_calls = [
        lambda: handoff.i420_to_rgb_device(t(1, 4, 4)), lambda: handoff.i420_to_rgb_device(t(1, 7, 4)),       # H = 3, 5: rows 4, 7
        lambda: handoff.i420_to_rgb_device(t(1, 6, 5)), lambda: handoff.i420_to_rgb_device(t(6, 6)),
        lambda: handoff.i420_to_rgb_device(t(1, 6, 6, 1)), lambda: handoff.i420_to_rgb_device(t(1, 6, 6, dtype=torch.float32)),
        lambda: handoff.i420_to_rgb_device(good, "yuv"), lambda: handoff.i420_to_rgb_device(good.cpu()),
        lambda: handoff.i420_to_rgb_device(t(2, 6, 12)[:, :, ::2]),
        lambda: handoff.i420_to_rgb_device(good, out=t(2, 4, 6, 4)), lambda: handoff.i420_to_rgb_device(good, out=t(2, 6, 4, 3)),
        lambda: handoff.i420_to_rgb_device(good, out=t(2, 4, 6, 3, dtype=torch.int8)),
        lambda: handoff.i420_to_rgb_device(good, out=torch.zeros((2, 4, 6, 3), dtype=torch.uint8)),
        lambda: handoff.i420_to_rgb_device(good, out=t(2, 4, 6, 6)[..., ::2]),
    ]
    torch.cuda.synchronize()
    handoff.rgb_to_i420_device(out)                                # any launch below would change the name again
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    assert _lib.lib().elvis_last_launch() == b"rgb_to_i420_kernel<rgb>"
    empty = handoff.i420_to_rgb_device(t(0, 6, 6))
    assert empty.shape == (0, 4, 6, 3) and empty.dtype == torch.uint8 and empty.device == good.device


# ----------------------------------------------------------------------------- clip files
@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """Five 18 x 6 frames, the Y4M and raw files `write_y4m` / `convert_frames_to_yuv420p` make of them, and the
    statements' word on what comes back: the forward statement, then the inverse."""
    from elvis_amd import handoff
    d = tmp_path_factory.mktemp("clip")
    frames = list(_frames(5, 6, 18, 31))
    y4m, raw = str(d / "clip.y4m"), str(d / "clip.yuv")
    handoff.write_y4m(frames, y4m, 29.97)
    with open(raw, "wb") as f:
        f.write(handoff.convert_frames_to_yuv420p(frames))
    planes = F.rgb_to_i420(np.stack(frames))
    assert open(y4m, "rb").read() == F.y4m_bytes(frames, 29.97) and open(raw, "rb").read() == planes.tobytes()
    return dict(frames=frames, y4m=y4m, raw=raw, planes=planes, rgb=R.i420_to_rgb(planes), bgr=R.i420_to_rgb(planes, "bgr"))


def test_load_y4m_and_yuv420p(gpu_device, clip):
    from elvis_amd import handoff
    for chunk in (1, 2, None):
        for order in ("rgb", "bgr"):
            got = handoff.load_y4m_device(clip["y4m"], gpu_device, order, chunk_frames=chunk)
            assert got.shape == (5, 6, 18, 3) and got.dtype == torch.uint8 and got.is_contiguous() and got.device == gpu_device
            assert np.array_equal(got.cpu().numpy(), clip[order]), (chunk, order)
            assert np.array_equal(handoff.load_yuv420p_device(clip["raw"], 18, 6, gpu_device, order, chunk_frames=chunk).cpu().numpy(), clip[order])
        raw = open(clip["raw"], "rb").read()
        assert np.array_equal(handoff.load_yuv420p_device(raw, 18, 6, gpu_device, chunk_frames=chunk).cpu().numpy(), clip["bgr"])
        for start, count in ((0, 2), (1, 3), (3, None), (4, 1), (5, 0), (2, 0)):
            want = clip["bgr"][start:None if count is None else start + count]
            for got in (handoff.load_y4m_device(clip["y4m"], gpu_device, start=start, count=count, chunk_frames=chunk),
                        handoff.load_yuv420p_device(clip["raw"], 18, 6, gpu_device, start=start, count=count, chunk_frames=chunk),
                        handoff.load_yuv420p_device(bytearray(raw), 18, 6, gpu_device, start=start, count=count, chunk_frames=chunk)):
                assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want), (chunk, start, count)
    for start, count in ((-1, 2), (4, 2), (6, None), (0, -1)):
        with pytest.raises(ValueError):
            handoff.load_y4m_device(clip["y4m"], gpu_device, start=start, count=count)
    with pytest.raises(ValueError):
        handoff.load_y4m_device(clip["y4m"], gpu_device, "yuv")


def test_read_y4m_of_write_y4m(gpu_device, clip):
    import elvis_amd
    frames, rate = elvis_amd.read_y4m(clip["y4m"])
    assert rate == 29.97 and len(frames) == 5 and all(f.shape == (6, 18, 3) and f.dtype == np.uint8 for f in frames)
    assert np.array_equal(np.stack(frames), clip["rgb"])
    assert np.array_equal(np.stack(elvis_amd.read_y4m(clip["y4m"], gpu_device, "bgr")[0]), clip["bgr"])


# ----------------------------------------------------------------------------- restore_yuv_clip
def _identity(clip_d, maps, block_size, device, first_frame_index, **kw):
    assert isinstance(clip_d, torch.Tensor) and clip_d.is_cuda and clip_d.dtype == torch.uint8 and not kw
    return clip_d


def _plus_global_index(clip_d, maps, block_size, device, first_frame_index, **kw):
    """Adds the frame's global index to every byte, and its map's first entry: a range that lands at another's offset,
    or with another's maps, shows."""
    add = torch.arange(first_frame_index, first_frame_index + clip_d.shape[0], device=clip_d.device) + torch.from_numpy(maps[:, 0, 0]).to(clip_d.device)
    return ((clip_d.to(torch.int32) + add.view(-1, 1, 1, 1).to(torch.int32)) & 255).to(torch.uint8)


def _want_files(bgr_clip):
    """What the driver writes for the resident BGR clip `bgr_clip` [n,6,18,3]: the forward statement's planes."""
    planes = F.rgb_to_i420(np.ascontiguousarray(bgr_clip), "bgr")
    return planes, F.y4m_header(18, 6, 29.97) + b"".join(b"FRAME\n" + p.tobytes() for p in planes)


def test_restore_yuv_clip_identity_between_the_formats(gpu_device, clip, tmp_path):
    """The inverse statement, then the forward statement, whichever container is on either side."""
    from elvis_amd import drivers
    maps = np.ones((5, 3, 9), np.int32)
    planes, y4m_file = _want_files(clip["bgr"])
    cases = [(clip["y4m"], "a.y4m", {}, y4m_file), (clip["raw"], "b.y4m", dict(width=18, height=6, framerate=29.97), y4m_file),
             (clip["y4m"], "c.yuv", {}, planes.tobytes()), (clip["raw"], "d.yuv", dict(width=18, height=6), planes.tobytes())]
    for src, name, kw, want in cases:
        out = str(tmp_path / name)
        drivers.restore_yuv_clip("blur", src, out, maps, 2, devices=[gpu_device], _shard_fn=_identity, **kw)
        assert open(out, "rb").read() == want, name
    out = str(tmp_path / "e.y4m")
    drivers.restore_yuv_clip("sinsr", clip["y4m"], out, maps, 2, devices=[gpu_device], framerate=25, _shard_fn=_identity)
    assert open(out, "rb").read() == F.y4m_header(18, 6, 25) + y4m_file[len(F.y4m_header(18, 6, 29.97)):]


def test_restore_yuv_clip_ranges_land_at_their_own_offsets(gpu_device, clip, tmp_path):
    from elvis_amd import drivers, handoff
    maps = (np.arange(5, dtype=np.int32) * 7)[:, None, None] * np.ones((5, 3, 9), np.int32)
    changed = ((clip["bgr"].astype(np.int32) + (np.arange(5) * 8)[:, None, None, None]) & 255).astype(np.uint8)
    planes, y4m_file = _want_files(changed)
    # the same device twice is one device, as in every driver here: one range, in-process
    out = str(tmp_path / "one.y4m")
    drivers.restore_yuv_clip("dct", clip["y4m"], out, maps, 2, devices=[0, 0], _shard_fn=_plus_global_index)
    assert open(out, "rb").read() == y4m_file
    # two ranges and a halo, the workers called as the parent calls them, the later range first
    for name, want, head in (("two.y4m", y4m_file, len(handoff.y4m_header(18, 6, 29.97))), ("two.yuv", planes.tobytes(), 0)):
        out = str(tmp_path / name)
        with open(out, "wb") as f:
            f.write(want[:head] + b"\xee" * (len(want) - head))
        source, sink = drivers.ClipFileSource(clip["raw"], "yuv", 18, 6, 5), drivers.ClipFileSink(out, name[-3:], head, 18, 6)
        for start, end in ((3, 5), (0, 3)):
            drivers._shard_worker(drivers.ShardJob(_plus_global_index, source, sink, resident=True, start=start, end=end, halo=1, maps=maps,
                                                   block_size=2, device="cuda:0", kw={}))
        assert open(out, "rb").read() == want, name


def _model_clip(tmp_path, n, seed):
    from elvis_amd import handoff
    frames = list(_frames(n, 64, 96, seed))
    path = str(tmp_path / "in.y4m")
    handoff.write_y4m(frames, path, 30)
    decoded = R.i420_to_rgb(F.rgb_to_i420(np.stack(frames)), "bgr")          # what a worker holds: BGR, decoded without a PNG
    rounds = np.random.default_rng(seed + 1).integers(0, 3, size=(n, 8, 12)).astype(np.int32)
    return path, [decoded[i] for i in range(n)], rounds


def test_restore_yuv_clip_blur(gpu_device, tmp_path):
    from elvis_amd import drivers, restore
    path, decoded, rounds = _model_clip(tmp_path, 3, 40)
    want = F.rgb_to_i420(np.stack(restore.restore_frames_blur(decoded, rounds, 8, gpu_device, batch_size=2)), "bgr")
    out = str(tmp_path / "out.yuv")
    drivers.restore_yuv_clip("blur", path, out, rounds, 8, devices=["cuda:0"], batch_size=2)
    assert open(out, "rb").read() == want.tobytes()


def test_restore_yuv_clip_dct_and_its_halo(gpu_device, tmp_path):
    from elvis_amd import drivers, handoff, restore
    path, decoded, rounds = _model_clip(tmp_path, 4, 50)
    rounds[:] = np.maximum(rounds, 1)                                        # every block restored: the halo shows everywhere
    want = F.rgb_to_i420(np.stack(restore.restore_frames_dct(decoded, rounds, 8, gpu_device)), "bgr")
    out = str(tmp_path / "out.y4m")
    drivers.restore_yuv_clip("dct", path, out, rounds, 8, devices=["cuda:0"])
    head = handoff.y4m_header(96, 64, 30)
    assert open(out, "rb").read() == head + b"".join(b"FRAME\n" + p.tobytes() for p in want)
    # two ranges, each with the restorer's halo read from the file: the same bytes as the whole clip at once
    split = str(tmp_path / "split.yuv")
    with open(split, "wb") as f:
        f.truncate(want.size)
    source, sink = drivers.ClipFileSource(path, "y4m", 96, 64, 4), drivers.ClipFileSink(split, "yuv", 0, 96, 64)
    for start, end in ((0, 2), (2, 4)):
        drivers._shard_worker(drivers.ShardJob(drivers._dct_clip_shard, source, sink, resident=True, start=start, end=end, halo=3,
                                               maps=rounds, block_size=8, device="cuda:0", kw={}))
    assert open(split, "rb").read() == want.tobytes()
    # and without the halo the ranges' edge frames miss their neighbours
    with open(split, "wb") as f:
        f.truncate(want.size)
    for start, end in ((0, 2), (2, 4)):
        drivers._shard_worker(drivers.ShardJob(drivers._dct_clip_shard, source, sink, resident=True, start=start, end=end, halo=0,
                                               maps=rounds, block_size=8, device="cuda:0", kw={}))
    assert open(split, "rb").read() != want.tobytes()


def test_restore_yuv_clip_pixels_never_visit_the_host(gpu_device, tmp_path, monkeypatch):
    """With `frames_to_host` and the host branch of `frames_to_device` refusing, the driver still runs: only I420 planes
    cross the bus."""
    from elvis_amd import drivers, handoff, recompose, restore
    path, decoded, rounds = _model_clip(tmp_path, 3, 60)
    want = F.rgb_to_i420(np.stack(restore.restore_frames_blur(decoded, rounds, 8, gpu_device, batch_size=2)), "bgr")

    def refuse(*args, **kw):
        raise AssertionError("pixels went through the host")

    real_to_device = recompose.frames_to_device

    def resident_only(frames, device):
        return real_to_device(frames, device) if isinstance(frames, torch.Tensor) else refuse()

    for module in (recompose, restore, drivers, handoff):
        for name, fn in (("frames_to_host", refuse), ("frames_to_device", resident_only)):
            if hasattr(module, name):
                monkeypatch.setattr(module, name, fn)
    with pytest.raises(AssertionError, match="through the host"):
        restore.restore_frames_blur(decoded, rounds, 8, gpu_device, batch_size=2)      # the host-to-host form is caught
    out = str(tmp_path / "out.yuv")
    drivers.restore_yuv_clip("blur", path, out, rounds, 8, devices=[gpu_device], batch_size=2)
    monkeypatch.undo()
    assert open(out, "rb").read() == want.tobytes()
