"""The clip intake on the GPU (elvis_amd/intake.py, csrc/resize.hip): bit-exact against the numpy statement in
tests/_resize_ref.py on its cases - whole ratios, fractional ones, tiles with remainders, a source row too wide for the
LDS -, `out=` inside guard bytes, the nearest resize, the error conventions, and the file-to-clip intake.  After every
resize the launch note is the instantiation `_resize_ref.area_kernel` derives from the plan and the two ratios."""
import numpy as np
import pytest
import torch

import _resize_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _launched():
    from elvis_amd import _lib
    return _lib.lib().elvis_last_launch().decode()


def _params():
    out = []
    for c in R.CHANNELS:
        for name, size in R.cases(c).items():
            for n in ((1,) if name in R.STEEP or name in R.STEEP_C1 else (1, 3)):
                out.append(pytest.param(size, c, n, id=f"{name if name.startswith('tiles') else name + f'_c{c}'}_n{n}"))
    return out


@pytest.mark.parametrize("size,c,n", _params())
def test_area_resize_is_the_statement_bit_for_bit(size, c, n):
    from elvis_amd import intake
    hs, ws, hd, wd = size
    x = R.frames(hs, ws, c, n)
    got = intake.resize_area_device(_up(x), hd, wd)
    assert _launched() == R.area_kernel(hs, ws, hd, wd, c)
    got = got.cpu().numpy()
    want = R.resize_area_u8(x, hd, wd)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ, first at {np.argwhere(got != want)[:3].tolist()}"


@pytest.mark.parametrize("name", ["7x10->3x4", "6x12->3x4", "17x33->16x32"])
def test_out_buffer_inside_guards_whatever_it_held(name):
    from elvis_amd import intake
    hs, ws, hd, wd = {**R.WHOLE, **R.FRACTIONAL}[name]
    n, c, guard = 3, 3, 37                                   # an odd guard: the result does not start on a dword
    x = R.frames(hs, ws, c, n)
    want = R.resize_area_u8(x, hd, wd)
    results = []
    for fill in (0xA5, 0x5A):
        big = torch.full((guard + want.size + guard,), fill, dtype=torch.uint8, device=DEV)
        out = big[guard:guard + want.size].view(n, hd, wd, c)
        assert intake.resize_area_device(_up(x), hd, wd, out=out) is out
        assert _launched() == R.area_kernel(hs, ws, hd, wd, c)
        host = big.cpu().numpy()
        assert (host[:guard] == fill).all() and (host[-guard:] == fill).all(), "guard bytes were written"
        results.append(host[guard:-guard].reshape(want.shape))
    assert np.array_equal(results[0], want) and np.array_equal(results[1], want)


def test_a_source_that_starts_off_a_dword_gives_the_same_bytes():
    """The rows are staged with dword loads where a dword lies whole inside the tile's segment: a clip that is a view at an
    odd byte offset takes the byte path at other places, and gives the same result."""
    from elvis_amd import intake
    hs, ws, hd, wd = R.cases(3)["tiles1.5_c3"]
    x = R.frames(hs, ws, 3, 2)
    want = R.resize_area_u8(x, hd, wd)
    for off in (1, 2, 3):
        big = torch.zeros(off + x.size, dtype=torch.uint8, device=DEV)
        view = big[off:].view(x.shape)
        view.copy_(_up(x))
        assert np.array_equal(intake.resize_area_device(view, hd, wd).cpu().numpy(), want), off
        assert _launched() == R.area_kernel(hs, ws, hd, wd, 3)


@pytest.mark.parametrize("src,dst", [((4, 6), (16, 24)), ((4, 6), (9, 13)), ((16, 24), (4, 6)), ((16, 24), (5, 7)), ((1, 1), (3, 5))])
def test_nearest_resize_is_the_statement_and_the_hosts(src, dst):
    from elvis_amd import intake
    from elvis_amd.complexity import resize_masks_nearest
    rng = np.random.default_rng(7)
    for shape in ((3,) + src, (2,) + src + (3,), (1,) + src + (1,), (2,) + src + (4,)):
        x = rng.integers(0, 256, shape, dtype=np.uint8)
        got = intake.resize_nearest_device(_up(x), *dst)
        assert _launched() == R.NEAREST_KERNEL
        got = got.cpu().numpy()
        assert np.array_equal(got, R.resize_nearest_u8(x, *dst)), shape
    masks = [rng.integers(0, 2, src, dtype=np.uint8), None, rng.integers(0, 2, src, dtype=np.uint8),
             rng.integers(0, 2, (src[0] + 1, src[1]), dtype=np.uint8)]
    got = intake.resize_masks_nearest_device(masks, *dst, device=DEV)
    want = resize_masks_nearest(masks, *dst)
    assert got[1] is None and all(np.array_equal(g, w) for g, w in zip(got, want) if w is not None)
    assert np.array_equal(intake.resize_nearest_device(_up(np.stack([masks[0], masks[2]])), *dst).cpu().numpy(),
                          np.stack([want[0], want[2]]))


def test_error_conventions_on_the_device():
    from elvis_amd import intake
    x = _up(R.frames(6, 8, 3, 1))
    with pytest.raises(ValueError, match="height"):
        intake.resize_area_device(x, 7, 8)
    with pytest.raises(ValueError, match="width"):
        intake.resize_area_device(x, 6, 9)
    with pytest.raises(ValueError, match="positive"):
        intake.resize_area_device(x, 0, 4)
    with pytest.raises(ValueError, match="positive"):
        intake.resize_nearest_device(x, 4, 0)
    with pytest.raises(ValueError, match="uint8"):
        intake.resize_area_device(x.float(), 3, 4)
    with pytest.raises(ValueError, match="uint8"):
        intake.resize_area_device(x[0], 3, 4)                                  # rank 3
    with pytest.raises(ValueError, match="uint8"):
        intake.resize_area_device(_up(np.zeros((1, 6, 8, 2), np.uint8)), 3, 4)   # two channels
    with pytest.raises(ValueError, match="uint8"):
        intake.resize_nearest_device(x[:, :, ::2], 3, 4)                       # not contiguous
    for bad in (torch.zeros((1, 3, 4, 1), dtype=torch.uint8, device=DEV), torch.zeros((1, 3, 4, 3), dtype=torch.int8, device=DEV),
                torch.zeros((1, 3, 4, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="out must be"):
            intake.resize_area_device(x, 3, 4, out=bad)
        with pytest.raises(ValueError, match="out must be"):
            intake.resize_nearest_device(x, 3, 4, out=bad)
    # the library's own check, without the Python one in front of it
    from elvis_amd import _lib as L
    h = L.lib()
    assert h.elvis_resize_area_u8(1, 1, 1, 6, 8, 7, 8, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 4, None) == -1
    assert b"height" in h.elvis_last_error()


def test_host_forms_take_cv2s_argument_order():
    from elvis_amd import intake
    x = R.frames(7, 10, 3, 1)
    small = intake.resize_area(x[0], (4, 3), device=DEV)                       # (width, height)
    assert np.array_equal(small, R.resize_area_u8(x, 3, 4)[0])
    gray = intake.resize_area(x[0, :, :, 0], (4, 3), device=DEV)
    assert gray.shape == (3, 4) and np.array_equal(gray, R.resize_area_u8(x[..., :1], 3, 4)[0, :, :, 0])


@pytest.fixture(scope="module")
def y4m_clip(tmp_path_factory):
    from elvis_amd.handoff import load_y4m_device, write_y4m
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (12, 18, 3), dtype=np.uint8) for _ in range(5)]
    path = str(tmp_path_factory.mktemp("intake") / "clip.y4m")
    write_y4m(frames, path, 25.0, DEV)
    return path, load_y4m_device(path, DEV, "rgb").cpu().numpy(), frames


def test_intake_from_a_y4m_file(y4m_clip):
    from elvis_amd import intake
    path, decoded, frames = y4m_clip
    want = R.resize_area_u8(decoded[[0, 2]], 6, 8)
    for chunk in (1, None):
        clip, rate = intake.load_clip_device(path, 8, 6, DEV, frame_stride=2, max_frames=2, chunk_frames=chunk)
        assert rate == 25.0 and clip.is_cuda and tuple(clip.shape) == (2, 6, 8, 3)
        assert np.array_equal(clip.cpu().numpy(), want), chunk
    assert np.array_equal(intake.intake_device(_up(decoded), 8, 6, 2, 2).cpu().numpy(), want)
    # a raw file of the same frames: the size comes from the caller, there is no frame rate
    from elvis_amd.handoff import convert_frames_to_yuv420p
    raw = path[:-4] + ".yuv"
    with open(raw, "wb") as f:
        f.write(convert_frames_to_yuv420p(frames, DEV))
    clip, rate = intake.load_clip_device(raw, 8, 6, DEV, src_width=18, src_height=12, frame_stride=2, max_frames=2)
    assert rate is None and np.array_equal(clip.cpu().numpy(), want)


def test_analyze_clip_file_is_the_removability_of_the_working_size_clip(tmp_path):
    from elvis_amd import drivers, intake
    from elvis_amd.handoff import write_y4m
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, (1, 120, 120, 3), dtype=np.uint8)
    frames = [np.roll(base[0], 3 * i, axis=1) for i in range(3)]               # 120x120 -> 80x80: the segmenter's default radius needs 68 pixels a side
    path = str(tmp_path / "src.y4m")
    write_y4m(frames, path, 30.0, DEV)
    clip, _ = intake.load_clip_device(path, 80, 80, DEV)
    want = drivers.calculate_removability_scores_device(clip.cpu().numpy(), 16, device=DEV, order="rgb")
    got = drivers.analyze_clip_file(path, 80, 80, 16, device=DEV)
    assert got.shape == (3, 5, 5) and np.array_equal(got, want)
