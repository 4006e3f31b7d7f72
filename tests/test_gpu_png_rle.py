"""The run-length stream of the device PNG writer (`deflate="rle"`: csrc/png.hip png_stats_rle_kernel / png_pack_rle_kernel,
csrc/png_rle.h) against its statement (tests/_png_rle_ref.py): the device files are the statement's bit for bit on the
smallest shapes where the token rule can break - run lengths around 3, 258 and 516, spans that end 1, 2, 3 and 259 bytes
into a second one, segments, every filter - and, independently of the statement, PIL and the device's own reader decode
them to the input and zlib's CRC-32 agrees with every chunk.  Then phase 1's statistics, guard bytes, batches and upload
chunks, the v1 drivers with all three writers, the literal stream unchanged, and the size conditions."""
import os

import numpy as np
import pytest
import torch

import _png_ref as R
import _png_rle_ref as S
from elvis_amd import drivers, frameio, png
from test_gpu_png import _check_file, _resident, _same_pixels, _v1_directory

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("index", range(len(S.CASES)), ids=S.CASE_IDS)
def test_device_files_equal_the_statement(gpu_device, index):
    case = S.CASES[index]
    frames = case.frames()
    files = png.encode_png_device(_resident(frames, gpu_device, case.offset), case.order, case.filt, case.segment_rows, deflate="rle")
    assert len(files) == case.n
    for f, (data, enc) in enumerate(zip(files, S.expected(index))):
        _check_file(data, frames[f], case.order)
        assert len(data) == len(enc.file)
        assert data == enc.file, f"frame {f}: first differing byte {next(i for i, (a, b) in enumerate(zip(data, enc.file)) if a != b)}"
    # the device's own reader: the single distance code of length 1 through inflate.h
    back = png.decode_png_device(files, gpu_device, case.order, case.c)
    assert np.array_equal(back.cpu().numpy(), frames)


@pytest.mark.parametrize("name", ["content-rect-fadaptive", "span-w4355", "span-rgb-1366", "seg-h33-s16", "run-w261", "type-byte-run"])
def test_types_statistics_and_guard_bytes(gpu_device, name):
    index = S.CASE_IDS.index(name)
    case, encs = S.CASES[index], S.expected(index)
    frames = case.frames()
    guard = 64
    out, plan, types = png._encode_clip(_resident(frames, gpu_device), case.order, case.filt, case.segment_rows, "test", guard=guard,
                                        deflate="rle")
    host = out.cpu().numpy()
    total = int(plan.file_offsets[-1])
    assert host.size == total + 2 * guard
    assert (host[:guard] == 0xA5).all() and (host[guard + total:] == 0xA5).all(), "the pack kernels wrote outside the output buffer"
    assert np.array_equal(types.cpu().numpy(), np.stack([e.types for e in encs]))
    assert [int(b - a) for a, b in zip(plan.file_offsets[:-1], plan.file_offsets[1:])] == [len(e.file) for e in encs]
    assert np.array_equal(plan.lengths, np.stack([e.lengths for e in encs]))
    files = png._finish_files(host[guard:guard + total], plan, case.h, case.w, case.c)
    assert [v.tobytes() for v in files] == [e.file for e in encs]
    # phase 1 alone: every one of the 290 words a segment
    n, h, w, c = frames.shape
    nseg = (h + case.segment_rows - 1) // case.segment_rows
    d = _resident(frames, gpu_device)
    types_d = torch.empty(n * h, dtype=torch.uint8, device=gpu_device)
    stats_d = torch.full((n * nseg * png.RLE_STATS_STRIDE,), -1, dtype=torch.int32, device=gpu_device)
    png.check(png.lib().elvis_png_stats_rle(png.ptr(d), png.ptr(types_d), png.ptr(stats_d), n, h, w, c, int(case.order == "bgr"),
                                            png._filter_code(case.filt), case.segment_rows, None), gpu_device)
    torch.cuda.synchronize(gpu_device)
    stats = stats_d.cpu().numpy().view(np.uint32).reshape(n, nseg, png.RLE_STATS_STRIDE)
    want = np.stack([S.segment_stats(e, h, w * c + 1, case.segment_rows) for e in encs])
    assert np.array_equal(stats, want)


def test_bytes_do_not_depend_on_chunks_or_batch(gpu_device, tmp_path):
    frames = np.concatenate([S.make_content(kind, 1, 33, 65, 3, 7) for kind in ("rect", "period9", "diag")])
    d = _resident(frames, gpu_device)
    batch = png.encode_png_device(d, deflate="rle")
    assert batch == [S.encode(f).file for f in frames]
    for f in range(3):
        assert png.encode_png_device(d[f:f + 1].contiguous(), deflate="rle") == [batch[f]], "a frame encodes to other bytes alone"
    for chunk in (1, 2, None):
        paths = [tmp_path / f"c{chunk}" / f"{i}.png" for i in range(3)]
        png.save_frames(list(frames), paths, gpu_device, chunk_frames=chunk, deflate="rle")
        assert [p.read_bytes() for p in paths] == batch
    paths = [tmp_path / "dev" / f"{i}.png" for i in range(3)]
    png.save_frames_device(d, paths, deflate="rle")
    assert [p.read_bytes() for p in paths] == batch
    for p, f in zip(paths, frames):
        assert np.array_equal(frameio.load_frame(p), f)
    assert png.encode_png_device(d[:0], deflate="rle") == []
    # gray masks as [n, H, W] and as [n, H, W, 1]
    masks = S.make_content("rect", 3, 17, 63, 1, 0)
    m = _resident(masks[:, :, :, 0], gpu_device)
    assert png.encode_png_device(m, deflate="rle") == png.encode_png_device(m[:, :, :, None].contiguous(), deflate="rle") == \
        [S.encode(f).file for f in masks]


def test_literal_stream_is_unchanged(gpu_device):
    for kind in ("diag", "zeros", "noise"):
        frames = R.make_content(kind, 2, 33, 65, 3, 5)
        want = [R.encode(f).file for f in frames]
        d = _resident(frames, gpu_device)
        assert png.encode_png_device(d, deflate="literal") == want
        assert png.encode_png_device(d) == want


def test_flat_frames_and_masks_are_small(gpu_device):
    """A condition, not a measurement: a flat 64x96x3 frame is 64 * (96 * 3 + 1) = 18 496 filtered bytes and its file is under
    one sixteenth of that, 1 156 bytes, which the literal stream (a bit a byte: at least 2 312) cannot meet; a 64x96 rectangle
    mask is under a quarter of its 6 208 filtered bytes."""
    for value in (0, 255):
        frame = np.full((1, 64, 96, 3), value, dtype=np.uint8)
        d = _resident(frame, gpu_device)
        (data,) = png.encode_png_device(d, "bgr", "adaptive", 16, deflate="rle")
        _check_file(data, frame[0], "bgr")
        print(f"flat {value}: {len(data)} bytes")
        assert len(data) < 18496 // 16, len(data)
        assert len(png.encode_png_device(d, "bgr", "adaptive", 16)[0]) >= 2312
    mask = S.make_content("rect", 1, 64, 96, 1, 0)
    (data,) = png.encode_png_device(_resident(mask, gpu_device), "bgr", "adaptive", 16, deflate="rle")
    _check_file(data, mask[0], "bgr")
    print(f"rectangle mask: {len(data)} bytes")
    assert len(data) < 6208 // 4, len(data)


def test_v1_drivers_with_all_three_writers(gpu_device, tmp_path):
    frames_dir, npz, b, names = _v1_directory(tmp_path)
    dirs = {}
    for writer in ("pil", "device", "device-rle"):
        root = tmp_path / writer
        dirs[writer] = {k: str(root / k) for k in ("stretch_out", "stretch_full", "stretch_blk", "out", "stretched", "full", "blk")}
        p = dirs[writer]
        drivers.stretch_shrunk_frames(frames_dir, npz, b, out_dir=p["stretch_out"], fullres_masks_dir=p["stretch_full"],
                                      block_masks_dir=p["stretch_blk"], devices=[gpu_device], png_writer=writer)
        drivers.restore_shrunk_frames(frames_dir, npz, b, p["out"], stretched_dir=p["stretched"], fullres_masks_dir=p["full"],
                                      block_masks_dir=p["blk"], devices=[gpu_device], png_writer=writer)
        for k in p:
            assert sorted(os.listdir(p[k])) == names, (writer, k)
    for writer in ("device", "device-rle"):
        for k in ("stretch_out", "out", "stretched"):
            _same_pixels(dirs["pil"][k], dirs[writer][k], names)
        for k in ("stretch_full", "full", "stretch_blk", "blk"):
            _same_pixels(dirs["pil"][k], dirs[writer][k], names, gray=True)
    # "device-rle" did write these with the run-length stream: frames, stretched frames and full-resolution masks are the
    # statement's files; the block-resolution masks stay PIL's
    rle = dirs["device-rle"]
    for k in ("out", "stretched", "stretch_out"):
        data = open(os.path.join(rle[k], names[0]), "rb").read()
        assert data == S.encode(frameio.load_frame(os.path.join(dirs["pil"][k], names[0])), "bgr", "adaptive", 16).file
    for k in ("full", "stretch_full"):
        from PIL import Image
        with Image.open(os.path.join(dirs["pil"][k], names[0])) as im:
            mask = np.asarray(im)
        data = open(os.path.join(rle[k], names[0]), "rb").read()
        assert data == S.encode(mask, "bgr", "adaptive", 16).file
        assert data != open(os.path.join(dirs["device"][k], names[0]), "rb").read()
    for k in ("blk", "stretch_blk"):
        assert open(os.path.join(rle[k], names[0]), "rb").read() == open(os.path.join(dirs["pil"][k], names[0]), "rb").read()
