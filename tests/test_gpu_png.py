"""The PNG writer on the device (csrc/png.hip, elvis_amd/png.py) against its statement (tests/_png_ref.py): the device files
are the statement's files bit for bit on every case of the matrix, and - independently of the statement - PIL decodes them
to the input and zlib's CRC-32 agrees with every chunk.  Then: bytes do not depend on the upload chunks or on the batch,
guard bytes around the output buffer, gray masks, the directory drivers with both writers, and a compression bound that a
stored-only encoder cannot meet."""
import os
import zlib

import numpy as np
import pytest
import torch

import _png_ref as R
import elvis_amd
from elvis_amd import drivers, frameio, png

pytestmark = pytest.mark.gpu


def _resident(frames: np.ndarray, dev, offset: int = 0) -> torch.Tensor:
    """The clip on the device, `offset` bytes past a dword (allocations are aligned far beyond one)."""
    if not offset:
        return torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    base = torch.empty(frames.size + 8, dtype=torch.uint8, device=dev)
    view = base[offset:offset + frames.size].view(frames.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(frames)).to(dev))
    assert view.data_ptr() % 4 == offset and view.is_contiguous()
    return view


def _check_file(data: bytes, frame: np.ndarray, order: str) -> None:
    """Without the statement: PIL gives the input back, every chunk's CRC is zlib's."""
    assert np.array_equal(R.decode_with_pil(data, order).reshape(frame.shape), frame)
    for kind, body, crc, _ in R.parse_chunks(data):
        assert zlib.crc32(kind + body) == crc, kind


@pytest.mark.parametrize("index", range(len(R.CASES)), ids=R.CASE_IDS)
def test_device_files_equal_the_statement(gpu_device, index):
    case = R.CASES[index]
    frames = case.frames()
    files = png.encode_png_device(_resident(frames, gpu_device, case.offset), case.order, case.filt, case.segment_rows)
    assert len(files) == case.n
    for f, (data, enc) in enumerate(zip(files, R.expected(index))):
        _check_file(data, frames[f], case.order)
        assert len(data) == len(enc.file)
        assert data == enc.file, f"frame {f}: first differing byte {next(i for i, (a, b) in enumerate(zip(data, enc.file)) if a != b)}"


def test_types_statistics_and_guard_bytes(gpu_device):
    index = R.CASE_IDS.index("content-diag-fadaptive")
    case, encs = R.CASES[index], R.expected(index)
    frames = case.frames()
    guard = 64
    out, plan, types = png._encode_clip(_resident(frames, gpu_device), case.order, case.filt, case.segment_rows, "test", guard=guard)
    host = out.cpu().numpy()
    total = int(plan.file_offsets[-1])
    assert host.size == total + 2 * guard
    assert (host[:guard] == 0xA5).all() and (host[guard + total:] == 0xA5).all(), "the pack kernels wrote outside the output buffer"
    assert np.array_equal(types.cpu().numpy(), np.stack([e.types for e in encs]))
    assert [int(b - a) for a, b in zip(plan.file_offsets[:-1], plan.file_offsets[1:])] == [len(e.file) for e in encs]
    files = png._finish_files(host[guard:guard + total], plan, case.h, case.w, case.c)
    assert [v.tobytes() for v in files] == [e.file for e in encs]


def test_bytes_do_not_depend_on_chunks_or_batch(gpu_device, tmp_path):
    frames = np.concatenate([R.make_content(kind, 1, 33, 65, 3, 7) for kind in ("diag", "noise", "hot")])
    d = _resident(frames, gpu_device)
    batch = png.encode_png_device(d)
    for f in range(3):
        assert png.encode_png_device(d[f:f + 1].contiguous()) == [batch[f]], "a frame encodes to other bytes alone"
    for chunk in (1, 2, None):
        paths = [tmp_path / f"c{chunk}" / f"{i}.png" for i in range(3)]
        png.save_frames(list(frames), paths, gpu_device, chunk_frames=chunk)
        assert [p.read_bytes() for p in paths] == batch
    png.save_frames(frames, [tmp_path / "arr" / f"{i}.png" for i in range(3)], str(gpu_device))        # one [n,...] array
    assert [(tmp_path / "arr" / f"{i}.png").read_bytes() for i in range(3)] == batch
    for i in range(3):
        assert np.array_equal(frameio.load_frame(tmp_path / "arr" / f"{i}.png"), frames[i])
    assert png.encode_png_device(d[:0]) == []
    # frames of two shapes in one call: every run of equal shapes is a clip
    mixed = [frames[0], frames[1][:16], frames[2]]
    paths = [tmp_path / "mixed" / f"{i}.png" for i in range(3)]
    png.save_frames(mixed, paths, gpu_device)
    for p, f in zip(paths, mixed):
        assert np.array_equal(frameio.load_frame(p), f)


def test_gray_masks_through_the_three_functions(gpu_device, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(9)
    masks = (rng.integers(0, 2, size=(3, 17, 63)) * 255).astype(np.uint8)
    d = _resident(masks, gpu_device)
    files = png.encode_png_device(d)
    assert files == png.encode_png_device(d[:, :, :, None].contiguous()) == [R.encode(m, "bgr", "adaptive", 16).file for m in masks]
    png.save_frames_device(d, [tmp_path / "a" / f"{i}.png" for i in range(3)])
    png.save_frames(list(masks), [tmp_path / "b" / f"{i}.png" for i in range(3)], gpu_device)
    for i in range(3):
        assert (tmp_path / "a" / f"{i}.png").read_bytes() == (tmp_path / "b" / f"{i}.png").read_bytes() == files[i]
        with Image.open(tmp_path / "a" / f"{i}.png") as im:
            assert im.mode == "L" and np.array_equal(np.asarray(im), masks[i])


def test_device_argument_checks(gpu_device):
    ok = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=gpu_device)
    with pytest.raises(ValueError, match="contiguous"):
        png.encode_png_device(ok[:, :, ::2])
    with pytest.raises(ValueError, match="channels"):
        png.encode_png_device(torch.zeros((1, 8, 8, 2), dtype=torch.uint8, device=gpu_device))
    with pytest.raises(ValueError, match="empty"):
        png.encode_png_device(torch.zeros((1, 0, 8, 3), dtype=torch.uint8, device=gpu_device))
    with pytest.raises(ValueError, match="empty"):
        png.encode_png_device(torch.zeros((1, 8, 0, 3), dtype=torch.uint8, device=gpu_device))
    with pytest.raises(ValueError, match="path"):
        png.save_frames_device(ok, ["only-one.png"])


def test_flat_frame_is_compressed(gpu_device):
    """A stored-only encoder cannot pass: a flat 64x96x3 frame is 64 * (96 * 3 + 1) = 18 496 filtered bytes, and its file
    must be under a quarter of that (one bit a byte is about 2.5 KB with the block headers)."""
    frame = np.full((1, 64, 96, 3), 90, dtype=np.uint8)
    (data,) = png.encode_png_device(_resident(frame, gpu_device))
    _check_file(data, frame[0], "bgr")
    assert len(data) < 18496 // 4, len(data)


def _v1_directory(tmp_path, n=3, by=4, bx=6, b=8, k=2, seed=21):
    """A 3-frame 32x48 clip as the v1 client side receives it: shrunk frames 00001.png ... and the packed masks."""
    rng = np.random.default_rng(seed)
    masks = np.zeros((n, by, bx), np.uint8)
    for i in range(n):
        for r in range(by):
            masks[i, r, rng.choice(bx, k, replace=False)] = 1
    d = tmp_path / "frames"
    for i in range(n):
        frameio.save_frame(rng.integers(0, 256, size=(by * b, (bx - k) * b, 3), dtype=np.uint8), d / f"{i + 1:05d}.png")
    frameio.save_block_masks(masks, tmp_path / "masks.npz")
    return str(d), str(tmp_path / "masks.npz"), b, [f"{i + 1:05d}.png" for i in range(n)]


def _same_pixels(dir_a, dir_b, names, gray=False):
    from PIL import Image
    for name in names:
        with Image.open(os.path.join(dir_a, name)) as a, Image.open(os.path.join(dir_b, name)) as bb:
            assert a.mode == bb.mode == ("L" if gray else "RGB") and a.size == bb.size
            assert np.array_equal(np.asarray(a), np.asarray(bb)), name


def test_v1_drivers_with_both_writers(gpu_device, tmp_path):
    frames_dir, npz, b, names = _v1_directory(tmp_path)
    dirs = {}
    for writer in ("pil", "device"):
        root = tmp_path / writer
        dirs[writer] = {k: str(root / k) for k in ("stretch_out", "stretch_full", "stretch_blk", "out", "stretched", "full", "blk")}
        p = dirs[writer]
        drivers.stretch_shrunk_frames(frames_dir, npz, b, out_dir=p["stretch_out"], fullres_masks_dir=p["stretch_full"],
                                      block_masks_dir=p["stretch_blk"], devices=[gpu_device], png_writer=writer)
        drivers.restore_shrunk_frames(frames_dir, npz, b, p["out"], stretched_dir=p["stretched"], fullres_masks_dir=p["full"],
                                      block_masks_dir=p["blk"], devices=[gpu_device], png_writer=writer)
        for k in p:
            assert sorted(os.listdir(p[k])) == names, (writer, k)
    for k in ("stretch_out", "out", "stretched"):
        _same_pixels(dirs["pil"][k], dirs["device"][k], names)
        assert frameio.load_frame(os.path.join(dirs["device"][k], names[0])).shape == (32, 48, 3)
    for k in ("stretch_full", "full", "stretch_blk", "blk"):
        _same_pixels(dirs["pil"][k], dirs["device"][k], names, gray=True)
    # the device writer did write these: its files are the statement's, not PIL's
    for k in ("out", "stretched", "stretch_out"):
        data = open(os.path.join(dirs["device"][k], names[0]), "rb").read()
        assert data == R.encode(frameio.load_frame(os.path.join(dirs["pil"][k], names[0])), "bgr", "adaptive", 16).file
        assert data != open(os.path.join(dirs["pil"][k], names[0]), "rb").read()
    with pytest.raises(ValueError, match="png_writer"):
        drivers.restore_shrunk_frames(frames_dir, npz, b, str(tmp_path / "x"), devices=[gpu_device], png_writer="gpu")


def test_exported(gpu_device):
    frame = R.make_content("hramp", 1, 5, 9, 3, 0)
    assert elvis_amd.encode_png_device(_resident(frame, gpu_device)) == [R.encode(frame[0]).file]
