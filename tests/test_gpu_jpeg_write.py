"""The JPEG writer on the device (csrc/jpeg_write.hip, csrc/jpeg_encode.h, elvis_amd/jpeg_write.py) against its statement
(tests/_jpeg_write_ref.py) and PIL on libjpeg-turbo, byte for byte: every case of the corpus in both channel orders with
guard bytes around every buffer, clips of mixed content whose scans fall off dword boundaries, a frame alone and in a
batch, block counts around a wave and around the chunks of the prefix sum and the stuffing pass, work buffers that start
from 0xFF and from 0x7F, the round trip through the device reader, and the directory drivers on a .jpg directory."""
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import _jpeg_ref as R
import _jpeg_write_ref as W
import elvis_amd
from elvis_amd import drivers, frameio, jpeg, jpeg_write, png, recompose

pytestmark = pytest.mark.gpu
GUARD = 64
BUFFERS = ("out_buf", "coef_buf", "bits_buf", "words_buf", "ffc_buf", "sizes_buf")
# the chunks the device's prefix sums and its stuffing pass work in (ELVIS_JPEG_SCAN_CHUNK, ELVIS_JPEG_STUFF_CHUNK)
SCAN_CHUNK = jpeg_write.SCAN_CHUNK_BLOCKS
STUFF_CHUNK = jpeg_write.STUFF_CHUNK_BYTES


def _guards_intact(buf: torch.Tensor) -> bool:
    host = buf.cpu().numpy()
    return bool((host[:GUARD] == 0xA5).all() and (host[-GUARD:] == 0xA5).all())


def _files(got):
    host = got["out"].cpu().numpy()
    off = got["out_off"]
    return [got["header"] + host[int(off[f]):int(off[f + 1])].tobytes() for f in range(off.size - 1)]


def _encode(frames: np.ndarray, device, order, quality, subsampling, fill=0):
    """(files, the dict of jpeg_write._encode_clip) of a host clip, guards checked."""
    got = jpeg_write._encode_clip(torch.from_numpy(np.ascontiguousarray(frames)).to(device), order, quality, subsampling, "test", guard=GUARD, fill=fill)
    for key in BUFFERS:
        assert _guards_intact(got[key]), key
    return _files(got), got


@lru_cache(maxsize=None)
def _pil_segment(name: str) -> bytes:
    c = W.case(name)
    return R.walk(W.pil_encode(c.frame(), c.quality, c.subsampling)).segments[0]


def _clips():
    """The corpus as clips: the cases of one size, sampling and quality."""
    groups = {}
    for c in W.cases():
        groups.setdefault((c.h, c.w, c.sampling, c.quality), []).append(c)
    return groups


@pytest.mark.parametrize("order", ["bgr", "rgb"])
def test_device_bytes_equal_the_statement_and_pil(gpu_device, order):
    for (h, w, sampling, quality), group in _clips().items():
        frames = np.stack([c.frame() for c in group])
        if order == "bgr" and sampling != "gray":
            frames = frames[..., ::-1]
        files, got = _encode(frames, gpu_device, order, quality, group[0].subsampling)
        assert got["blocks"] == len(W.encoded(group[0].name).blocks)
        coef = got["coef_buf"].cpu().numpy()[GUARD:-GUARD].view(np.int16).reshape(len(group), got["blocks"], 64)
        for i, c in enumerate(group):
            want = W.encoded(c.name, order)
            assert np.array_equal(coef[i], want.blocks), c.name
            assert files[i] == want.data, c.name
            if R.have_turbo():
                assert R.walk(files[i]).segments[0] == _pil_segment(c.name), c.name


def test_gray_clips_without_a_channel_axis(gpu_device):
    c = W.case("w53-h37-gray-q75-noise")
    clip = torch.from_numpy(np.ascontiguousarray(c.frame()[None, :, :, 0])).to(gpu_device)
    assert clip.shape == (1, 37, 53)
    assert jpeg_write.encode_jpeg_device(clip, quality=75) == [W.encoded(c.name).data]
    assert jpeg_write.encode_jpeg_device(clip[:0]) == []


def test_mixed_content_off_dword_boundaries_alone_and_in_a_batch(gpu_device):
    kinds = ("flat", "noise", "ramp", "checker", "white", "noise", "checker255")
    frames = np.stack([W.make_frame(k, 37, 53, 3, 900 + i) for i, k in enumerate(kinds)])
    files, got = _encode(frames, gpu_device, "rgb", 95, "420")
    sizes = np.diff(got["out_off"])
    assert len(set(sizes.tolist())) >= 5 and (got["out_off"][1:-1] % 4 != 0).any() and (sizes % 4 != 0).any()
    for i in range(len(kinds)):
        assert files[i] == W.encode(frames[i], 95, "420").data, kinds[i]
        alone, _ = _encode(frames[i:i + 1], gpu_device, "rgb", 95, "420")
        assert alone == [files[i]], kinds[i]
    assert files == jpeg_write.encode_jpeg_device(torch.from_numpy(frames).to(gpu_device), "rgb")


@pytest.mark.parametrize("blocks", [63, 64, 65, SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1, 2 * SCAN_CHUNK, 2 * SCAN_CHUNK + 1])
def test_block_counts_around_a_wave_and_a_scan_chunk(gpu_device, blocks):
    rng = np.random.default_rng(blocks)
    frames = rng.integers(0, 256, size=(2, 8, 8 * blocks, 1), dtype=np.uint8)
    frames[1, :, : 8 * blocks // 2] = 200                       # another length, so that the second frame's offsets differ
    files, got = _encode(frames, gpu_device, "rgb", 95, "420")
    assert got["blocks"] == blocks
    for i in range(2):
        assert files[i] == W.encode(frames[i], 95, "420").data, i


def test_one_frame_spans_more_than_two_chunks_of_the_scan_and_of_the_stuffing(gpu_device):
    rng = np.random.default_rng(7)
    frame = rng.integers(0, 256, size=(1, 150, 157, 3), dtype=np.uint8)
    files, got = _encode(frame, gpu_device, "bgr", 95, "420")
    want = W.encode(frame[0], 95, "420", "bgr")
    assert got["blocks"] > 2 * SCAN_CHUNK and got["chunks"] > 2 and len(want.unstuffed) > 2 * STUFF_CHUNK
    # FF bytes in more than one chunk of the stuffing pass, so that the prefix over the chunks counts
    assert sum(1 for k in range(0, len(want.unstuffed), STUFF_CHUNK) if b"\xff" in want.unstuffed[k:k + STUFF_CHUNK]) > 2
    assert files == [want.data]
    if R.have_turbo():
        assert R.walk(files[0]).segments[0] == R.walk(W.pil_encode(frame[0, :, :, ::-1], 95, "420")).segments[0]


@pytest.mark.parametrize("fill", [0xFF, 0x7F])
def test_work_buffers_that_start_dirty_give_the_same_bytes(gpu_device, fill):
    kinds = ("noise", "flat", "checker255")
    for sampling, c in (("420", 3), ("444", 3), ("gray", 1)):
        frames = np.stack([W.make_frame(k, 37, 53, c, 40 + i) for i, k in enumerate(kinds)])
        sub = "420" if sampling == "gray" else sampling
        clean, _ = _encode(frames, gpu_device, "rgb", 95, sub)
        dirty, _ = _encode(frames, gpu_device, "rgb", 95, sub, fill=fill)
        assert dirty == clean, sampling
        assert clean == [W.encode(f, 95, sub).data for f in frames], sampling


def test_round_trip_equals_pil_decoding_pils_own_file(gpu_device):
    rng = np.random.default_rng(11)
    for shape, sub, q in (((3, 37, 53, 3), "420", 95), ((2, 24, 40, 3), "422", 75), ((2, 17, 33, 3), "444", 30), ((2, 37, 53, 1), "420", 95)):
        frames = rng.integers(0, 256, size=shape, dtype=np.uint8)
        clip = torch.from_numpy(frames).to(gpu_device)
        for order in ("bgr", "rgb"):
            decoded, nbytes = jpeg_write.jpeg_roundtrip_device(clip, q, sub, order)
            assert decoded.shape == clip.shape and decoded.dtype == torch.uint8 and decoded.device == clip.device
            files = jpeg_write.encode_jpeg_device(clip, order, q, sub)
            assert nbytes.dtype == np.int64 and nbytes.tolist() == [len(f) for f in files]
            for i in range(shape[0]):
                rgb = frames[i] if order == "rgb" or shape[3] == 1 else frames[i, :, :, ::-1]
                want = R.decode_with_pil(W.pil_encode(rgb, q, sub), order, shape[3])
                assert np.array_equal(decoded[i].cpu().numpy(), want), (shape, order, i)


def test_saved_files_and_host_frames_at_any_chunk_size(gpu_device, tmp_path):
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, size=(4, 23, 25, 3), dtype=np.uint8)
    want = [W.encode(f, 95, "420", "bgr").data for f in frames]
    paths = [tmp_path / "a" / f"{i}.jpg" for i in range(4)]
    jpeg_write.save_jpeg_frames_device(torch.from_numpy(frames).to(gpu_device), paths)
    assert [p.read_bytes() for p in paths] == want
    for chunk in (1, 3, None):
        paths = [tmp_path / f"c{chunk}" / f"{i}.jpeg" for i in range(4)]
        elvis_amd.save_jpeg_frames(list(frames), paths, str(gpu_device), chunk_frames=chunk)
        assert [p.read_bytes() for p in paths] == want, chunk
    for i, p in enumerate(paths):
        assert np.array_equal(frameio.load_frame(p), R.decode(want[i], "bgr").pixels)


# ----------------------------------------------------------------------------- the drivers on a .jpg directory
def _jpg_directory(d, n=3, h=32, w=40, seed=31):
    rng = np.random.default_rng(seed)
    names = [f"{i + 1:05d}.jpg" for i in range(n)]
    for name in names:
        frameio.save_frame(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), os.path.join(d, name))
    return names


def _copy_dir(src, dst):
    os.makedirs(dst)
    for name in os.listdir(src):
        with open(os.path.join(src, name), "rb") as a, open(os.path.join(dst, name), "wb") as b:
            b.write(a.read())


def test_drivers_write_a_jpg_directory_on_the_device(gpu_device, tmp_path, monkeypatch):
    from elvis_amd.restore import restore_frames_dct_device
    src = str(tmp_path / "src")
    names = _jpg_directory(src)
    rounds = np.random.default_rng(12).integers(0, 3, size=(3, 4, 5)).astype(np.int32)
    # what the driver computes before it writes: the restored resident clip of the decoded frames
    decoded = recompose.frames_to_device([frameio.load_frame(os.path.join(src, n)) for n in names], gpu_device)
    restored = restore_frames_dct_device(decoded, rounds, 8)
    want_pixels, want_bytes = jpeg_write.jpeg_roundtrip_device(restored.contiguous())
    want_files = jpeg_write.encode_jpeg_device(restored.contiguous())
    assert not torch.equal(restored, decoded)
    # jpeg_writer="device": the GPU's own files, which PIL and the device reader decode to the round-trip pixels
    dev_dir = str(tmp_path / "device")
    _copy_dir(src, dev_dir)
    drivers.restore_dct_adaptive(dev_dir, rounds, 8, devices=[gpu_device], jpeg_writer="device")
    assert sorted(os.listdir(dev_dir)) == names
    for i, n in enumerate(names):
        data = open(os.path.join(dev_dir, n), "rb").read()
        assert data[:2] == b"\xff\xd8" and data == want_files[i] and len(data) == want_bytes[i]
        assert np.array_equal(frameio.load_frame(os.path.join(dev_dir, n)), want_pixels[i].cpu().numpy()), n
    assert torch.equal(jpeg.load_images_device([os.path.join(dev_dir, n) for n in names], gpu_device), want_pixels)
    # the default: PIL's files of the same restored frames, byte for byte what the driver wrote before there was an option
    pil_dir, ref_dir = str(tmp_path / "pil"), str(tmp_path / "ref")
    _copy_dir(src, pil_dir)
    drivers.restore_dct_adaptive(pil_dir, rounds, 8, devices=[gpu_device])
    for i, n in enumerate(names):
        frameio.save_frame(restored[i].cpu().numpy(), os.path.join(ref_dir, n))
        assert open(os.path.join(pil_dir, n), "rb").read() == open(os.path.join(ref_dir, n), "rb").read(), n
    # a replaced shard function returns host frames: they go up once and give the same files
    host_dir = str(tmp_path / "host")
    _copy_dir(src, host_dir)
    drivers.restore_dct_adaptive(host_dir, rounds, 8, devices=[gpu_device], jpeg_writer="device", _shard_fn=_restored_on_the_host)
    for i, n in enumerate(names):
        assert open(os.path.join(host_dir, n), "rb").read() == want_files[i], n

    # reader and both writers on the device: the pixels never visit the host
    def refuse(*args, **kw):
        raise AssertionError("pixels went through the host")

    real_to_device = recompose.frames_to_device
    monkeypatch.setattr(recompose, "frames_to_host", refuse)
    monkeypatch.setattr(png, "save_frames", refuse)
    monkeypatch.setattr(jpeg_write, "save_jpeg_frames", refuse)
    monkeypatch.setattr(frameio, "save_frame", refuse)
    monkeypatch.setattr(drivers, "save_frame", refuse)
    monkeypatch.setattr(recompose, "frames_to_device", lambda frames, device: real_to_device(frames, device) if isinstance(frames, torch.Tensor) else refuse())
    all_dir = str(tmp_path / "all")
    _copy_dir(src, all_dir)
    drivers.restore_dct_adaptive(all_dir, rounds, 8, devices=[gpu_device], png_reader="device", png_writer="device", jpeg_writer="device")
    monkeypatch.undo()
    for i, n in enumerate(names):
        assert open(os.path.join(all_dir, n), "rb").read() == want_files[i], n


def _restored_on_the_host(frames, maps, block_size, device, first_frame_index, **kw):
    from elvis_amd.restore import restore_frames_dct_device
    clip = recompose.frames_to_device(frames, device)
    return recompose.frames_to_host(restore_frames_dct_device(clip, maps, block_size))


def test_v1_masks_are_written_as_gray_jpeg(gpu_device, tmp_path):
    masks = (np.random.default_rng(2).integers(0, 2, size=(2, 24, 40), dtype=np.uint8) * 255)
    clip = torch.from_numpy(masks).to(gpu_device)
    drivers._write_clip(clip, str(tmp_path), ["1.jpg", "2.png"], "device", "device")
    data = (tmp_path / "1.jpg").read_bytes()
    assert data == W.encode(masks[0], 95, "420").data and len(jpeg.parse_jpeg(data).components) == 1
    assert (tmp_path / "2.png").read_bytes()[:8] == png.PNG_SIGNATURE
    assert np.array_equal(frameio.load_frame(tmp_path / "2.png")[:, :, 0], masks[1])


def test_exported(gpu_device):
    c = W.case("w16-h16-420-q100-checker255")
    clip = torch.from_numpy(c.frame()[None]).to(gpu_device)
    assert elvis_amd.encode_jpeg_device(clip, "rgb", 100, "420") == [W.encoded(c.name).data]


def _payload(buf: torch.Tensor, dtype):
    return buf.cpu().numpy()[GUARD:-GUARD].view(dtype)


@pytest.mark.parametrize("fill", [0x00, 0xFF])
@pytest.mark.parametrize("sampling,c", [("420", 3), ("422", 3), ("444", 3), ("gray", 1)])
def test_prefix_sums_stream_words_and_sizes_equal_what_the_statement_implies(gpu_device, sampling, c, fill):
    """The work buffers between the kernels, each against the statement: `bits_buf` holds every block's exclusive bit offset
    and the total (jpeg_bits_kernel's lengths through jpeg_scan_kernel), `words_buf` the unstuffed stream most significant
    byte first with zeros up to the dword (jpeg_pack_kernel into what jpeg_clear_kernel cleared - the buffers start from
    0xFF in half of the runs), `ffc_buf` the exclusive FF counts of the 1024-byte chunks and their total (jpeg_ff_kernel
    through jpeg_scan_kernel), `sizes_buf` the bytes of every finished scan with EOI (jpeg_sizes_kernel)."""
    kinds = ("noise", "flat", "checker255", "white")
    frames = np.stack([W.make_frame(k, 37, 53, c, 60 + i) for i, k in enumerate(kinds)])
    sub = "420" if sampling == "gray" else sampling
    files, got = _encode(frames, gpu_device, "rgb", 95, sub, fill=fill)
    n, blocks, chunks = len(kinds), got["blocks"], got["chunks"]
    bits = _payload(got["bits_buf"], np.uint32).reshape(n, blocks + 1).astype(np.int64)
    ffc = _payload(got["ffc_buf"], np.uint32).reshape(n, chunks + 1).astype(np.int64)
    sizes = _payload(got["sizes_buf"], np.uint32).astype(np.int64)
    words = _payload(got["words_buf"], "<u4").astype(">u4").tobytes()
    want = [W.encode(f, 95, sub) for f in frames]
    assert chunks == max(-(-len(e.unstuffed) // STUFF_CHUNK) for e in want) and chunks >= 2
    assert any(len(e.unstuffed) % 4 for e in want) and any(b"\xff" in e.unstuffed for e in want)
    at = 0
    for i, e in enumerate(want):
        assert e.block_bits.size == blocks and (e.block_bits > 0).all()
        assert np.array_equal(bits[i], np.concatenate([[0], np.cumsum(e.block_bits)])), f"{kinds[i]}: bit offsets"
        assert len(e.unstuffed) == (int(bits[i, blocks]) + 7) // 8
        padded = e.unstuffed + bytes(-len(e.unstuffed) % 4)
        assert words[at:at + len(padded)] == padded, f"{kinds[i]}: stream words"
        at += len(padded)
        ff = [e.unstuffed[k:k + STUFF_CHUNK].count(b"\xff") for k in range(0, chunks * STUFF_CHUNK, STUFF_CHUNK)]
        assert np.array_equal(ffc[i], np.concatenate([[0], np.cumsum(ff)])), f"{kinds[i]}: FF counts"
        assert sizes[i] == len(e.unstuffed) + sum(ff) + 2 == len(e.scan) + 2, f"{kinds[i]}: size"
        assert files[i] == e.data
    assert at == len(words)
