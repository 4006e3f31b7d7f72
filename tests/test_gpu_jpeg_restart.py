"""Restart intervals of the JPEG writer on the device (csrc/jpeg_write.hip, csrc/jpeg_encode.h, elvis_amd/jpeg_write.py
`restart_rows=` / `restart_mcus=`) against their statement (tests/_jpeg_restart_ref.py) and PIL on libjpeg-turbo, byte for
byte: every case of the restart corpus in both channel orders with guard bytes around every buffer and work buffers that
start from 0x00, 0xFF and 0x7F, a clip of mixed content whose intervals differ in length and start off dword boundaries
alone and in a batch, intervals of 255, 256 and 257 blocks around a chunk of the prefix sum, an interval longer than two
chunks of the stuffing pass, intervals of one byte, more (frame, interval) pairs than grid.y takes, the explicit
`restart_rows=0, restart_mcus=0`, the round trip through the device reader, and a directory driver."""
import os

import numpy as np
import pytest
import torch

import _jpeg_ref as R
import _jpeg_restart_ref as S
import _jpeg_write_ref as W
import elvis_amd
from elvis_amd import drivers, frameio, jpeg, jpeg_write, recompose

pytestmark = pytest.mark.gpu
GUARD = 64
BUFFERS = ("out_buf", "coef_buf", "bits_buf", "words_buf", "ffc_buf", "sizes_buf")
FILLS = (0x00, 0xFF, 0x7F)
SCAN_CHUNK = jpeg_write.SCAN_CHUNK_BLOCKS
STUFF_CHUNK = jpeg_write.STUFF_CHUNK_BYTES


def _guards_intact(buf: torch.Tensor) -> bool:
    host = buf.cpu().numpy()
    return bool((host[:GUARD] == 0xA5).all() and (host[-GUARD:] == 0xA5).all())


def _files(got):
    host = got["out"].cpu().numpy()
    off = got["out_off"]
    return [got["header"] + host[int(off[f]):int(off[f + 1])].tobytes() for f in range(off.size - 1)]


def _encode(frames: np.ndarray, device, order, quality, subsampling, fill=0, **restart):
    """(files, the dict of jpeg_write._encode_clip) of a host clip with `restart_rows=` or `restart_mcus=`, guards checked."""
    pair = (restart.get("restart_rows", 0), restart.get("restart_mcus", 0))
    got = jpeg_write._encode_clip(torch.from_numpy(np.ascontiguousarray(frames)).to(device), order, quality, subsampling, "test", guard=GUARD, fill=fill,
                                  restart=pair)
    for key in BUFFERS:
        assert _guards_intact(got[key]), key
    return _files(got), got


def _payload(buf: torch.Tensor, dtype):
    return buf.cpu().numpy()[GUARD:-GUARD].view(dtype)


# ----------------------------------------------------------------------------- the corpus
@pytest.mark.parametrize("order", ["bgr", "rgb"])
def test_device_bytes_equal_the_statement_and_pil(gpu_device, order):
    for k, c in enumerate(S.cases()):
        frame = c.frame()
        if order == "bgr" and c.channels == 3:
            frame = frame[..., ::-1]
        files, got = _encode(frame[None], gpu_device, order, c.quality, c.subsampling, fill=FILLS[(k + (order == "rgb")) % 3], **c.restart)
        want = S.encoded(c.name, order)
        assert got["restart_interval"] == want.ri and got["segments"] == len(want.intervals), c.name
        coef = _payload(got["coef_buf"], np.int16).reshape(got["blocks"], 64)
        assert np.array_equal(coef, want.blocks), c.name
        assert files == [want.data], c.name
        if R.have_turbo():
            assert S.entropy_part(files[0])[1] == S.entropy_part(S.pil_encode(c))[1], c.name


@pytest.mark.parametrize("name", ["w53-h37-gray-q75-noise-mcus3", "w53-h37-420-q95-checker255-mcus1", "w53-h37-444-q95-ramp-mcus5", "w53-h37-422-q30-white-rows1",
                                  "w33-h16-gray-q75-flat128-mcus1", "w17-h17-420-q100-flat200-mcus1"])
def test_work_buffers_that_start_dirty_give_the_same_bytes_and_layouts(gpu_device, name):
    """Every work buffer of the restart layout against the statement, from three starting contents: `bits_buf` [segments,
    segment_blocks + 1] holds every block's bit offset in its own interval and the interval's bit count (the elements past
    a short last interval repeat it), `words_buf` a span of whole words per interval with zeros up to the dword, `ffc_buf`
    [segments, chunks + 1], `sizes_buf` [segments] the bytes of every interval with its marker or EOI."""
    c = S.case(name)
    want = S.encoded(c.name)
    seen = []
    for fill in FILLS:
        files, got = _encode(c.frame()[None], gpu_device, "rgb", c.quality, c.subsampling, fill=fill, **c.restart)
        assert files == [want.data], fill
        segs, segb, chunks = got["segments"], got["segment_blocks"], got["chunks"]
        assert segs == len(want.intervals) > 1 and segb == want.ri * want.bpm and got["seg_off"].size == segs + 1
        bits = _payload(got["bits_buf"], np.uint32).reshape(segs, segb + 1).astype(np.int64)
        ffc = _payload(got["ffc_buf"], np.uint32).reshape(segs, chunks + 1).astype(np.int64)
        sizes = _payload(got["sizes_buf"], np.uint32).astype(np.int64)
        words = _payload(got["words_buf"], "<u4").astype(">u4").tobytes()
        at = 0
        for s, (stuffed, raw) in enumerate(want.intervals):
            lo, hi = s * segb, min((s + 1) * segb, len(want.blocks))
            lengths = []
            W.entropy(want.blocks[lo:hi].astype(np.int64), want.comp[lo:hi], None, lengths)
            offsets = np.concatenate([[0], np.cumsum(lengths)])
            assert np.array_equal(bits[s, :hi - lo + 1], offsets) and (bits[s, hi - lo:] == offsets[-1]).all(), (fill, s)
            assert len(raw) == (offsets[-1] + 7) // 8
            padded = raw + bytes(-len(raw) % 4)
            assert words[at:at + len(padded)] == padded, (fill, s)
            at += len(padded)
            ff = [raw[k:k + STUFF_CHUNK].count(b"\xff") for k in range(0, chunks * STUFF_CHUNK, STUFF_CHUNK)]
            assert np.array_equal(ffc[s], np.concatenate([[0], np.cumsum(ff)])), (fill, s)
            assert sizes[s] == len(stuffed) + 2 == got["seg_off"][s + 1] - got["seg_off"][s], (fill, s)
        assert at == len(words)
        seen.append((bits.tobytes(), words, ffc.tobytes(), sizes.tobytes()))
    assert seen[0] == seen[1] == seen[2]


# ----------------------------------------------------------------------------- batching
def test_mixed_content_off_dword_boundaries_alone_and_in_a_batch(gpu_device):
    kinds = ("flat", "noise", "ramp", "checker", "white", "noise", "checker255")
    frames = np.stack([W.make_frame(k, 37, 53, 3, 900 + i) for i, k in enumerate(kinds)])
    for restart in (dict(restart_rows=1), dict(restart_mcus=3), dict(restart_mcus=1)):
        files, got = _encode(frames, gpu_device, "rgb", 95, "420", **restart)
        seg = np.diff(got["seg_off"])
        assert len(set(seg.tolist())) >= 5 and (got["seg_off"][1:-1] % 4 != 0).any() and (seg % 4 != 0).any()
        assert np.array_equal(got["out_off"], got["seg_off"][::got["segments"]]) and got["out_off"].size == len(kinds) + 1
        for i in range(len(kinds)):
            assert files[i] == S.encode(frames[i], 95, "420", **restart).data, (kinds[i], restart)
            alone, _ = _encode(frames[i:i + 1], gpu_device, "rgb", 95, "420", **restart)
            assert alone == [files[i]], (kinds[i], restart)
        assert files == jpeg_write.encode_jpeg_device(torch.from_numpy(frames).to(gpu_device), "rgb", **restart)


# ----------------------------------------------------------------------------- interval sizes
@pytest.mark.parametrize("mcus", [SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1])
def test_interval_block_counts_around_a_scan_chunk(gpu_device, mcus):
    rng = np.random.default_rng(mcus)
    # gray, 600 blocks: two whole intervals of `mcus` blocks and a short one
    frames = rng.integers(0, 256, size=(2, 160, 240, 1), dtype=np.uint8)
    frames[1, :, :120] = 200
    files, got = _encode(frames, gpu_device, "rgb", 95, "420", restart_mcus=mcus)
    assert got["blocks"] == 600 and got["segment_blocks"] == mcus and got["segments"] == 3
    for i in range(2):
        assert files[i] == S.encode(frames[i], 95, "420", restart_mcus=mcus).data, i
    # 128x128 gray: 256 blocks, one interval short of, equal to and longer than the scan
    (c,) = [x for x in S.cases() if x.w == 128 and x.restart_mcus == mcus]
    assert len(S.encoded(c.name).intervals) == (2 if mcus < SCAN_CHUNK else 1)
    assert _encode(c.frame()[None], gpu_device, "rgb", c.quality, c.subsampling, restart_mcus=mcus)[0] == [S.encoded(c.name).data]
    # the 4:2:0 equivalent: 6 blocks an MCU, intervals of 43 MCUs are 258 blocks, of 42 are 252; 256 = 6 * 42 + 4 is no whole MCU
    colour = rng.integers(0, 256, size=(1, 128, 176, 3), dtype=np.uint8)
    for k in (42, 43):
        files, got = _encode(colour, gpu_device, "bgr", 95, "420", restart_mcus=k)
        assert got["segment_blocks"] == 6 * k and got["segments"] == -(-88 // k)
        assert files == [S.encode(colour[0], 95, "420", "bgr", restart_mcus=k).data], k


def test_one_interval_spans_more_than_two_chunks_of_the_stuffing(gpu_device):
    rng = np.random.default_rng(7)
    frame = rng.integers(0, 256, size=(1, 48, 157, 3), dtype=np.uint8)
    files, got = _encode(frame, gpu_device, "bgr", 100, "420", restart_rows=2)
    want = S.encode(frame[0], 100, "420", "bgr", restart_rows=2)
    assert len(want.intervals) == 2 and got["segments"] == 2 and got["chunks"] > 2
    assert all(len(raw) > 2 * STUFF_CHUNK for _, raw in want.intervals)
    assert all(sum(1 for k in range(0, len(raw), STUFF_CHUNK) if b"\xff" in raw[k:k + STUFF_CHUNK]) > 2 for _, raw in want.intervals)
    assert files == [want.data]
    # rows so many that the interval holds the frame: DRI and one segment
    files, got = _encode(frame, gpu_device, "bgr", 100, "420", restart_rows=1000)
    want = S.encode(frame[0], 100, "420", "bgr", restart_rows=1000)
    assert got["segments"] == 1 and got["restart_interval"] == 10000 and files == [want.data] and not S.markers(want.scan)


def test_intervals_of_one_byte(gpu_device):
    frames = np.full((3, 40, 72, 1), 128, np.uint8)
    frames[1, 8:16, 16:24] = 255            # one block that is longer, in the middle of a frame in the middle
    files, got = _encode(frames, gpu_device, "rgb", 75, "420", restart_mcus=1)
    assert got["segments"] == 45 and got["segment_blocks"] == 1
    seg = np.diff(got["seg_off"])
    assert (seg == 3).sum() == 3 * 45 - 1 and seg.max() > 3            # one byte and the marker
    nbytes = (_payload(got["bits_buf"], np.uint32).reshape(135, 2)[:, 1].astype(np.int64) + 7) // 8
    assert (nbytes == 1).sum() == 134 and _payload(got["words_buf"], np.uint32).size == ((nbytes + 3) // 4).sum() >= 135      # a word span each
    for i in range(3):
        want = S.encode(frames[i], 75, "420", restart_mcus=1)
        assert files[i] == want.data and (i == 1 or all(len(raw) == 1 for _, raw in want.intervals)), i
    if R.have_turbo():
        c = S.case("w33-h16-gray-q75-flat128-mcus1")
        assert S.entropy_part(_encode(c.frame()[None], gpu_device, "rgb", 75, "420", restart_mcus=1)[0][0])[1] == S.entropy_part(S.pil_encode(c))[1]


def test_more_segments_than_grid_y_takes(gpu_device):
    """257 frames of 256 intervals each are 65792 (frame, interval) pairs: the last frame's lie past 65535, where the
    segments go on along grid.z."""
    rng = np.random.default_rng(3)
    frames = np.full((257, 128, 128), 128, np.uint8)
    frames[0] = rng.integers(0, 256, size=(128, 128), dtype=np.uint8)
    frames[255] = rng.integers(0, 256, size=(128, 128), dtype=np.uint8)
    frames[256] = rng.integers(0, 256, size=(128, 128), dtype=np.uint8)
    got = jpeg_write._encode_clip(torch.from_numpy(frames).to(gpu_device), "rgb", 95, "420", "test", guard=GUARD, fill=0xFF, restart=(0, 1))
    for key in BUFFERS:
        assert _guards_intact(got[key]), key
    assert got["segments"] == 256 and got["seg_off"].size == 257 * 256 + 1 > 65536
    files = _files(got)
    flat = S.encode(frames[1], 95, "420", restart_mcus=1).data
    assert all(f == flat for f in files[1:255])
    for i in (0, 255, 256):
        assert files[i] == S.encode(frames[i], 95, "420", restart_mcus=1).data, i


# ----------------------------------------------------------------------------- the explicit Ri = 0
def test_explicit_zero_is_todays_output_and_todays_layouts(gpu_device):
    kinds = ("noise", "flat", "checker255", "white")
    frames = np.stack([W.make_frame(k, 37, 53, 3, 60 + i) for i, k in enumerate(kinds)])
    clip = torch.from_numpy(frames).to(gpu_device)
    want = [W.encode(f, 95, "420").data for f in frames]
    assert jpeg_write.encode_jpeg_device(clip, "rgb", restart_rows=0, restart_mcus=0) == want
    assert jpeg_write.encode_jpeg_device(clip, "rgb") == want
    assert elvis_amd.encode_jpeg_device(clip, "rgb", 95, "420", restart_rows=0) == want
    files, got = _encode(frames, gpu_device, "rgb", 95, "420", restart_rows=0, restart_mcus=0)
    old = jpeg_write._encode_clip(clip, "rgb", 95, "420", "test", GUARD, 0)          # the positional signature
    assert files == want and _files(old) == want
    assert sorted(got) == sorted(old) == sorted(BUFFERS + ("out", "out_off", "header", "blocks", "chunks"))
    n, blocks, chunks = len(kinds), got["blocks"], got["chunks"]
    assert got["out_off"].shape == (n + 1,) and got["out_off"].dtype == np.int64
    stream = [len(W.encode(f, 95, "420").unstuffed) for f in frames]
    assert _payload(got["bits_buf"], np.uint32).size == n * (blocks + 1)
    assert _payload(got["words_buf"], np.uint32).size == sum(-(-s // 4) for s in stream)
    assert _payload(got["ffc_buf"], np.uint32).size == n * (chunks + 1) and _payload(got["sizes_buf"], np.uint32).size == n
    for key in BUFFERS:
        assert torch.equal(got[key], old[key]), key


# ----------------------------------------------------------------------------- the round trip
def test_round_trip_with_intervals_gives_the_same_pixels_and_the_statements_sizes(gpu_device):
    rng = np.random.default_rng(11)
    for shape, sub, q in (((3, 37, 53, 3), "420", 95), ((2, 24, 40, 3), "422", 75), ((2, 37, 53, 1), "420", 95)):
        frames = rng.integers(0, 256, size=shape, dtype=np.uint8)
        clip = torch.from_numpy(frames).to(gpu_device)
        plain, plain_bytes = jpeg_write.jpeg_roundtrip_device(clip, q, sub)
        for restart in (dict(restart_rows=1), dict(restart_mcus=2)):
            decoded, nbytes = jpeg_write.jpeg_roundtrip_device(clip, q, sub, **restart)
            assert torch.equal(decoded, plain), (shape, restart)
            want = [len(S.encode(f, q, sub, "bgr", **restart).data) for f in frames]
            assert nbytes.dtype == np.int64 and nbytes.tolist() == want and nbytes.tolist() != plain_bytes.tolist(), (shape, restart)


def test_saved_files_and_host_frames(gpu_device, tmp_path):
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, size=(4, 23, 25, 3), dtype=np.uint8)
    want = [S.encode(f, 95, "420", "bgr", restart_rows=1).data for f in frames]
    paths = [tmp_path / "a" / f"{i}.jpg" for i in range(4)]
    jpeg_write.save_jpeg_frames_device(torch.from_numpy(frames).to(gpu_device), paths, restart_rows=1)
    assert [p.read_bytes() for p in paths] == want
    for chunk in (3, None):
        paths = [tmp_path / f"c{chunk}" / f"{i}.jpeg" for i in range(4)]
        elvis_amd.save_jpeg_frames(list(frames), paths, str(gpu_device), chunk_frames=chunk, restart_rows=1)
        assert [p.read_bytes() for p in paths] == want, chunk


# ----------------------------------------------------------------------------- a driver on a .jpg directory
def test_a_driver_writes_intervals_that_pil_and_the_device_reader_decode(gpu_device, tmp_path):
    from elvis_amd.restore import restore_frames_dct_device
    names = [f"{i + 1:05d}.jpg" for i in range(3)]
    plain_dir, rst_dir = str(tmp_path / "plain"), str(tmp_path / "rst")
    for d in (plain_dir, rst_dir):
        rng = np.random.default_rng(31)
        for name in names:
            frameio.save_frame(rng.integers(0, 256, size=(32, 40, 3), dtype=np.uint8), os.path.join(d, name))
    rounds = np.random.default_rng(12).integers(0, 3, size=(3, 4, 5)).astype(np.int32)
    decoded = recompose.frames_to_device([frameio.load_frame(os.path.join(plain_dir, n)) for n in names], gpu_device)
    restored = restore_frames_dct_device(decoded, rounds, 8).contiguous()
    drivers.restore_dct_adaptive(plain_dir, rounds, 8, devices=[gpu_device], jpeg_writer="device")
    drivers.restore_dct_adaptive(rst_dir, rounds, 8, devices=[gpu_device], jpeg_writer="device", jpeg_restart_rows=1)
    want = jpeg_write.encode_jpeg_device(restored, restart_rows=1)
    for i, n in enumerate(names):
        data = open(os.path.join(rst_dir, n), "rb").read()
        info = jpeg.parse_jpeg(data, n)
        assert data == want[i] and b"\xff\xdd\x00\x04\x00\x03" in data and info.restart_interval == 3 and len(info.segments) == 2, n
        assert jpeg.parse_jpeg(open(os.path.join(plain_dir, n), "rb").read(), n).restart_interval == 0
        assert np.array_equal(frameio.load_frame(os.path.join(rst_dir, n)), frameio.load_frame(os.path.join(plain_dir, n))), n
    assert torch.equal(jpeg.load_images_device([os.path.join(rst_dir, n) for n in names], gpu_device),
                       jpeg.load_images_device([os.path.join(plain_dir, n) for n in names], gpu_device))
    assert np.array_equal(jpeg.load_images_device([os.path.join(rst_dir, names[0])], gpu_device)[0].cpu().numpy(),
                          frameio.load_frame(os.path.join(rst_dir, names[0])))
