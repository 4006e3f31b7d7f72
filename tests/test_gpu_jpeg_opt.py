"""Per-frame optimised Huffman tables of the JPEG writer on the device (csrc/jpeg_write.hip `jpeg_bits_kernel` in its tally
mode, the per-frame table stride of `jpeg_bits_kernel` and `jpeg_pack_kernel`, elvis_amd/jpeg_write.py `optimize=True`)
against the statement of tests/_jpeg_opt_ref.py and PIL with `optimize=True`, byte for byte: the corpus in both channel
orders, every case alone and inside a batch of frames with other content, the length-limit fixture, the histogram buffer
as a stage of its own with work buffers that start dirty, segments of 255 / 256 / 257 and 511 / 513 blocks and short last
segments, the ROI dead zone, restart intervals through both decoders, the sizes without the files, the quality search,
and a directory driver."""
import io
import os

import numpy as np
import pytest
import torch

import _jpeg_opt_ref as O
import _jpeg_ref as R
import _jpeg_roi_ref as X
from elvis_amd import drivers, frameio, handoff, jpeg, jpeg_write, recompose

pytestmark = pytest.mark.gpu
GUARD = 64
BUFFERS = ("out_buf", "coef_buf", "bits_buf", "words_buf", "ffc_buf", "sizes_buf", "hist_buf")


def _guards_intact(buf: torch.Tensor) -> bool:
    host = buf.cpu().numpy()
    return bool((host[:GUARD] == 0xA5).all() and (host[-GUARD:] == 0xA5).all())


def _encode(frames: np.ndarray, device, order, quality, subsampling, fill=0, levels=None, B=0, **restart):
    """(files, the dict of jpeg_write._encode_clip) of a host clip with `optimize=True`, guards checked."""
    pair = (restart.get("restart_rows", 0), restart.get("restart_mcus", 0))
    got = jpeg_write._encode_clip(torch.from_numpy(np.ascontiguousarray(frames)).to(device), order, quality, subsampling, "test", guard=GUARD, fill=fill,
                                  restart=pair, roi_levels=levels, roi_block_size=B, optimize=True)
    for key in BUFFERS:
        assert _guards_intact(got[key]), key
    assert "header" not in got and len(got["headers"]) == len(frames)
    host = got["out"].cpu().numpy()
    off = got["out_off"]
    return [got["headers"][f] + host[int(off[f]):int(off[f + 1])].tobytes() for f in range(off.size - 1)], got


def _hist(got) -> np.ndarray:
    return got["hist_buf"].cpu().numpy()[GUARD:-GUARD].view(np.uint32).reshape(-1, 2, 272).astype(np.int64)


def _mates(c: O.Case, order: str) -> np.ndarray:
    """The case's frame between two frames of its shape with other content."""
    frame = c.frame()
    if order == "bgr" and c.channels == 3:
        frame = frame[..., ::-1]
    noise = R.make_content("noise", c.h, c.w, c.channels, c.seed + 5000)
    flat = np.full_like(frame, 77)
    return np.stack([noise, frame, flat])


# ----------------------------------------------------------------------------- the corpus
@pytest.mark.parametrize("sampling", R.SAMPLINGS)
@pytest.mark.parametrize("order", ["bgr", "rgb"])
def test_device_bytes_equal_the_statement_and_pil_alone_and_in_a_batch(gpu_device, order, sampling):
    differ = 0
    for k, c in enumerate(c for c in O.cases() if c.sampling == sampling):
        want = O.encoded(c.name, order)
        clip = _mates(c, order)
        files, got = _encode(clip[1:2], gpu_device, order, c.quality, c.subsampling, fill=(0x00, 0xFF)[k % 2], **c.restart)
        assert files == [want.data], c.name
        assert got["huffman"] == [want.tables] and np.array_equal(_hist(got)[0], want.hist) and np.array_equal(got["ehuff"][0], want.words), c.name
        batch, got = _encode(clip, gpu_device, order, c.quality, c.subsampling, fill=(0xFF, 0x00)[k % 2], **c.restart)
        assert batch[1] == want.data, c.name
        differ += len(set(got["huffman"])) > 1
        if c.w * c.h > 64:              # a noise frame and a flat one never share their tables
            assert len(set(got["huffman"])) >= 2 and len({h[:h.index(b"\xff\xda")] for h in got["headers"]}) >= 2, c.name
        if R.have_turbo():
            assert O.dht_and_tail(files[0]) == O.dht_and_tail(O.pil_encode(c)), c.name
        if order == "rgb":
            # the size condition, which the statement shows to hold for this case: no longer than the standard scan
            std_scan = len(O.dht_and_tail(want.standard)[2])
            assert len(O.dht_and_tail(want.data)[2]) <= std_scan
            standard = jpeg_write.encode_jpeg_device(torch.from_numpy(clip[1:2]).to(gpu_device), order, c.quality, c.subsampling, **c.restart)
            assert standard == [want.standard] and len(O.dht_and_tail(files[0])[2]) <= len(O.dht_and_tail(standard[0])[2]), c.name
    assert differ > 30


def test_the_length_limit_fixture_on_the_device(gpu_device):
    want = O.encoded(O.FIXTURE.name)
    assert want.prelimit[1] == 17
    files, got = _encode(O.FIXTURE.frame()[None], gpu_device, "rgb", 75, "420", fill=0xFF)
    assert np.array_equal(_hist(got)[0], want.hist) and got["huffman"] == [want.tables]
    assert files == [want.data]
    if R.have_turbo():
        assert O.dht_and_tail(files[0]) == O.dht_and_tail(O.pil_encode(O.FIXTURE))


# ----------------------------------------------------------------------------- the histogram buffer
SEGMENT_CASES = [(136, 128, 255), (136, 128, 256), (136, 128, 257), (136, 256, 511), (136, 256, 513)]          # (h, w, restart_mcus), gray


@pytest.mark.parametrize("h,w,mcus", SEGMENT_CASES)
def test_the_histogram_at_segments_around_a_workgroup(gpu_device, h, w, mcus):
    """A gray frame's MCU is a block, so an interval of `mcus` MCUs is a segment of `mcus` blocks: one block short of one
    or two workgroups of 256 lanes, exactly that many, one more; the frame's last segment is short."""
    frame = R.make_content("noise", h, w, 1, 40 + mcus)
    want = O.encode(frame, 75, "420", "rgb", restart_mcus=mcus)
    blocks = (h // 8) * (w // 8)
    assert want.ri == mcus and 0 < blocks % mcus < 40 and blocks // mcus == 1
    seen = []
    for fill in (0x00, 0xFF):
        files, got = _encode(frame[None], gpu_device, "rgb", 75, "420", fill=fill, restart_mcus=mcus)
        assert got["segment_blocks"] == mcus and got["segments"] == 2
        hist = _hist(got)
        assert hist.shape == (1, 2, 272) and np.array_equal(hist[0], want.hist) and not hist[0, 1].any(), fill
        assert files == [want.data], fill
        seen.append(got["hist_buf"].cpu().numpy().tobytes())
    assert seen[0] == seen[1]


@pytest.mark.parametrize("name", ["w37-h53-420", "w37-h53-422", "w40-h56-444", "w17-h33-420"])
def test_the_histogram_of_colour_frames_with_short_last_segments_and_dirty_buffers(gpu_device, name):
    mine = [c for c in O.cases() if c.name.startswith(name) and (c.restart_mcus == 3 or c.restart_rows)]
    assert len(mine) >= 3
    for c in mine:
        want = O.encoded(c.name)
        clip = _mates(c, "rgb")
        mates = [O.encode(clip[i], c.quality, c.subsampling, "rgb", **c.restart).hist for i in (0, 2)]
        for fill in (0x00, 0xFF):
            _, got = _encode(clip, gpu_device, "rgb", c.quality, c.subsampling, fill=fill, **c.restart)
            hist = _hist(got)
            assert np.array_equal(hist[1], want.hist), (c.name, fill)
            assert np.array_equal(hist[0], mates[0]) and np.array_equal(hist[2], mates[1]), (c.name, fill)
    # 37 x 53 in 4:2:0 is 3 x 4 MCUs and in 4:2:2 3 x 7, 17 x 33 in 4:2:0 2 x 3: intervals of 3 MCUs fill them; 40 x 56 in 4:4:4
    # is 5 x 7 = 35 MCUs, whose last interval holds 2
    if name == "w40-h56-444":
        assert any(c.restart_mcus == 3 for c in mine)


def test_the_tally_entry_point_zeroes_the_histogram_itself(gpu_device):
    h = jpeg_write.lib()
    frames = R.make_content("noise", 24, 40, 3, 3)[None]
    clip = torch.from_numpy(frames).to(gpu_device)
    got = jpeg_write._encode_clip(clip, "rgb", 90, "420", "test", optimize=True)
    coef = got["coef_buf"]
    want = O.encode(frames[0], 90, "420", "rgb").hist
    for start in (0, 0x7FFFFFFF, -1):
        hist = torch.full((2 * 272,), start, dtype=torch.int32, device=gpu_device)
        for _ in range(2):              # a second call over its own result counts once, not twice
            jpeg_write.check(h.elvis_jpeg_tally(jpeg_write.ptr(coef), jpeg_write.ptr(hist), 1, 24, 40, 3, 2, 0, None), gpu_device)
        torch.cuda.synchronize(gpu_device)
        assert np.array_equal(hist.cpu().numpy().view(np.uint32).reshape(2, 272).astype(np.int64), want), start
    assert h.elvis_last_launch() == b"jpeg_bits_kernel"
    assert h.elvis_jpeg_tally(jpeg_write.ptr(coef), None, 1, 24, 40, 3, 2, 0, None) == -1 and b"null" in h.elvis_last_error()
    assert h.elvis_jpeg_tally(jpeg_write.ptr(coef), jpeg_write.ptr(hist), 1, 24, 40, 3, 2, 70000, None) == -1 and b"restart_mcus" in h.elvis_last_error()
    assert h.elvis_jpeg_tally(None, None, 0, 24, 40, 3, 2, 0, None) == 0


# ----------------------------------------------------------------------------- combinations
@pytest.mark.parametrize("restart", [{}, dict(restart_rows=1), dict(restart_mcus=3)])
def test_optimize_with_a_map_of_roi_levels_equals_the_statement(gpu_device, restart):
    for c in (c for c in X.cases() if c.map_kind in ("random", "checker30", "all48") and (c.w, c.h) in ((53, 37), (64, 48), (33, 17))):
        want = O.encode(c.frame(), c.quality, c.subsampling, "rgb", levels=c.levels(), B=c.B, **restart)
        files, got = _encode(c.frame()[None], gpu_device, "rgb", c.quality, c.subsampling, levels=c.levels()[None], B=c.B, **restart)
        assert np.array_equal(_hist(got)[0], want.hist), c.name
        assert files == [want.data] and len(files[0]) <= len(want.standard), c.name


def test_optimised_files_decode_to_the_pixels_of_the_standard_ones(gpu_device):
    for shape, sub, q in (((3, 37, 53, 3), "420", 95), ((2, 24, 40, 3), "422", 75), ((2, 40, 56, 3), "444", 50), ((2, 37, 53, 1), "420", 95)):
        frames = np.random.default_rng(shape[2]).integers(0, 256, size=shape, dtype=np.uint8)
        frames[1] = R.make_content("ramp", *shape[1:], 9)
        clip = torch.from_numpy(frames).to(gpu_device)
        plain = jpeg_write.encode_jpeg_device(clip, "bgr", q, sub, restart_rows=1)
        files = jpeg_write.encode_jpeg_device(clip, "bgr", q, sub, restart_rows=1, optimize=True)
        assert files == [O.encode(f, q, sub, "bgr", restart_rows=1).data for f in frames]
        assert all(len(a) < len(b) for a, b in zip(files, plain))
        mine, theirs = jpeg.decode_jpeg_device(files, gpu_device, "bgr", shape[3]), jpeg.decode_jpeg_device(plain, gpu_device, "bgr", shape[3])
        assert torch.equal(mine, theirs)
        for i, (a, b) in enumerate(zip(files, plain)):
            assert np.array_equal(R.decode(a, "bgr", shape[3]).coef, R.decode(b, "bgr", shape[3]).coef), i
            if R.have_turbo():
                assert np.array_equal(R.decode_with_pil(a, "bgr", shape[3]), R.decode_with_pil(b, "bgr", shape[3])), i
                assert np.array_equal(mine[i].cpu().numpy(), R.decode_with_pil(a, "bgr", shape[3])), i
        decoded, nbytes = jpeg_write.jpeg_roundtrip_device(clip, q, sub, restart_rows=1, optimize=True)
        assert torch.equal(decoded, mine) and nbytes.tolist() == [len(f) for f in files]


def test_sizes_with_optimize_are_the_lengths_of_the_files(gpu_device):
    frames = np.random.default_rng(16).integers(0, 256, size=(3, 37, 53, 3), dtype=np.uint8)
    frames[1] = R.make_content("ramp", 37, 53, 3, 17)
    frames[2] = 200
    clip = torch.from_numpy(frames).to(gpu_device)
    levels = np.random.default_rng(18).integers(0, 49, size=(3, 3, 4)).astype(np.uint8)
    for roi in ({}, dict(roi_levels=levels, roi_block_size=16)):
        for restart in ({}, dict(restart_rows=1), dict(restart_mcus=5)):
            for q, sub in ((95, "420"), (40, "444")):
                sizes = jpeg_write.jpeg_encoded_sizes_device(clip, q, sub, "rgb", optimize=True, **restart, **roi)
                files = jpeg_write.encode_jpeg_device(clip, "rgb", q, sub, optimize=True, **restart, **roi)
                assert sizes.dtype == np.int64 and sizes.tolist() == [len(f) for f in files], (roi.keys(), restart, q)
                headers = {f.index(b"\xff\xda") for f in files}
                assert len(headers) > 1                     # the headers differ in length, and the sizes count each
    assert jpeg_write.jpeg_encoded_sizes_device(clip[:0], optimize=True).shape == (0,)
    assert jpeg_write.encode_jpeg_device(clip[:0], optimize=True) == []
    got = jpeg_write._encode_clip(clip, "rgb", 95, "420", "test", guard=GUARD, sizes_only=True, optimize=True)
    assert "out" not in got and "header" not in got and all(_guards_intact(got[k]) for k in BUFFERS[1:])


def test_the_quality_search_with_optimize_fits_and_is_no_lower(gpu_device):
    frames = np.stack([R.make_content("noise", 37, 53, 3, 77), R.make_content("ramp", 37, 53, 3, 78)])
    clip = torch.from_numpy(frames).to(gpu_device)
    std_sizes = X.statement_sizes(frames)
    cache = {}

    def opt_sizes(q):
        if q not in cache:
            cache[q] = np.asarray([len(O.encode(f, q, "420", "bgr").data) for f in frames], np.int64)
        return cache[q]

    std_total, opt_total = (lambda q: int(std_sizes(q).sum())), (lambda q: int(opt_sizes(q).sum()))
    target = std_total(60)
    for top in (100, 95):
        want_std, _, probes_std = X.bisect_transcription(std_total, target, top)
        want_opt, fits, probes_opt = X.bisect_transcription(opt_total, target, top)
        # the premise, from the statement: at every quality either search probes the optimised clip is no larger
        assert all(opt_total(q) <= std_total(q) for q in set(probes_std) | set(probes_opt))
        q, got, ok = jpeg_write.jpeg_quality_for_bytes(clip, target, top, optimize=True)
        assert (q, ok) == (want_opt, fits) and ok and np.array_equal(got, opt_sizes(q)) and int(got.sum()) <= target
        q_std = jpeg_write.jpeg_quality_for_bytes(clip, target, top)[0]
        assert q_std == want_std and q >= q_std and 1 < q_std < top
    decoded, nbytes, q, ok = jpeg_write.jpeg_roundtrip_at_bytes_device(clip, target, optimize=True)
    assert ok and q == X.bisect_transcription(opt_total, target, 95)[0] and np.array_equal(nbytes, opt_sizes(q)) and int(nbytes.sum()) <= target
    again, again_bytes = jpeg_write.jpeg_roundtrip_device(clip, q, optimize=True)
    assert torch.equal(decoded, again) and np.array_equal(nbytes, again_bytes)
    # the hand-off form hands it on
    importance = [np.random.default_rng(5).random((3, 4)) for _ in range(2)]
    levels = handoff.roi_levels_from_importance(importance)
    decoded, nbytes, quality, _ = handoff.encode_with_roi_device(clip, importance, 16, optimize=True)
    want = [O.encode(f, 95, "420", "bgr", levels=m, B=16, restart_rows=1) for f, m in zip(frames, levels)]
    assert quality == 95 and nbytes.tolist() == [len(e.data) for e in want]
    plain = handoff.encode_with_roi_device(clip, importance, 16)
    assert torch.equal(decoded, plain[0]) and plain[1].tolist() == [len(e.standard) for e in want]


def test_saved_files_and_chunks_take_optimize(gpu_device, tmp_path):
    frames = np.random.default_rng(14).integers(0, 256, size=(4, 23, 25, 3), dtype=np.uint8)
    want = [O.encode(f, 95, "420", "bgr", restart_rows=1).data for f in frames]
    paths = [tmp_path / "a" / f"{i}.jpg" for i in range(4)]
    jpeg_write.save_jpeg_frames_device(torch.from_numpy(frames).to(gpu_device), paths, restart_rows=1, optimize=True)
    assert [p.read_bytes() for p in paths] == want
    for chunk in (3, 1, None):              # a frame's bytes depend on that frame alone
        paths = [tmp_path / f"c{chunk}" / f"{i}.jpg" for i in range(4)]
        jpeg_write.save_jpeg_frames(list(frames), paths, str(gpu_device), chunk_frames=chunk, restart_rows=1, optimize=True)
        assert [p.read_bytes() for p in paths] == want, chunk


def test_a_driver_writes_optimised_files_that_pil_opens(gpu_device, tmp_path):
    from PIL import Image
    from elvis_amd.restore import restore_frames_dct_device
    names = [f"{i + 1:05d}.jpg" for i in range(3)]
    plain_dir, opt_dir = str(tmp_path / "plain"), str(tmp_path / "opt")
    for d in (plain_dir, opt_dir):
        rng = np.random.default_rng(31)
        for name in names:
            frameio.save_frame(rng.integers(0, 256, size=(32, 40, 3), dtype=np.uint8), os.path.join(d, name))
    rounds = np.random.default_rng(12).integers(0, 3, size=(3, 4, 5)).astype(np.int32)
    decoded = recompose.frames_to_device([frameio.load_frame(os.path.join(plain_dir, n)) for n in names], gpu_device)
    restored = restore_frames_dct_device(decoded, rounds, 8).contiguous()
    drivers.restore_dct_adaptive(plain_dir, rounds, 8, devices=[gpu_device], jpeg_writer="device")
    drivers.restore_dct_adaptive(opt_dir, rounds, 8, devices=[gpu_device], jpeg_writer="device", jpeg_optimize=True)
    want = jpeg_write.encode_jpeg_device(restored, optimize=True)
    for i, n in enumerate(names):
        data = open(os.path.join(opt_dir, n), "rb").read()
        assert data == want[i] and len(data) < os.path.getsize(os.path.join(plain_dir, n)), n
        with Image.open(io.BytesIO(data)) as img:
            assert img.size == (40, 32) and img.format == "JPEG"
            img.load()
        assert np.array_equal(frameio.load_frame(os.path.join(opt_dir, n)), frameio.load_frame(os.path.join(plain_dir, n))), n
    assert torch.equal(jpeg.load_images_device([os.path.join(opt_dir, n) for n in names], gpu_device),
                       jpeg.load_images_device([os.path.join(plain_dir, n) for n in names], gpu_device))
