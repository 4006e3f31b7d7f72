"""Per-block rate allocation and the byte target of the JPEG writer on the device (csrc/jpeg_write.hip `jpeg_fdct_kernel`
with a map, csrc/jpeg_encode.h, elvis_amd/jpeg_write.py `roi_levels=` / `roi_block_size=`, `jpeg_encoded_sizes_device`,
`jpeg_quality_for_bytes`, elvis_amd/handoff.py `encode_with_roi_device`) against the statement of
tests/_jpeg_roi_ref.py, byte for byte: the ROI corpus in both channel orders with guard bytes around every buffer, a clip
whose frames have maps of their own, no map and a map of zeros against the writer without one, blocks across a workgroup
boundary, a ragged last workgroup with clamped cells, the chroma minimum over 2 x 2 cells, restart intervals, work buffers
that start dirty, the map resident or on the host, the sizes without the files, the quality search, and the round trip."""
import numpy as np
import pytest
import torch

import _jpeg_ref as R
import _jpeg_roi_ref as X
import _jpeg_write_ref as W
import elvis_amd
from elvis_amd import handoff, jpeg_write

pytestmark = pytest.mark.gpu
GUARD = 64
BUFFERS = ("out_buf", "coef_buf", "bits_buf", "words_buf", "ffc_buf", "sizes_buf")
FILLS = (0x00, 0xFF, 0x7F)


def _guards_intact(buf: torch.Tensor) -> bool:
    host = buf.cpu().numpy()
    return bool((host[:GUARD] == 0xA5).all() and (host[-GUARD:] == 0xA5).all())


def _files(got):
    host = got["out"].cpu().numpy()
    off = got["out_off"]
    return [got["header"] + host[int(off[f]):int(off[f + 1])].tobytes() for f in range(off.size - 1)]


def _encode(frames: np.ndarray, levels, B, device, order, quality, subsampling, fill=0, **restart):
    """(files, the dict of jpeg_write._encode_clip) of a host clip with its maps, guards checked."""
    pair = (restart.get("restart_rows", 0), restart.get("restart_mcus", 0))
    got = jpeg_write._encode_clip(torch.from_numpy(np.ascontiguousarray(frames)).to(device), order, quality, subsampling, "test", guard=GUARD, fill=fill,
                                  restart=pair, roi_levels=levels, roi_block_size=B)
    for key in BUFFERS:
        assert _guards_intact(got[key]), key
    return _files(got), got


def _coef(got) -> np.ndarray:
    return got["coef_buf"].cpu().numpy()[GUARD:-GUARD].view(np.int16).reshape(-1, got["blocks"], 64)


def _noise(n, h, w, c, seed) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, c), dtype=np.uint8)


# ----------------------------------------------------------------------------- the corpus
@pytest.mark.parametrize("order", ["bgr", "rgb"])
def test_device_bytes_equal_the_statement(gpu_device, order):
    for k, c in enumerate(X.cases()):
        frame = c.frame()
        if order == "bgr" and c.channels == 3:
            frame = frame[..., ::-1]
        files, got = _encode(frame[None], c.levels()[None], c.B, gpu_device, order, c.quality, c.subsampling, fill=FILLS[(k + (order == "rgb")) % 3])
        want = X.encoded(c.name, order)
        assert np.array_equal(_coef(got)[0], want.blocks), c.name
        assert files == [want.data], c.name


def test_three_frames_with_three_maps_alone_and_in_a_batch(gpu_device):
    frames = _noise(3, 37, 53, 3, 21)
    levels = np.stack([X.make_map(kind, 5, 7, 90 + i) for i, kind in enumerate(("random", "checker30", "corner"))])
    assert len({m.tobytes() for m in levels}) == 3
    want = [X.encode(f, 95, "420", "bgr", m, 8).data for f, m in zip(frames, levels)]
    files, _ = _encode(frames, levels, 8, gpu_device, "bgr", 95, "420")
    assert files == want and len(set(want)) == 3
    for i in range(3):
        assert _encode(frames[i:i + 1], levels[i:i + 1], 8, gpu_device, "bgr", 95, "420")[0] == [want[i]], i
    # the same frame under another frame's map gives other bytes: the map is taken per frame
    assert X.encode(frames[0], 95, "420", "bgr", levels[1], 8).data != want[0]
    swapped, _ = _encode(frames, levels[::-1].copy(), 8, gpu_device, "bgr", 95, "420")
    assert swapped == [X.encode(f, 95, "420", "bgr", m, 8).data for f, m in zip(frames, levels[::-1])] and swapped[1] == want[1]
    assert jpeg_write.encode_jpeg_device(torch.from_numpy(frames).to(gpu_device), roi_levels=levels, roi_block_size=8) == want


# ----------------------------------------------------------------------------- no ROI
def test_no_map_and_a_map_of_zeros_are_the_writer_without_one(gpu_device):
    for shape, sub, q in (((3, 37, 53, 3), "420", 95), ((2, 17, 33, 3), "422", 75), ((2, 48, 64, 3), "444", 50), ((2, 40, 52, 1), "420", 95)):
        frames = _noise(*shape, seed=shape[1])
        clip = torch.from_numpy(frames).to(gpu_device)
        want = [W.encode(f, q, sub, "bgr").data for f in frames]
        assert jpeg_write.encode_jpeg_device(clip, "bgr", q, sub) == want
        assert jpeg_write.encode_jpeg_device(clip, "bgr", q, sub, roi_levels=None, roi_block_size=0) == want
        for B in (8, 16, 32):
            for grid in X.GRIDS:
                by, bx = X.grid_dims(shape[2], shape[1], B, grid)
                assert jpeg_write.encode_jpeg_device(clip, "bgr", q, sub, roi_levels=np.zeros((shape[0], by, bx), np.uint8), roi_block_size=B) == want
    # the dict of the plain call keeps its keys, with and without a map
    frames = _noise(2, 17, 33, 3, 1)
    _, plain = _encode(frames, None, 0, gpu_device, "bgr", 95, "420")
    _, mapped = _encode(frames, np.zeros((2, 2, 4), np.uint8), 8, gpu_device, "bgr", 95, "420")
    assert sorted(plain) == sorted(mapped) == sorted(BUFFERS + ("out", "out_off", "header", "blocks", "chunks"))
    for key in BUFFERS:
        assert torch.equal(plain[key], mapped[key]), key


# ----------------------------------------------------------------------------- block placement
def test_levels_that_differ_across_a_workgroup_boundary(gpu_device):
    """64 x 48 in 4:4:4 has 48 luma blocks and 144 in all, 3 per MCU: a workgroup of 32 blocks ends inside an MCU, and
    every cell has a level of its own."""
    frame = _noise(1, 48, 64, 3, 5)
    levels = (np.arange(48, dtype=np.uint8).reshape(1, 6, 8) * 5 % 49).astype(np.uint8)
    want = X.encode(frame[0], 95, "444", "rgb", levels[0], 8)
    assert len(want.blocks) == 144 and want.block_levels[95] != want.block_levels[96]          # MCU 31's Cr, MCU 32's Y
    assert want.block_levels[30] == want.block_levels[31] == want.block_levels[32] != want.block_levels[33]       # MCU 10 across the boundary
    assert len(set(want.block_levels.tolist())) > 20
    files, got = _encode(frame, levels, 8, gpu_device, "rgb", 95, "444")
    assert np.array_equal(_coef(got)[0], want.blocks) and files == [want.data]
    # gray: 48 blocks, one workgroup and a half
    gray = _noise(1, 48, 64, 1, 6)
    want = X.encode(gray[0], 95, "420", "rgb", levels[0], 8)
    assert len(want.blocks) == 48 and np.array_equal(want.block_levels, levels[0].reshape(-1)) and want.block_levels[31] != want.block_levels[32]
    assert _encode(gray, levels, 8, gpu_device, "rgb", 95, "420")[0] == [want.data]


@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_ragged_last_workgroup_clamped_cells_and_the_floored_grid(gpu_device, sampling):
    """33 x 17 at B = 8: the floored grid is 2 x 4, so the blocks of the fifth column and of the third row take the last
    cell's level, and the frame's blocks do not fill a workgroup."""
    channels = 1 if sampling == "gray" else 3
    sub = "420" if sampling == "gray" else sampling
    frame = _noise(1, 17, 33, channels, 8)
    levels = np.array([[[0, 6, 12, 18], [24, 30, 36, 42]]], np.uint8)
    want = X.encode(frame[0], 95, sub, "bgr", levels[0], 8)
    assert len(want.blocks) % 32 != 0
    luma = want.block_levels[(want.comp == 0) & ~want.dummy]
    assert sorted(set(luma.tolist())) == [0, 6, 12, 18, 24, 30, 36, 42] and (luma == 42).sum() >= 4       # clamped in both axes
    clamped = X.encode(frame[0], 95, sub, "bgr", levels[0], 8, mutant="cell_not_clamped")
    assert clamped.data != want.data
    files, got = _encode(frame, levels, 8, gpu_device, "bgr", 95, sub)
    assert np.array_equal(_coef(got)[0], want.blocks) and files == [want.data]
    # the full grid of the same frame, 3 x 5
    full = (np.arange(15, dtype=np.uint8).reshape(1, 3, 5) * 3).astype(np.uint8)
    assert _encode(frame, full, 8, gpu_device, "bgr", 95, sub)[0] == [X.encode(frame[0], 95, sub, "bgr", full[0], 8).data]
    # one axis floored, the other full
    mixed = (np.arange(10, dtype=np.uint8).reshape(1, 2, 5) * 4).astype(np.uint8)
    assert _encode(frame, mixed, 8, gpu_device, "bgr", 95, sub)[0] == [X.encode(frame[0], 95, sub, "bgr", mixed[0], 8).data]


def test_a_chroma_block_takes_the_minimum_of_its_four_cells(gpu_device):
    frame = _noise(1, 32, 32, 3, 9)
    rng = np.random.default_rng(10)
    for trial in range(4):
        levels = np.zeros((1, 4, 4), np.uint8)
        for y in range(2):
            for x in range(2):
                levels[0, 2 * y:2 * y + 2, 2 * x:2 * x + 2] = rng.permutation(np.array([6, 18, 30, 42], np.uint8)).reshape(2, 2)
        want = X.encode(frame[0], 95, "420", "rgb", levels[0], 8)
        assert (want.block_levels[want.comp > 0] == 6).all() and set(want.block_levels[want.comp == 0].tolist()) == {6, 18, 30, 42}
        for mutant in ("top_left_cell", "max_not_min", "chroma_footprint_in_chroma_pixels"):
            assert X.encode(frame[0], 95, "420", "rgb", levels[0], 8, mutant=mutant).data != want.data, mutant
        files, got = _encode(frame, levels, 8, gpu_device, "rgb", 95, "420")
        assert np.array_equal(_coef(got)[0], want.blocks) and files == [want.data], trial
    # 4:2:2: two cells side by side
    levels = np.tile(np.array([[30, 12], [6, 40]], np.uint8), (2, 2))[None]
    want = X.encode(frame[0], 95, "422", "rgb", levels[0], 8)
    assert set(want.block_levels[want.comp > 0].tolist()) == {12, 6}
    assert _encode(frame, levels, 8, gpu_device, "rgb", 95, "422")[0] == [want.data]


# ----------------------------------------------------------------------------- restart intervals
@pytest.mark.parametrize("restart", [dict(restart_rows=1), dict(restart_mcus=3)])
def test_restart_intervals_combine_with_a_map(gpu_device, restart):
    for c in (c for c in X.cases() if c.map_kind in ("random", "checker30") and (c.w, c.h) in ((53, 37), (64, 48), (33, 17))):
        files, got = _encode(c.frame()[None], c.levels()[None], c.B, gpu_device, "rgb", c.quality, c.subsampling, **restart)
        want = X.encode(c.frame(), c.quality, c.subsampling, "rgb", c.levels(), c.B, **restart)
        assert want.ri > 0 and got["restart_interval"] == want.ri, c.name
        assert files == [want.data], c.name


# ----------------------------------------------------------------------------- dirty buffers, resident maps
@pytest.mark.parametrize("name", ["w53-h37-420-q75-noise-b32floor-checker30", "w64-h48-444-q95-checker-b16floor-random"])
def test_work_buffers_that_start_dirty_give_the_same_bytes(gpu_device, name):
    c = X.case(name)
    want = X.encoded(c.name)
    seen = []
    for fill in FILLS:
        for restart in ({}, dict(restart_rows=1)):
            files, got = _encode(c.frame()[None], c.levels()[None], c.B, gpu_device, "rgb", c.quality, c.subsampling, fill=fill, **restart)
            if not restart:
                assert files == [want.data], fill
                seen.append(tuple(got[key].cpu().numpy()[GUARD:-GUARD].tobytes() for key in ("coef_buf", "bits_buf", "ffc_buf", "sizes_buf", "out_buf")))
            else:
                assert files == [X.encode(c.frame(), c.quality, c.subsampling, "rgb", c.levels(), c.B, **restart).data], fill
    assert seen[0] == seen[1] == seen[2]


def test_a_resident_map_and_a_host_map_give_the_same_bytes(gpu_device):
    frames = _noise(3, 40, 52, 3, 12)
    clip = torch.from_numpy(frames).to(gpu_device)
    levels = np.random.default_rng(13).integers(0, 49, size=(3, 3, 4)).astype(np.uint8)
    want = [X.encode(f, 95, "420", "bgr", m, 16).data for f, m in zip(frames, levels)]
    resident = torch.from_numpy(levels).to(gpu_device)
    assert jpeg_write.encode_jpeg_device(clip, roi_levels=levels, roi_block_size=16) == want
    assert jpeg_write.encode_jpeg_device(clip, roi_levels=resident, roi_block_size=16) == want
    assert jpeg_write.encode_jpeg_device(clip, roi_levels=torch.from_numpy(levels), roi_block_size=16) == want
    assert torch.equal(resident.cpu(), torch.from_numpy(levels))          # the map is read, never written
    with pytest.raises(ValueError, match="contiguous"):
        jpeg_write.encode_jpeg_device(clip, roi_levels=torch.from_numpy(np.zeros((3, 3, 8), np.uint8)).to(gpu_device)[:, :, ::2], roi_block_size=16)
    with pytest.raises(ValueError, match="above 48"):
        jpeg_write.encode_jpeg_device(clip, roi_levels=torch.full((3, 3, 4), 49, dtype=torch.uint8, device=gpu_device), roi_block_size=16)


def test_saved_files_take_the_map(gpu_device, tmp_path):
    frames = _noise(4, 23, 25, 3, 14)
    levels = np.random.default_rng(15).integers(0, 49, size=(4, 3, 4)).astype(np.uint8)
    want = [X.encode(f, 95, "420", "bgr", m, 8, restart_rows=1).data for f, m in zip(frames, levels)]
    paths = [tmp_path / "a" / f"{i}.jpg" for i in range(4)]
    jpeg_write.save_jpeg_frames_device(torch.from_numpy(frames).to(gpu_device), paths, restart_rows=1, roi_levels=levels, roi_block_size=8)
    assert [p.read_bytes() for p in paths] == want
    for chunk in (3, None):
        paths = [tmp_path / f"c{chunk}" / f"{i}.jpg" for i in range(4)]
        elvis_amd.save_jpeg_frames(list(frames), paths, str(gpu_device), chunk_frames=chunk, restart_rows=1, roi_levels=levels, roi_block_size=8)
        assert [p.read_bytes() for p in paths] == want, chunk


# ----------------------------------------------------------------------------- sizes and the search
def test_sizes_are_the_lengths_of_the_files(gpu_device):
    frames = _noise(3, 37, 53, 3, 16)
    frames[1] = R.make_content("ramp", 37, 53, 3, 17)
    clip = torch.from_numpy(frames).to(gpu_device)
    levels = np.random.default_rng(18).integers(0, 49, size=(3, 3, 4)).astype(np.uint8)
    for roi in ({}, dict(roi_levels=levels, roi_block_size=16)):
        for restart in ({}, dict(restart_rows=1), dict(restart_mcus=5)):
            for q, sub in ((95, "420"), (40, "444")):
                sizes = jpeg_write.jpeg_encoded_sizes_device(clip, q, sub, "rgb", **restart, **roi)
                files = jpeg_write.encode_jpeg_device(clip, "rgb", q, sub, **restart, **roi)
                assert sizes.dtype == np.int64 and sizes.tolist() == [len(f) for f in files], (roi.keys(), restart, q)
                if roi:
                    assert sizes.tolist() == [len(X.encode(f, q, sub, "rgb", m, 16, **restart).data) for f, m in zip(frames, levels)]
    assert jpeg_write.jpeg_encoded_sizes_device(clip[:0]).shape == (0,)
    gray = torch.from_numpy(_noise(2, 24, 40, 1, 19)).to(gpu_device)
    assert jpeg_write.jpeg_encoded_sizes_device(gray, 75).tolist() == [len(f) for f in jpeg_write.encode_jpeg_device(gray, quality=75)]
    # the size query runs no stuffing pass and makes no output buffer
    got = jpeg_write._encode_clip(clip, "rgb", 95, "420", "test", guard=GUARD, sizes_only=True)
    assert "out" not in got and "out_buf" not in got and all(_guards_intact(got[k]) for k in BUFFERS[1:])


def test_the_quality_search_equals_the_transcription_on_the_statements_sizes(gpu_device):
    frames = np.stack([R.make_content("noise", 37, 53, 3, 77), R.make_content("ramp", 37, 53, 3, 78)])
    clip = torch.from_numpy(frames).to(gpu_device)
    levels = np.stack([X.make_map("random", 3, 4, 79), X.make_map("checker30", 3, 4, 80)])
    for roi, kw in (({}, {}), (dict(levels=levels, B=16), dict(roi_levels=levels, roi_block_size=16))):
        sizes = X.statement_sizes(frames, "420", **roi)
        total = lambda q: int(sizes(q).sum())
        target = total(60)
        for top in (100, 95):
            q, got, fits = jpeg_write.jpeg_quality_for_bytes(clip, target, top, **kw)
            want_q, want_fits, _ = X.bisect_transcription(total, target, top)
            assert (q, fits) == (want_q, want_fits) and fits and 1 < q < top, (roi.keys(), top)
            assert np.array_equal(got, sizes(q)) and int(got.sum()) <= target
        q, got, fits = jpeg_write.jpeg_quality_for_bytes(clip, total(1) - 1, **kw)
        assert (q, fits) == (1, False) and np.array_equal(got, sizes(1))
        decoded, nbytes, q, fits = jpeg_write.jpeg_roundtrip_at_bytes_device(clip, target, **kw)
        assert fits and q == X.bisect_transcription(total, target, 95)[0] and np.array_equal(nbytes, sizes(q)) and int(nbytes.sum()) <= target
        again, again_bytes = jpeg_write.jpeg_roundtrip_device(clip, q, **kw)
        assert torch.equal(decoded, again) and np.array_equal(nbytes, again_bytes)


# ----------------------------------------------------------------------------- the round trip
def test_round_trip_with_a_map_gives_the_pixels_pil_decodes(gpu_device):
    for shape, sub, q, B in (((3, 37, 53, 3), "420", 95, 8), ((2, 24, 40, 3), "422", 75, 16), ((2, 37, 53, 1), "420", 95, 32)):
        frames = _noise(*shape, seed=shape[2])
        clip = torch.from_numpy(frames).to(gpu_device)
        by, bx = X.grid_dims(shape[2], shape[1], B, "ceil")
        levels = np.random.default_rng(B).integers(0, 37, size=(shape[0], by, bx)).astype(np.uint8)
        for restart in ({}, dict(restart_rows=1)):
            decoded, nbytes = jpeg_write.jpeg_roundtrip_device(clip, q, sub, roi_levels=levels, roi_block_size=B, **restart)
            files = jpeg_write.encode_jpeg_device(clip, "bgr", q, sub, roi_levels=levels, roi_block_size=B, **restart)
            assert files == [X.encode(f, q, sub, "bgr", m, B, **restart).data for f, m in zip(frames, levels)]
            assert nbytes.tolist() == [len(f) for f in files] and tuple(decoded.shape) == shape
            host = decoded.cpu().numpy()
            for i, f in enumerate(files):
                assert np.array_equal(host[i], R.decode(f, "bgr", shape[3]).pixels), (shape, i)
                if R.have_turbo():
                    assert np.array_equal(host[i], R.decode_with_pil(f, "bgr", shape[3])), (shape, i)
        plain, plain_bytes = jpeg_write.jpeg_roundtrip_device(clip, q, sub)
        assert not torch.equal(plain, decoded) and int(nbytes.sum()) < int(plain_bytes.sum())


def test_encode_with_roi_device_is_the_two_steps_done_by_hand(gpu_device):
    frames = _noise(3, 48, 64, 3, 30)
    frames[2] = R.make_content("ramp", 48, 64, 3, 31)
    clip = torch.from_numpy(frames).to(gpu_device)
    rng = np.random.default_rng(32)
    importance = [rng.random((3, 4)) for _ in range(3)]
    importance[0][0, 0], importance[1][2, 3] = 1.0, 0.0
    levels = handoff.roi_levels_from_importance(importance)
    assert levels.shape == (3, 3, 4) and levels.min() == 0 and levels.max() == 28
    decoded, nbytes, quality, got_levels = elvis_amd.encode_with_roi_device(clip, importance, 16)
    assert quality == 95 and np.array_equal(got_levels, levels) and got_levels.dtype == np.uint8
    by_hand, by_hand_bytes = jpeg_write.jpeg_roundtrip_device(clip, 95, "420", "bgr", restart_rows=1, roi_levels=levels, roi_block_size=16)
    assert torch.equal(decoded, by_hand) and np.array_equal(nbytes, by_hand_bytes)
    want = [X.encode(f, 95, "420", "bgr", m, 16, restart_rows=1).data for f, m in zip(frames, levels)]
    assert nbytes.tolist() == [len(f) for f in want]
    assert np.array_equal(decoded.cpu().numpy()[1], R.decode(want[1], "bgr", 3).pixels)
    # with a budget: the search inside 1..quality, then the same round trip
    target = int(sum(len(X.encode(f, 70, "420", "bgr", m, 16, restart_rows=1).data) for f, m in zip(frames, levels)))
    decoded, nbytes, quality, got_levels = handoff.encode_with_roi_device(clip, importance, 16, quality=90, target_bytes=target)
    q, sizes, fits = jpeg_write.jpeg_quality_for_bytes(clip, target, 90, restart_rows=1, roi_levels=levels, roi_block_size=16)
    assert fits and quality == q and 1 < q <= 90 and np.array_equal(nbytes, sizes) and int(nbytes.sum()) <= target
    by_hand, _ = jpeg_write.jpeg_roundtrip_device(clip, q, restart_rows=1, roi_levels=levels, roi_block_size=16)
    assert torch.equal(decoded, by_hand) and np.array_equal(got_levels, levels)
    # other options go through
    decoded, nbytes, quality, _ = handoff.encode_with_roi_device(clip, importance, 16, quality=60, subsampling="444", order="rgb", restart_rows=0, base_qp=48)
    lv48 = handoff.roi_levels_from_importance(importance, base_qp=48)
    assert lv48.max() == 17 and nbytes.tolist() == [len(X.encode(f, 60, "444", "rgb", m, 16).data) for f, m in zip(frames, lv48)]


def test_the_new_names_are_exported():
    for name in ("JPEG_ROI_MAX_LEVEL", "jpeg_roi_scale16", "jpeg_roi_levels", "jpeg_encoded_sizes_device", "jpeg_quality_for_bytes",
                 "jpeg_roundtrip_at_bytes_device"):
        assert getattr(elvis_amd, name) is getattr(jpeg_write, name), name
    for name in ("roi_levels_from_importance", "encode_with_roi_device"):
        assert getattr(elvis_amd, name) is getattr(handoff, name), name
