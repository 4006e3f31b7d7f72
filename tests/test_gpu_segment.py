"""The foreground segmenter on the device (csrc/segment.hip) against its numpy statement (tests/_segment_ref.py): the
masks and every intermediate of the workspace, byte for byte.  The references are computed once and never modified."""
import numpy as np
import pytest
import torch

import _segment_ref as R
import elvis_amd
from elvis_amd import _lib, drivers, frameio, segment

pytestmark = pytest.mark.gpu

STAGES = ("red", "sad", "shift", "M", "S", "Mn", "Sn", "F", "thr", "pre")


SAD_TY, SAD_TX, TILE, MORPH = R.kernel_tiles()
TILE_EDGES = R.tile_edges()
CASES = R.cases(TILE_EDGES)
_expected = {}


def expected(name):
    """The statement's (masks, details) of a case, computed once; read-only."""
    if name not in _expected:
        frames, order, kw = CASES[name]
        masks, det = R.segment(frames, order, R.SegmentConfig(**kw), details=True)
        masks.setflags(write=False)
        for a in det.values():
            a.setflags(write=False)
        _expected[name] = (masks, det)
    return _expected[name]


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)           # a copy: the shared references are read-only


def _same(name, got, ref):
    got = got.cpu().numpy().astype(np.int64)
    assert got.shape == ref.shape, f"{name}: shape {got.shape}, the statement's {ref.shape}"
    diff = got != ref
    assert not diff.any(), (f"{name}: {int(diff.sum())} of {diff.size} differ, first at {tuple(np.argwhere(diff)[0])}: "
                            f"{got[diff][0]} against the statement's {ref[diff][0]}")


def _compare(name, masks, det, ref_masks, ref_det):
    for stage in STAGES:                                   # in the order of the pipeline: the first wrong stage is named
        _same(f"{name} {stage}", det[stage], ref_det[stage])
    assert masks.dtype == torch.uint8
    _same(f"{name} masks", masks, ref_masks.astype(np.int64))


def test_the_case_list_covers_the_matrix_and_the_forced_branches():
    shapes = {f.shape[1:3] for f, o, k in CASES.values()}
    assert {(20, 20), (21, 23), (22, 27), (48, 64), (72, 130)} <= shapes and set(TILE_EDGES.values()) <= shapes
    assert (21 * 3) % 4 and (23 * 3) % 4 and (27 * 3) % 4                              # rows that are no whole dwords
    for hw in ((20, 20), (21, 23), (22, 27), (48, 64)):
        assert {f.shape[0] for f, o, k in CASES.values() if f.shape[1:3] == hw} >= {1, 2, 3, 5}
    assert {f.shape[3] for f, o, k in CASES.values()} == {1, 3} and {o for f, o, k in CASES.values()} == {"rgb", "bgr"}
    assert {(k.get("dilation", 1), k.get("temporal_vote", True)) for f, o, k in CASES.values()} >= {
        (d, v) for d in (0, 1, 4) for v in (False, True)}
    assert any(k["radius"] == 8 and f.shape[1:3] == (72, 130) for f, o, k in CASES.values())
    assert all(f.dtype == np.uint8 and f.shape[1] <= 136 and f.shape[2] <= 284 and f.shape[0] <= 5 for f, o, k in CASES.values())
    # a second tile exactly where the names say, none one reduced pixel earlier
    assert TILE_EDGES["sad_rows"][0] // 4 - 4 == SAD_TY + 1 and TILE_EDGES["sad_columns"][1] // 4 - 4 == SAD_TX + 1
    assert TILE_EDGES["terms_fuse_rows"][0] // 4 == TILE + 1 and TILE_EDGES["morph_columns"][1] // 4 == MORPH + 1
    # the forced branches, on the statement
    masks, det = expected("flat_40x52_n3")
    assert not det["sad"].any() and not det["shift"].any() and (det["thr"] == 255).all() and masks.all()
    masks, det = expected("framed_48x64_n3")
    share = det["pre"].reshape(3, -1).mean(axis=1)
    assert (share > 0.7).all() and (share < 1).all() and masks.all()                   # above max_share: all ones
    masks, det = expected("quiet_48x64_n3")
    assert 0 < det["M"].max() < 864 and 0 < det["S"].max() < 384
    for name, r in (("shift_plus_r_minus_r_48x64_n3", 2), ("shift_plus_r_minus_r_r8_100x112_n2", 8)):
        assert expected(name)[1]["shift"][1:].tolist() == [[r, -r]] * (len(CASES[name][0]) - 1)
    # and the ordinary cases have a mask that is neither empty nor full
    for name in ("48x64_n5", "72x130_r8_n3", "all_tiles_133x282_n3", "21x23_n3"):
        m = expected(name)[0]
        assert 0 < m.mean() < 1, name


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_statement_byte_for_byte(gpu_device, name):
    frames, order, kw = CASES[name]
    ref_masks, ref_det = expected(name)
    fd = _dev(frames, gpu_device)
    masks, det = elvis_amd.foreground_masks_device(fd, order, segment.SegmentConfig(**kw), details=True)
    assert _lib.lib().elvis_last_launch().decode() == "seg_upsample_kernel"
    _compare(name, masks, det, ref_masks, ref_det)
    assert np.array_equal(fd.cpu().numpy(), frames)                                    # the input is not written
    plain = elvis_amd.foreground_masks_device(fd, order, segment.SegmentConfig(**kw))
    assert isinstance(plain, torch.Tensor) and torch.equal(plain, masks)


@pytest.mark.parametrize("name", sorted(CASES))
def test_strip_means_and_votes_equal_the_statement(gpu_device, name):
    """The two work buffers STAGES leaves out: `means`, the border strips' mean colours (seg_strips_kernel's only output),
    and `voted`, the masks after the temporal vote with `count`, their set pixels (seg_vote_kernel's)."""
    frames, order, kw = CASES[name]
    cfg = R.SegmentConfig(**kw)
    _, ref = expected(name)
    _, det = elvis_amd.foreground_masks_device(_dev(frames, gpu_device), order, segment.SegmentConfig(**kw), details=True)
    m = frames.shape[0]
    _same(f"{name} means", det["means"], np.stack([R.strip_means(ref["red"][e]) for e in range(m)]))
    voted = np.stack([R.vote(ref["pre"], e, m) if cfg.temporal_vote else ref["pre"][e] for e in range(m)])
    _same(f"{name} voted", det["voted"], voted)
    _same(f"{name} count", det["count"], voted.reshape(m, -1).sum(axis=1))


def _scene(n):
    pan, move, noise = R.SCENES["pan_4_8_obj_0_8"]
    frames, boxes = R.scene(pan, move, noise)
    frames, boxes = frames[:n], boxes[:n]
    masks, det = R.segment(frames, details=True)
    for a in (frames, masks):
        a.setflags(write=False)
    return frames, boxes, masks, det


@pytest.fixture(scope="module")
def scene6():
    """The second scene of the host test (a pan of (4, 8), the object moving by (0, 8), noise 2), its six frames, and
    the statement's masks of them."""
    return _scene(6)


@pytest.fixture(scope="module")
def scene5():
    """The first five frames of that scene as a clip of their own."""
    return _scene(5)


def test_the_scene_meets_its_conditions_on_the_device(gpu_device, scene6):
    frames, boxes, ref, ref_det = scene6
    masks, det = elvis_amd.foreground_masks_device(_dev(frames, gpu_device), details=True)
    got = masks.cpu().numpy()
    inside_ok, far_ok = R.scene_conditions(got, boxes)
    assert inside_ok, "a block wholly inside the object is background"
    assert far_ok, "a block two or more blocks away from the object is foreground"
    assert det["shift"].cpu().tolist() == [[-1, -2]] + [[1, 2]] * 5
    _compare("scene", masks, det, ref, ref_det)


def test_the_result_does_not_depend_on_how_the_clip_is_cut(gpu_device, scene5):
    frames, boxes, ref, _ = scene5
    whole = elvis_amd.foreground_masks_device(_dev(frames, gpu_device))
    assert np.array_equal(whole.cpu().numpy(), ref)
    for k in (1, 2, 5, None):
        for arg in ((frames, [f for f in frames]) if k == 2 else (frames,)):
            got = elvis_amd.segment_frames(arg, device=str(gpu_device), chunk_frames=k)
            assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (5, 240, 320)
            assert np.array_equal(got, ref), f"chunk_frames={k}: {int((got != ref).sum())} bytes differ"
    # the middle frames alone, with the frames around them as halo
    fd = _dev(frames, gpu_device)
    for a, b in ((1, 4), (2, 4), (2, 3), (1, 2), (0, 2), (3, 5)):
        lo = max(0, a - 2)
        part = elvis_amd.foreground_masks_device(fd[a:b], before=fd[lo:a] if a > lo else None, after=fd[b:b + 1] if b < 5 else None)
        assert torch.equal(part, whole[a:b]), (a, b)
    # without the halo a middle frame is treated as a first frame: the halo is what makes the cut invisible
    assert not torch.equal(elvis_amd.foreground_masks_device(fd[2:4]), whole[2:4])
    # the statement takes the halo the same way
    assert np.array_equal(R.segment(frames[2:4], before=frames[0:2], after=frames[4:5]), ref[2:4])


def test_bgr_frames_and_one_channel_through_segment_frames(gpu_device, scene5):
    frames, boxes, ref, _ = scene5
    bgr = np.ascontiguousarray(frames[..., ::-1])
    assert np.array_equal(elvis_amd.segment_frames(bgr, device=str(gpu_device), order="bgr"), ref)
    gray = frames[..., 1]
    want = R.segment(gray[..., None])
    assert np.array_equal(elvis_amd.segment_frames(gray, device=str(gpu_device)), want)


def test_the_driver_is_segment_frames_then_the_existing_function(gpu_device, scene5):
    frames, boxes, ref, _ = scene5
    bgr = np.ascontiguousarray(frames[..., ::-1])
    dev = str(gpu_device)
    scores, masks = drivers.calculate_removability_scores_device(bgr, 16, device=dev, return_masks=True)
    assert np.array_equal(masks, ref) and np.array_equal(masks, elvis_amd.segment_frames(bgr, device=dev, order="bgr"))
    assert scores.dtype == np.float64 and scores.shape == (5, 15, 20)
    fed = drivers.calculate_removability_scores_from_frames(bgr, list(masks), 16, device=dev)
    assert np.array_equal(scores, fed)
    assert np.array_equal(elvis_amd.calculate_removability_scores_device(bgr, 16, device=dev, chunk_frames=2), scores)
    none = drivers.calculate_removability_scores_from_frames(bgr, None, 16, device=dev)
    assert none.shape == scores.shape and not np.array_equal(scores, none)
    alpha = drivers.calculate_removability_scores_device(bgr, 16, 0.25, 0.5, device=dev)
    assert np.array_equal(alpha, drivers.calculate_removability_scores_from_frames(bgr, list(masks), 16, 0.25, 0.5, device=dev))


def test_mask_files_round_trip_through_frameio(gpu_device, scene5, tmp_path):
    frames, boxes, ref, _ = scene5
    masks = elvis_amd.segment_frames(frames[:3], device=str(gpu_device))
    elvis_amd.save_foreground_masks(masks, tmp_path / "ufo_masks")
    paths = frameio.get_frame_paths(tmp_path / "ufo_masks")
    assert [p.name for p in paths] == ["00001.png", "00002.png", "00003.png"]
    for i, p in enumerate(paths):
        back = frameio.load_frame(p)                        # BGR, three equal channels of 0 / 255
        assert (back[..., 0] == back[..., 1]).all() and (back[..., 1] == back[..., 2]).all()
        assert np.array_equal(back[..., 0], masks[i] * 255)
        assert np.array_equal((back[..., 0] > 0).astype(np.uint8), masks[i])           # as elvis.py:1191 reads it back
