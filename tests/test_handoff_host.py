"""The encoder hand-off without a GPU: the conversion's constants and range, the block-grid rules and both file formats
against the reference's own output (tests/golden/handoff.npz, tools/make_handoff_golden.py), the Y4M header, the ABI."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import _handoff_ref as R
from elvis_amd import _lib, handoff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "handoff.npz"))


def _take(z, key, at, item, count):
    """The next `count` values of the flat float32 / float64 array `key`; `at` keeps the two cursors."""
    part = z[f"{key}_f{item}"][at[item]:at[item] + count]
    at[item] += count
    return part


# ----------------------------------------------------------------------------- the conversion's constants
def test_constant_identities():
    """The constants are written from memory of OpenCV's source; these identities are what holds them.  Pure green is
    Y 145, not the 144 the feature request quotes: 528482 * 255 + (1 << 19) + (16 << 20) = 152 064 414 = 145.02 * 2^20,
    and (145, 54, 34) is the BT.601 studio triple of green (16 + 128.553 = 144.553 rounds up) - the quoted figure
    contradicts the quoted coefficients, whose other identities (sums, black, white, red, blue) all hold."""
    assert sum(R.Y_ROW) == 900726
    assert sum(R.U_ROW) == 1 and sum(R.V_ROW) == 1
    px = np.asarray([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
    y, u, v = R.yuv_of(px)
    assert (y[0], u[0], v[0]) == (16, 128, 128) and (y[1], u[1], v[1]) == (235, 128, 128)
    assert y[2:].tolist() == [82, 145, 41]                      # BT.601 studio swing
    assert (u[2], v[2]) == (90, 240) and (u[3], v[3]) == (54, 34) and (u[4], v[4]) == (240, 110)


def test_every_colour_stays_in_range_and_in_int32():
    """No output leaves [16, 240] over all 2^24 colours (saturate_cast never fires), and no sum leaves int32."""
    c = np.arange(1 << 24, dtype=np.int64)
    rgb = np.stack([c >> 16, (c >> 8) & 255, c & 255], axis=-1)
    y, u, v = R.yuv_of(rgb)
    assert (y.min(), y.max()) == (16, 235)
    assert (u.min(), u.max()) == (16, 240) and (v.min(), v.max()) == (16, 240)
    for row, bias in ((R.Y_ROW, 16), (R.U_ROW, 128), (R.V_ROW, 128)):
        offset = (1 << 19) + (bias << 20)
        assert 0 <= 255 * sum(k for k in row if k < 0) + offset and 255 * sum(k for k in row if k > 0) + offset < 2 ** 31


def test_chroma_is_sampled_not_averaged():
    frame = np.zeros((1, 2, 2, 3), np.uint8)
    frame[0, 0, 0] = (255, 0, 0)
    planes = R.rgb_to_i420(frame).reshape(-1)
    assert planes.tolist() == [82, 16, 16, 16, 90, 240]
    assert R.rgb_to_i420(frame[..., ::-1].copy(), "bgr").reshape(-1).tolist() == planes.tolist()


# ----------------------------------------------------------------------------- the golden
def test_importance_scores_match_the_reference(g):
    at = {k: {4: 0, 8: 0} for k in ("sc", "tc", "mask", "score")}
    flat_frames = 0
    for (count, by, bx, item), (alpha, beta) in zip(g["importance_params"], g["importance_alpha_beta"]):
        sc, tc, masks, want = (_take(g, f"importance_{k}", at[k], item, count * by * bx).reshape(count, by, bx)
                               for k in ("sc", "tc", "mask", "score"))
        keep = masks.copy()
        got = handoff.calculate_importance_scores(None, 16, float(alpha), float(beta), SimpleNamespace(SC=sc, TC=tc), masks)
        assert isinstance(got, list) and len(got) == count
        assert np.array_equal(masks, keep), "the caller's masks were written"
        got = np.stack(got)
        assert got.dtype == want.dtype and np.array_equal(got, want)
        ref = R.calculate_importance_scores(float(alpha), float(beta), sc, tc, masks)
        assert ref.dtype == want.dtype and np.array_equal(ref, want)
        flat_frames += int(np.ptp(want[0]) == 0)
    assert flat_frames >= 2 and {int(p[0]) for p in g["importance_params"]} >= {1, 2}
    assert {0.0, 0.5, 1.0} <= set(np.unique(g["importance_mask_f8"]).tolist()) and np.float32(0.49999) in g["importance_mask_f4"]


def test_kvazaar_roi_matches_the_reference(g, tmp_path):
    at, pos = {4: 0, 8: 0}, 0
    seen = set()
    for base_qp, qp_range, by, bx, item, size in g["kvazaar_params"]:
        frames = [_take(g, "kvazaar_importance", at, item, by * bx).reshape(by, bx), _take(g, "kvazaar_importance", at, item, 6).reshape(2, 3)]
        want = g["kvazaar_files"][pos:pos + size].tobytes()
        pos += size
        path = str(tmp_path / "roi.bin")
        handoff.create_kvazaar_roi_file(frames, path, int(base_qp), int(qp_range))
        assert open(path, "rb").read() == want
        assert R.kvazaar_roi_bytes(frames, int(base_qp), int(qp_range)) == want
        delta = handoff.kvazaar_delta_qp(frames[0], int(base_qp), int(qp_range))
        assert delta.dtype == np.int8 and delta.shape == (by, bx)
        assert np.frombuffer(want[:8], "<i4").tolist() == [bx, by] and want[8:8 + by * bx] == delta.tobytes()
        seen |= {(int(base_qp), int(v)) for v in (delta.min(), delta.max())}
    assert pos == g["kvazaar_files"].size
    # both clips bite: +-14 where the HEVC range allows it, 0 - base_qp and 51 - base_qp where it does not
    assert {(30, -14), (30, 14), (5, -5), (5, 14), (48, -14), (48, 3)} <= seen


def test_kvazaar_cut_is_toward_zero():
    imp = np.asarray([[0.5 + 0.9 / 30, 0.5 - 0.9 / 30, 0.5 + 1.9 / 30, 0.5 - 1.9 / 30]])
    assert handoff.kvazaar_delta_qp(imp, 30).tolist() == [[0, 0, -1, 1]]
    assert handoff.kvazaar_delta_qp(imp.astype(np.float32), 30).tolist() == [[0, 0, -1, 1]]


def test_svtav1_roi_matches_the_reference(g, tmp_path):
    at, pos = {4: 0, 8: 0}, 0
    ratios = set()
    for by, bx, width, height, base_crf, qp_range, count, item, size in g["svtav1_params"]:
        grids = [_take(g, "svtav1_importance", at, item, by * bx).reshape(by, bx) for _ in range(count)]
        want = g["svtav1_files"][pos:pos + size].tobytes()
        pos += size
        path = str(tmp_path / "roi.txt")
        args = (int(base_crf), int(qp_range), int(width), int(height))
        handoff.create_svtav1_roi_file(grids, path, *args)
        assert open(path, "rb").read() == want
        assert R.svtav1_roi_text(grids, *args).encode() == want
        rows, cols = -(-height // 64), -(-width // 64)
        for i, (line, grid) in enumerate(zip(want.decode().splitlines(), grids)):
            delta = handoff.svtav1_delta_qp(grid, *args)
            assert delta.shape == (rows, cols) and np.issubdtype(delta.dtype, np.integer)
            assert [int(t) for t in line.split()] == [i] + delta.reshape(-1).tolist()
            assert R.svtav1_levels_margin(grid, width, height) >= 1e-4          # the unpinned resize cannot flip a level
            assert np.array_equal(handoff.resize_area_f32(grid, cols, rows), R.resize_area_f32(grid, cols, rows))
        ratios.add((by % rows == 0 and bx % cols == 0, (by, bx, rows, cols)))
    assert pos == g["svtav1_files"].size
    assert (True, (32, 64, 8, 16)) in ratios and (False, (67, 120, 17, 30)) in ratios


def test_svtav1_grid_must_be_larger_than_the_superblock_grid():
    for shape in ((17, 120), (67, 30), (8, 8)):
        with pytest.raises(ValueError):
            handoff.svtav1_delta_qp(np.zeros(shape, np.float32), 35, 15, 1920, 1080)


def test_resize_area_f32_by_hand():
    """3 -> 2 along x (cells of 1.5: weights 2/3, 1/3) and 4 -> 2 along y, a flat grid and a whole-ratio mean."""
    grid = np.asarray([[0, 3, 6]] * 4, np.float32)
    assert np.allclose(handoff.resize_area_f32(grid, 2, 2), [[1, 5], [1, 5]], atol=1e-6)
    assert np.array_equal(handoff.resize_area_f32(np.full((5, 7), 0.25, np.float32), 3, 2), R.resize_area_f32(np.full((5, 7), 0.25, np.float32), 3, 2))
    assert handoff.resize_area_f32(np.arange(16, dtype=np.float32).reshape(4, 4), 2, 2).tolist() == [[2.5, 4.5], [10.5, 12.5]]


def test_y4m_matches_the_reference(g):
    frames = list(g["y4m_frames"])
    pos = 0
    for rate, size in zip(g["y4m_framerates"], g["y4m_sizes"]):
        want = g["y4m_files"][pos:pos + size].tobytes()
        pos += size
        assert R.y4m_bytes(frames, float(rate)) == want
        h, w = frames[0].shape[:2]
        head = handoff.y4m_header(w, h, float(rate))
        assert want.startswith(head) and want[len(head):len(head) + 6] == b"FRAME\n"
        assert len(want) == len(head) + len(frames) * (6 + h * w * 3 // 2)
    assert R.yuv420p_bytes(frames) == b"".join(want[len(head) + i * (6 + 90) + 6:len(head) + (i + 1) * (6 + 90)] for i in range(len(frames)))


@pytest.mark.parametrize("rate,text", [(30, b"F30000:1000"), (29.97, b"F29970:1000"), (23.976, b"F23976:1000")])
def test_y4m_header(rate, text):
    want = b"YUV4MPEG2 W1920 H1080 " + text + b" Ip A1:1 C420\n"
    assert handoff.y4m_header(1920, 1080, rate) == want and R.y4m_header(1920, 1080, rate) == want


def test_default_chunk_is_a_few_tens_of_megabytes():
    assert handoff._chunk_frames((1080, 1920, 3), None) == 10
    assert handoff._chunk_frames((2, 2, 3), None) * 6 <= handoff.I420_CHUNK_BYTES
    assert handoff._chunk_frames((4320, 7680, 3), None) == 1 and handoff._chunk_frames((1080, 1920, 3), 3) == 3
    with pytest.raises(ValueError):
        handoff._chunk_frames((1080, 1920, 3), 0)


# ----------------------------------------------------------------------------- the ABI and the exports
def test_abi_symbol(built_lib):
    import elvis_amd
    header = open(os.path.join(ROOT, "include", "elvis_amd.h")).read()
    m = re.search(r"int\s+elvis_rgb_to_i420_u8\s*\(([^;]*)\)\s*;", header)
    assert m and len(m.group(1).split(",")) == 7 == len(_lib.SIGNATURES["elvis_rgb_to_i420_u8"])
    h = _lib.lib()
    assert hasattr(h, "elvis_rgb_to_i420_u8")
    # argument checks come before any launch, so they can be exercised without a device
    assert h.elvis_rgb_to_i420_u8(16, 16, 1, 3, 4, 0, None) == -1 and b"even" in h.elvis_last_error()
    assert h.elvis_rgb_to_i420_u8(16, 16, 1, 4, 6 + 1, 0, None) == -1
    assert h.elvis_rgb_to_i420_u8(16, 16, -1, 4, 4, 0, None) == -1
    assert h.elvis_rgb_to_i420_u8(None, 16, 1, 4, 4, 0, None) == -1 and b"null" in h.elvis_last_error()
    assert h.elvis_rgb_to_i420_u8(16, None, 1, 4, 4, 1, None) == -1
    assert h.elvis_rgb_to_i420_u8(None, None, 0, 4, 4, 0, None) == 0
    for name in ("rgb_to_i420_device", "convert_frames_to_yuv420p", "write_y4m", "calculate_importance_scores", "kvazaar_delta_qp",
                 "create_kvazaar_roi_file", "svtav1_delta_qp", "create_svtav1_roi_file"):
        assert getattr(elvis_amd, name) is getattr(handoff, name)
