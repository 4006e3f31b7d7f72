"""The clip intake on the CPU: the numpy statement (tests/_resize_ref.py) against the statements the project already has,
the mutants against the GPU cases, the tile plan, the ABI and build entries, and the intake's host logic with the device
calls stubbed."""
import os
import re

import numpy as np
import pytest
import torch

import _presley_degrade_ref as P
import _resize_ref as R
from elvis_amd import _build, _lib, degrade, intake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the statement
@pytest.mark.parametrize("b,d", [(12, d) for d in (12, 6, 4, 3, 5, 7, 1)] + [(31, 9)])
def test_on_squares_the_statement_is_the_block_degraders(b, d):
    x = np.random.default_rng(b * 100 + d).integers(0, 256, (3, b, b, 3), dtype=np.uint8)
    assert np.array_equal(R.resize_area_u8(x, d, d), P.resize_area_u8(x, d))


@pytest.mark.parametrize("src,dst", [(12, 5), (31, 9), (79, 10), (1001, 1000), (1500, 1499), (12, 4)])
def test_the_three_tables_are_one(src, dst):
    assert R.entries(src, dst) == P.area_entries(src, dst) == degrade.area_table(src, dst)
    start, first, w = intake.axis_tables(src, dst)
    flat = [(d, int(first[d]) + k, w[start[d] + k]) for d in range(dst) for k in range(start[d + 1] - start[d])]
    assert flat == degrade.area_table(src, dst)


@pytest.mark.parametrize("factor", [1, 2, 3, 4])
def test_at_whole_ratios_the_statement_is_the_glue_oracle(factor):
    glue = pytest.importorskip("oracle.glue_ref")
    x = np.random.default_rng(factor).integers(0, 256, (2, 4 * factor, 6 * factor, 3), dtype=np.uint8)
    got = R.resize_area_u8(x, 4, 6)
    for f in range(2):
        assert np.array_equal(got[f], glue.area_downscale_u8(x[f], factor, "cv2"))


def _all_sizes():
    return sorted({size for c in R.CHANNELS for size in R.cases(c).values() if size not in R.STEEP.values() and size not in R.STEEP_C1.values()})


@pytest.mark.parametrize("value", [0, 1, 127, 128, 254, 255])
def test_a_constant_frame_stays_constant(value):
    for hs, ws, hd, wd in _all_sizes():
        out = R.resize_area_u8(np.full((1, hs, ws, 3), value, np.uint8), hd, wd)
        assert (out == value).all(), (hs, ws, hd, wd)


# the case of tests/test_gpu_resize.py (name, channels, frames) whose bytes each mutant changes
SEEN_BY = {"fma": ("1500x1->1499x1", 3, 3), "box2_everywhere": ("6x12->3x4", 1, 3), "half_up": ("6x12->3x4", 3, 3),
           "swap_axes_tables": ("7x10->3x4", 1, 3), "fast_when_one_axis_whole": ("12x10->4x4", 3, 3)}


@pytest.mark.parametrize("mutant", sorted(SEEN_BY))
def test_every_mutant_changes_bytes_of_a_gpu_case(mutant):
    name, c, n = SEEN_BY[mutant]
    hs, ws, hd, wd = R.cases(c)[name]
    x = R.frames(hs, ws, c, n)
    assert not np.array_equal(R.resize_area_u8(x, hd, wd, mutant), R.resize_area_u8(x, hd, wd)), f"{mutant} is not seen by {name}"


def test_the_cutoff_drops_table_entries_where_the_gpu_cases_are():
    """`no_cutoff`: 1001 -> 1000 drops one entry and 1500 -> 1499 two, both GPU cases, so a kernel reading a table without
    the cut-off reads another table there.  In bytes the mutant cannot show at these sizes: a dropped entry weighs under
    1e-3 of its cell, at most 0.255 of a byte, and the kept weights move a sum by at most 0.001 * 255 from a whole number,
    never to within 0.255 of a half - which is why the drop is asserted on the table."""
    assert set(R.MUTANTS) == set(SEEN_BY) | {"no_cutoff"}
    for src, dst, dropped in ((1001, 1000, 1), (1500, 1499, 2)):
        kept, every = P.area_entries(src, dst), R.entries(src, dst, 0.0)
        assert len(every) - len(kept) == dropped
        gone = [e for e in every if (e[0], e[1]) not in {(k[0], k[1]) for k in kept}]
        assert len(gone) == dropped and all(0 < float(e[2]) < 1.1e-3 for e in gone)
    assert (1, 1001, 1, 1000) in R.FRACTIONAL.values() and (1500, 1, 1499, 1) in R.FRACTIONAL.values()


def test_nearest_statement_is_the_hosts_rule():
    from elvis_amd.complexity import resize_masks_nearest
    m = np.random.default_rng(2).integers(0, 2, (16, 24), dtype=np.uint8)
    for dst in ((4, 6), (5, 7), (33, 50)):
        assert np.array_equal(R.resize_nearest_u8(m[None], *dst)[0], resize_masks_nearest([m], *dst)[0])


# ----------------------------------------------------------------------------- plan, ABI, build
@pytest.mark.parametrize("ratio", [1.001, 1.5, 2.5, 7.9, 40])
@pytest.mark.parametrize("c", R.CHANNELS)
def test_the_plan_stays_within_the_lds(ratio, c):
    hd, wd = 97, 211
    hs, ws = int(round(hd * ratio)), int(round(wd * ratio))
    th, tw, lds = intake.resize_area_plan(hs, ws, hd, wd, c)
    assert 1 <= th <= hd and 1 <= tw <= wd and th * tw * c <= intake.TILE_VALUES
    assert 0 < lds <= intake.LDS_LIMIT <= 160 * 1024
    _, _, rows, stride = intake._plan(hs, ws, hd, wd, c)
    xs, xf, _ = intake.axis_tables(ws, wd)
    assert stride % 4 == 0 and stride >= intake._reach(xs, xf, tw) * c + 3 and rows * stride == lds


def test_a_row_no_lds_holds_is_read_in_place():
    assert intake.resize_area_plan(2, 90001, 1, 2, 4) == (1, 1, 0)
    assert intake.resize_area_plan(2, 90001, 1, 2, 1)[2] > 0


def test_every_area_instantiation_is_reached_by_a_gpu_case_at_every_channel_count():
    """elvis_resize_area_u8 dispatches on (both ratios whole, row_stride == 0).  The GPU cases reach all four kernels at
    C = 1, where only a destination column that reads more than 64 KiB of one source row goes in place (STEEP_C1), and
    at C = 3 and C = 4, where the STEEP cases do: no instantiation is out of `_plan`'s reach at any channel count.  The
    steep cases stay at two source rows (and, in tests/test_gpu_resize.py, at n = 1)."""
    assert set(R.AREA_KERNELS.values()) == {f"resize_area_kernel<{a},{b}>" for a in ("whole", "frac") for b in ("lds", "direct")}
    src = open(os.path.join(ROOT, "elvis_amd", "csrc", "resize.hip")).read()
    assert all(f'"{k}"' in src for k in R.AREA_KERNELS.values()) and f'elvis_note_launch("{R.NEAREST_KERNEL}")' in src
    assert "const bool direct = row_stride == 0;" in src and "const bool whole = hs % hd == 0 && ws % wd == 0;" in src
    for c in R.CHANNELS:
        reached = {}
        for name, size in R.cases(c).items():
            reached.setdefault(R.area_kernel(*size, c), []).append(name)
        assert set(reached) == set(R.AREA_KERNELS.values()), (c, sorted(reached))
        steep = set(R.STEEP) | (set(R.STEEP_C1) if c == 1 else set())
        assert set(reached["resize_area_kernel<whole,direct>"] + reached["resize_area_kernel<frac,direct>"]) <= steep
    assert all(size[0] == 2 for size in list(R.STEEP.values()) + list(R.STEEP_C1.values()))
    assert not set(R.STEEP_C1) & set(R.cases(3)) and set(R.STEEP_C1) <= set(R.cases(1))
    # at C = 1 the STEEP cases themselves still fit the LDS: that is why STEEP_C1 exists
    assert {R.area_kernel(*size, 1) for size in R.STEEP.values()} == {"resize_area_kernel<whole,lds>", "resize_area_kernel<frac,lds>"}


def test_the_header_declares_both_entry_points_and_the_source_is_built():
    src = open(os.path.join(ROOT, "include", "elvis_amd.h")).read()
    for name in ("elvis_resize_area_u8", "elvis_resize_nearest_u8"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src) and name in _lib.SIGNATURES
    assert "presley.py:186" in src
    assert "resize.hip" in _build.SOURCES and os.path.isfile(os.path.join(_build.CSRC, "resize.hip"))


def test_error_conventions_on_the_host():
    with pytest.raises(ValueError, match="height"):
        intake.resize_area_plan(6, 8, 7, 8, 3)
    with pytest.raises(ValueError, match="width"):
        intake.resize_area_plan(6, 8, 6, 9, 3)
    with pytest.raises(ValueError, match="positive"):
        intake.resize_area_plan(6, 8, 0, 8, 3)
    with pytest.raises(ValueError, match="channels"):
        intake.resize_area_plan(6, 8, 3, 4, 2)
    for fn in (intake.resize_area_device, intake.resize_nearest_device):
        with pytest.raises(ValueError, match="on the device"):
            fn(torch.zeros((1, 6, 8, 3), dtype=torch.uint8), 3, 4)            # a host tensor
    with pytest.raises(ValueError, match="uint8"):
        intake.resize_area(np.zeros((6, 8, 3), np.float32), (4, 3))
    with pytest.raises(ValueError, match="frame_stride"):
        intake._pick(5, 0, None, "x")
    with pytest.raises(ValueError, match="max_frames"):
        intake._pick(5, 1, -1, "x")


# ----------------------------------------------------------------------------- intake logic, device calls stubbed
def test_stride_then_cap():
    assert list(intake._pick(10, 3, None, "x")) == [0, 3, 6, 9]
    assert list(intake._pick(10, 3, 2, "x")) == [0, 3]                       # [::3][:2], not [:2][::3]
    assert list(intake._pick(5, 1, 9, "x")) == [0, 1, 2, 3, 4]
    assert list(intake._pick(5, 2, 0, "x")) == []


def test_load_clip_device_reads_windows_of_kept_frames(monkeypatch, tmp_path):
    from elvis_amd import handoff
    calls, resized = [], []
    path = tmp_path / "clip.yuv"
    path.write_bytes(bytes(12 * 18 * 3 // 2 * 7))                              # seven 12 x 18 I420 frames

    def load(source, width, height, device, order="bgr", *, start=0, count=None, chunk_frames=None):
        calls.append((width, height, order, start, count))
        return torch.arange(start, start + count, dtype=torch.uint8).view(-1, 1, 1, 1).expand(count, height, width, 3)

    def resize(frames_d, out_h, out_w, out=None):
        resized.append((tuple(frames_d.shape), out_h, out_w, frames_d[:, 0, 0, 0].tolist(), frames_d.is_contiguous()))
        out[:] = frames_d[:, :out_h, :out_w]
        return out

    monkeypatch.setattr(handoff, "load_yuv420p_device", load)
    monkeypatch.setattr(intake, "resize_area_device", resize)
    monkeypatch.setattr(intake.L, "resolve_device", lambda device: torch.device("cpu"))
    monkeypatch.setattr(torch.cuda, "device", lambda dev: __import__("contextlib").nullcontext())
    clip, rate = intake.load_clip_device(str(path), 8, 6, "cpu", src_width=18, src_height=12, frame_stride=3, max_frames=2, chunk_frames=1)
    assert rate is None and tuple(clip.shape) == (2, 6, 8, 3) and clip[:, 0, 0, 0].tolist() == [0, 3]
    assert calls == [(18, 12, "rgb", 0, 1), (18, 12, "rgb", 3, 1)]             # only the kept frames, (width, height) order
    assert [r[1:4] for r in resized] == [(6, 8, [0]), (6, 8, [3])] and all(r[4] for r in resized)
    calls.clear()
    resized.clear()
    clip, _ = intake.load_clip_device(str(path), 8, 6, "cpu", src_width=18, src_height=12, frame_stride=3)
    assert calls == [(18, 12, "rgb", 0, 7)] and resized[0][3] == [0, 3, 6] and resized[0][4]   # frames 1, 2, 4, 5 dropped before the resize
    with pytest.raises(ValueError, match="src_width"):
        intake.load_clip_device(str(path), 8, 6, "cpu", src_height=12)
    with pytest.raises(ValueError, match="width"):
        intake.load_clip_device(str(path), 20, 6, "cpu", src_width=18, src_height=12)


def test_names_are_exported():
    import elvis_amd
    for name in ("resize_area_device", "resize_nearest_device", "resize_area", "resize_masks_nearest_device", "intake_device",
                 "load_clip_device", "resize_area_plan", "analyze_clip_file"):
        assert callable(getattr(elvis_amd, name)), name
    for doc in (intake.__doc__, intake.resize_area_device.__doc__):
        assert "PARITY UNPINNED" in doc
    assert "DEPARTURE" in intake.__doc__
