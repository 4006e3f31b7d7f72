"""Restart intervals of the JPEG writer without a GPU: the statement of tests/_jpeg_restart_ref.py against PIL on
libjpeg-turbo (the DRI segment's place and content and everything from SOS to EOI byte for byte), what its corpus
contains, its mutants, the round trip through the reader's parser and the reader's statement, the host half of
elvis_amd/jpeg_write.py (`jpeg_restart_interval`, `jpeg_file_header(..., restart_interval=)`), the argument checks
before the library is touched, the new entry points' own checks, the `jpeg_restart_rows=` option of the directory drivers,
and csrc/jpeg_encode.h walked per restart interval on the host under the address and undefined-behaviour sanitizers
(tools/jpeg_restart_check.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _hooks
import _jpeg_ref as R
import _jpeg_restart_ref as S
import _jpeg_write_ref as W
import elvis_amd
from elvis_amd import _lib, drivers, frameio, jpeg, jpeg_write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
turbo = pytest.mark.skipif(not R.have_turbo(), reason="PIL is not built on libjpeg-turbo")


# ----------------------------------------------------------------------------- the statement against PIL
def test_the_corpus_has_the_sizes_samplings_settings_qualities_and_contents():
    cases = S.cases()
    assert len({c.name for c in cases}) == len(cases)
    assert S.WIDTHS == (1, 8, 9, 17, 33, 53) and S.HEIGHTS == (1, 8, 16, 17, 37)
    for w in S.WIDTHS:
        for h in S.HEIGHTS:
            assert {c.sampling for c in cases if (c.w, c.h) == (w, h)} == set(R.SAMPLINGS), (w, h)
    assert any((c.w, c.h, c.sampling) == (128, 128, "gray") for c in cases)
    assert {c.quality for c in cases} == {30, 75, 95, 100}
    assert {c.kind for c in cases} == {"flat200", "noise", "ramp", "white", "checker255", "flat128"}
    assert {c.kind for c in cases if (c.w, c.h) == (53, 37)} == set(S.CONTENTS)
    assert (S.case("w53-h37-444-q30-flat200-mcus7").frame() == 200).all()
    for s in R.SAMPLINGS:
        mine = [c for c in cases if c.sampling == s]
        assert {c.restart_rows for c in mine} == {0, 1, 2}, s
        assert {1, 2, 3, 5, 7} <= {c.restart_mcus for c in mine}, s
        assert any(c.restart_mcus >= S.encoded(c.name).mcus for c in mine), s
        assert all(bool(c.restart_rows) != bool(c.restart_mcus) for c in mine)


@turbo
@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_statement_equals_pil_dri_and_entropy_coded_bytes(sampling):
    for c in (c for c in S.cases() if c.sampling == sampling):
        e = S.encoded(c.name)
        pil = S.pil_encode(c)
        mine_w, pil_w = R.walk(e.data), R.walk(pil)
        assert sorted(mine_w.qt) == sorted(pil_w.qt) and all(np.array_equal(mine_w.qt[t], pil_w.qt[t]) for t in pil_w.qt), c.name
        assert (mine_w.width, mine_w.height, mine_w.comps, mine_w.scan) == (pil_w.width, pil_w.height, pil_w.comps, pil_w.scan), c.name
        assert mine_w.dc == pil_w.dc and mine_w.ac == pil_w.ac, c.name
        assert mine_w.ri == pil_w.ri == e.ri > 0, c.name
        mine_seen, mine_tail = S.entropy_part(e.data)
        pil_seen, pil_tail = S.entropy_part(pil)
        # DRI stands behind the last DHT, in front of SOS, in both; PIL's file may have other APPn segments in front
        assert mine_seen[-3:] == pil_seen[-3:] == [0xC4, 0xDD, 0xDA] and mine_seen.count(0xDD) == pil_seen.count(0xDD) == 1, c.name
        at = e.data.index(b"\xff\xdd")
        assert e.data[at:at + 6] == b"\xff\xdd\x00\x04" + e.ri.to_bytes(2, "big") and e.data[at:at + 6] in pil, c.name
        assert mine_tail == pil_tail == e.scan + b"\xff\xd9", c.name


def test_the_corpus_contains_what_could_pass_vacuously():
    enc = {c.name: S.encoded(c.name) for c in S.cases()}
    cases = {c.name: c for c in S.cases()}
    # at least 9 markers: the index wraps from D7 to D0
    wrapped = [e for e in enc.values() if len(e.intervals) >= 10]
    assert wrapped and all(S.markers(e.scan)[:9] == [0xD0 + k for k in range(8)] + [0xD0] for e in wrapped)
    assert all(len(S.markers(e.scan)) == len(e.intervals) - 1 == -(-e.mcus // e.ri) - 1 for e in enc.values())
    # an interval that does not divide an MCU row
    assert any(S.mcu_grid(c.w, c.h, c.channels, c.subsampling)[0] % enc[n].ri and 1 < enc[n].ri < enc[n].mcus for n, c in cases.items())
    # an interval that divides M exactly: the file ends pad, EOI, and no marker stands in front of EOI
    exact = [e for e in enc.values() if e.ri < e.mcus and e.mcus % e.ri == 0]
    assert exact and all(e.data.endswith(e.intervals[-1][0] + b"\xff\xd9") and e.intervals[-1][0] for e in exact)
    # Ri >= M: DRI and no marker
    whole = [e for e in enc.values() if e.ri >= e.mcus]
    assert whole and all(b"\xff\xdd\x00\x04" in e.data and not S.markers(e.scan) and len(e.intervals) == 1 for e in whole)
    # a pad byte FF stuffed in front of a marker
    assert any(raw.endswith(b"\xff") and stuffed.endswith(b"\xff\x00") and stuffed + bytes([0xFF, 0xD0 + (s & 7)]) in e.scan
               for e in enc.values() for s, (stuffed, raw) in enumerate(e.intervals[:-1]))
    # an interval of fewer than 4 stream bytes, followed by another one
    assert any(0 < len(raw) < 4 for e in enc.values() for _, raw in e.intervals[:-1])
    assert any(len(raw) == 1 for e in enc.values() for _, raw in e.intervals[:-1])
    # 4:2:0 with odd block counts: an interval whose first block follows an MCU that ends a row with dummy blocks
    found = False
    for n, c in cases.items():
        e = enc[n]
        if c.sampling != "420" or -(-c.w // 8) % 2 == 0 or e.ri >= e.mcus:
            continue
        for s in range(1, len(e.intervals)):
            first = s * e.ri * e.bpm
            found |= bool(e.dummy[first - e.bpm:first].any()) and e.blocks[first - e.bpm:first][e.dummy[first - e.bpm:first]][:, 0].any()
    assert found
    # a non-zero DC at the start of an interval >= 1 that equals the DC before it: only the predictor's reset shows
    found = False
    for e in enc.values():
        for s in range(1, len(e.intervals)):
            first = s * e.ri * e.bpm
            found |= e.blocks[first, 0] != 0 and e.blocks[first, 0] == e.blocks[first - e.bpm + (e.bpm - 3 if e.bpm > 1 else 0), 0]
    assert found


MUTANT_CASES = {
    "predictor_not_reset": "w53-h37-444-q30-flat200-mcus7",
    "marker_index_not_wrapped": "w53-h37-gray-q75-noise-mcus3",
    "marker_after_last": "w53-h37-gray-q75-noise-mcus3",
    "pad_zero": "w53-h37-gray-q75-noise-mcus3",
    "pad_ff_not_stuffed": "w53-h37-gray-q75-noise-mcus3",
    "marker_stuffed": "w53-h37-gray-q75-noise-mcus3",
}


def test_every_mutant_is_tried():
    assert set(MUTANT_CASES) | {"rows_not_capped"} == set(S.MUTANTS) and len(S.MUTANTS) >= 7


@pytest.mark.parametrize("mutant", sorted(MUTANT_CASES))
def test_mutants_change_the_bytes_of_their_case(mutant):
    c = S.case(MUTANT_CASES[mutant])
    want = S.encoded(c.name)
    got = S.encode(c.frame(), c.quality, c.subsampling, mutant=mutant, **c.restart)
    assert got.scan != want.scan and got.ri == want.ri
    if mutant == "marker_after_last":
        assert got.scan[:-2] == want.scan and 0xD0 <= got.scan[-1] <= 0xD7
    if mutant == "pad_ff_not_stuffed":
        assert len(got.scan) < len(want.scan)
    if mutant == "marker_index_not_wrapped":
        assert len(got.scan) == len(want.scan) and len(want.intervals) >= 10


def test_restart_rows_are_capped_at_65535_mcus():
    # 65535 pixels wide in 4:4:4: 8192 MCUs a row, so 8 rows would be 65536
    for fn in (lambda **kw: jpeg_write.jpeg_restart_interval(65535, 64, 3, "444", **kw), lambda **kw: S.restart_interval(65535, 64, 3, "444", **kw)):
        assert fn(restart_rows=7) == 7 * 8192
        assert fn(restart_rows=8) == 65535
        assert fn(restart_rows=1000) == 65535
    assert S.restart_interval(65535, 64, 3, "444", restart_rows=8, mutant="rows_not_capped") == 65536
    assert jpeg_write.jpeg_restart_interval(65535, 64, 1, "420", restart_rows=8) == 65535
    assert jpeg_write.jpeg_restart_interval(65535, 64, 3, "420", restart_rows=8) == 8 * 4096


# ----------------------------------------------------------------------------- the round trip on the host
@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_statement_files_parse_and_decode_to_the_pixels_without_an_interval(sampling):
    for c in (c for c in S.cases() if c.sampling == sampling):
        e = S.encoded(c.name)
        info = jpeg.parse_jpeg(e.data, c.name)
        assert info.restart_interval == e.ri and len(info.segments) == -(-e.mcus // e.ri) == len(e.intervals), c.name
        assert [s[2:] for s in info.segments] == [(k * e.ri, min(e.ri, e.mcus - k * e.ri)) for k in range(len(e.intervals))], c.name
        got = R.decode(e.data, "rgb", c.channels)
        assert got.status == R.OK and got.pixels.shape == (c.h, c.w, c.channels), c.name
        assert np.array_equal(got.pixels, R.decode(S.plain(c.name), "rgb", c.channels).pixels), c.name
        if R.have_turbo():
            assert np.array_equal(got.pixels, R.decode_with_pil(e.data, "rgb", c.channels)), c.name
            assert np.array_equal(got.pixels, R.decode_with_pil(S.pil_encode(c), "rgb", c.channels)), c.name


# ----------------------------------------------------------------------------- the host half of the package
def test_interval_and_header_equal_the_statement_and_the_default_is_todays_header():
    assert elvis_amd.jpeg_restart_interval is jpeg_write.jpeg_restart_interval
    for c in S.cases():
        e = S.encoded(c.name)
        assert jpeg_write.jpeg_restart_interval(c.w, c.h, c.channels, c.subsampling, **c.restart) == e.ri, c.name
        if c.w == 53 or c.h == 17:
            head = jpeg_write.jpeg_file_header(c.w, c.h, c.channels, c.quality, c.subsampling, restart_interval=e.ri)
            assert head + e.scan + b"\xff\xd9" == e.data, c.name
    assert jpeg_write.jpeg_restart_interval(53, 37) == 0 and jpeg_write.jpeg_restart_interval(53, 37, 3, "420", 0, 0) == 0
    for c in (W.case("w53-h37-420-q95-noise"), W.case("w53-h37-gray-q100-checker"), W.case("w53-h37-422-q30-ramp")):
        e = W.encoded(c.name)
        today = e.data[:len(e.data) - len(e.scan) - 2]
        assert jpeg_write.jpeg_file_header(c.w, c.h, c.channels, c.quality, c.subsampling, restart_interval=0) == today
        assert jpeg_write.jpeg_file_header(c.w, c.h, c.channels, c.quality, c.subsampling) == today
    for bad in (-1, 65536, True, 1.0, None):
        with pytest.raises(ValueError, match="restart_interval"):
            jpeg_write.jpeg_file_header(8, 8, restart_interval=bad)
    with pytest.raises(ValueError, match="give one"):
        jpeg_write.jpeg_restart_interval(8, 8, restart_rows=1, restart_mcus=1)
    with pytest.raises(ValueError, match="channels"):
        jpeg_write.jpeg_restart_interval(8, 8, 2, restart_rows=1)
    with pytest.raises(ValueError, match="subsampling"):
        jpeg_write.jpeg_restart_interval(8, 8, 3, "411", restart_rows=1)
    with pytest.raises(ValueError, match="65535"):
        jpeg_write.jpeg_restart_interval(0, 8, restart_rows=1)


def test_argument_checks_before_the_library_is_touched(monkeypatch, tmp_path):
    def touched(*a, **kw):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(jpeg_write, "lib", touched)
    clip = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    paths = [tmp_path / "a.jpg", tmp_path / "b.jpg"]
    calls = (lambda **kw: jpeg_write.encode_jpeg_device(clip, **kw),
             lambda **kw: jpeg_write.save_jpeg_frames_device(clip, paths, **kw),
             lambda **kw: jpeg_write.save_jpeg_frames(clip.numpy(), paths, "cuda:0", **kw),
             lambda **kw: jpeg_write.jpeg_roundtrip_device(clip, **kw))
    for fn in calls:
        for name in ("restart_rows", "restart_mcus"):
            for bad in (-1, True, False, 1.0, "1", None):
                with pytest.raises(ValueError, match=name):
                    fn(**{name: bad})
        with pytest.raises(ValueError, match="give one"):
            fn(restart_rows=1, restart_mcus=2)
        with pytest.raises(ValueError, match="restart_mcus"):
            fn(restart_mcus=65536)
    # the keywords are keyword-only on the forms that take the others by position
    with pytest.raises(TypeError):
        jpeg_write.encode_jpeg_device(clip, "bgr", 95, "420", 1)
    with pytest.raises(TypeError):
        jpeg_write.save_jpeg_frames_device(clip, paths, "bgr", 95, "420", 1)
    with pytest.raises(TypeError):
        jpeg_write.jpeg_roundtrip_device(clip, 95, "420", "bgr", 1)
    # a good interval goes on to the next check: the clip is not resident
    for fn in calls[:2] + calls[3:]:
        with pytest.raises(ValueError, match="resident on the device"):
            fn(restart_rows=1)
        with pytest.raises(ValueError, match="resident on the device"):
            fn(restart_mcus=65535)
    # more (frame, interval) pairs than a launch takes: refused before any launch, never a truncated grid
    assert 60000 * 256 <= jpeg_write.MAX_SEGMENTS < 60000 * 512
    with pytest.raises(ValueError, match="segments"):
        jpeg_write._check_segments(60000, 128, 256, 1, "420", 1, "encode_jpeg_device")
    assert jpeg_write._check_segments(60000, 128, 128, 1, "420", 1, "encode_jpeg_device") == (256, 256)
    assert jpeg_write._check_segments(3, 37, 53, 3, "420", 5, "x") == (3, 12) and jpeg_write._check_segments(3, 37, 53, 3, "420", 12, "x") == (1, 12)
    assert not os.listdir(tmp_path)


def test_new_entry_points_validate_before_any_launch(built_lib):
    h = _lib.lib()
    for c in S.cases():
        e = S.encoded(c.name)
        assert h.elvis_jpeg_segments(c.h, c.w, c.channels, W.SUBSAMPLINGS.index(c.subsampling), e.ri) == len(e.intervals), c.name
    assert h.elvis_jpeg_segments(37, 53, 3, 2, 0) == 1
    assert h.elvis_jpeg_segments(37, 53, 3, 2, -1) == 0 and b"restart_mcus" in h.elvis_last_error()
    assert h.elvis_jpeg_segments(37, 53, 3, 2, 65536) == 0 and h.elvis_jpeg_segments(37, 53, 2, 2, 1) == 0 and h.elvis_jpeg_segments(0, 53, 3, 2, 1) == 0
    assert h.elvis_jpeg_bits_rst(None, 16, 16, 1, 16, 16, 3, 2, 1, None) == -1 and b"null" in h.elvis_last_error()
    assert h.elvis_jpeg_bits_rst(16, 16, 16, 1, 16, 16, 3, 2, -1, None) == -1 and b"restart_mcus" in h.elvis_last_error()
    assert h.elvis_jpeg_bits_rst(16, 16, 16, 1, 16, 16, 3, 2, 65536, None) == -1 and b"restart_mcus" in h.elvis_last_error()
    assert h.elvis_jpeg_bits_rst(16, 16, 16, 1, 16, 16, 4, 2, 1, None) == -1 and b"channels" in h.elvis_last_error()
    assert h.elvis_jpeg_bits_rst(16, 16, 18, 1, 16, 16, 3, 2, 1, None) == -1 and b"aligned" in h.elvis_last_error()
    # 65535 frames of 128x256 gray with an interval of one MCU: 512 segments each, above 2^24 in all
    assert h.elvis_jpeg_bits_rst(16, 16, 16, 65535, 128, 256, 1, 2, 1, None) == -1 and b"segments" in h.elvis_last_error()
    assert h.elvis_jpeg_bits_rst(None, None, None, 0, 16, 16, 3, 2, 1, None) == 0
    assert h.elvis_jpeg_pack_rst(16, 16, 16, 16, 16, 4, 16, 0, 16, 1, 16, 16, 3, 2, 1, None) == -1 and b"chunks" in h.elvis_last_error()
    assert h.elvis_jpeg_pack_rst(16, 16, 16, 16, 16, -1, 16, 1, 16, 1, 16, 16, 3, 2, 1, None) == -1 and b"total_words" in h.elvis_last_error()
    assert h.elvis_jpeg_pack_rst(16, 16, 16, 16, None, 4, 16, 1, 16, 1, 16, 16, 3, 2, 1, None) == -1 and b"null" in h.elvis_last_error()
    assert h.elvis_jpeg_pack_rst(16, 16, 16, 12, 16, 4, 16, 1, 16, 1, 16, 16, 3, 2, 1, None) == -1 and b"aligned" in h.elvis_last_error()
    assert h.elvis_jpeg_pack_rst(16, 16, 16, 16, 16, 4, 16, 1, 16, 1, 16, 16, 3, 2, 70000, None) == -1 and b"restart_mcus" in h.elvis_last_error()
    assert h.elvis_jpeg_stuff_rst(16, 16, 16, 4, 16, 1, 16, None, 8, 1, 16, 16, 3, 2, 1, None) == -1 and b"null" in h.elvis_last_error()
    assert h.elvis_jpeg_stuff_rst(16, 16, 16, 4, 16, 1, 16, 16, -8, 1, 16, 16, 3, 2, 1, None) == -1 and b"out_bytes" in h.elvis_last_error()
    assert h.elvis_jpeg_stuff_rst(16, 16, 16, 4, 16, 1, 16, 16, 8, 1, 16, 16, 3, 7, 1, None) == -1 and b"sampling" in h.elvis_last_error()
    assert h.elvis_jpeg_stuff_rst(16, 16, 16, 4, 16, 1, 16, 16, 8, 1, 16, 16, 3, 2, -5, None) == -1 and b"restart_mcus" in h.elvis_last_error()
    for name in ("elvis_jpeg_segments", "elvis_jpeg_bits_rst", "elvis_jpeg_pack_rst", "elvis_jpeg_stuff_rst"):
        assert name in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "elvis_amd.h")).read()
    assert f"#define ELVIS_JPEG_MAX_SEGMENTS {jpeg_write.MAX_SEGMENTS}\n" in header


# ----------------------------------------------------------------------------- the drivers
def test_jpeg_restart_rows_option_of_the_drivers(tmp_path, monkeypatch):
    src = tmp_path / "src"
    rng = np.random.default_rng(0)
    for i in range(3):
        frameio.save_frame(rng.integers(0, 250, size=(16, 24, 3), dtype=np.uint8), os.path.join(str(src), f"{i + 1:05d}.jpg"))
    maps = np.ones((3, 2, 3), np.int32)
    v1 = tmp_path / "v1"
    v1.mkdir()
    for i in range(3):
        frameio.save_frame(np.zeros((16, 24, 3), np.uint8), v1 / f"{i + 1:05d}.png")
    frameio.save_block_masks(np.zeros((3, 2, 3), np.uint8), tmp_path / "masks.npz")
    calls = (
        lambda **kw: drivers.restore_downsampled_with_sinsr(str(src), str(tmp_path / "out"), maps, 8, devices=["cpu"], _shard_fn=_hooks.plus_device_tag, **kw),
        lambda **kw: drivers.restore_downsampled_with_realesrgan(str(src), str(tmp_path / "out"), maps, 8, devices=["cpu"],
                                                                 _shard_fn=_hooks.plus_device_tag, **kw),
        lambda **kw: drivers.restore_blur_adaptive(str(src), maps, 8, devices=["cpu"], _shard_fn=_hooks.plus_device_tag, **kw),
        lambda **kw: drivers.restore_dct_adaptive(str(src), maps, 8, devices=["cpu"], _shard_fn=_hooks.plus_device_tag, **kw),
        lambda **kw: drivers.stretch_shrunk_frames(str(v1), str(tmp_path / "masks.npz"), 8, out_dir=str(tmp_path / "s"), devices=["cpu"],
                                                   _shard_fn=_hooks.plus_device_tag, **kw),
        lambda **kw: drivers.restore_shrunk_frames(str(v1), str(tmp_path / "masks.npz"), 8, out_dir=str(tmp_path / "r"), devices=["cpu"],
                                                   _shard_fn=_hooks.plus_device_tag, **kw),
    )
    for call in calls:
        for kw in (dict(jpeg_restart_rows=1), dict(jpeg_restart_rows=2, jpeg_writer="pil")):
            with pytest.raises(ValueError, match=r"jpeg_restart_rows.*jpeg_writer"):
                call(**kw)
        for bad in (-1, True, 1.5, "1"):
            with pytest.raises(ValueError, match="jpeg_restart_rows"):
                call(jpeg_restart_rows=bad, jpeg_writer="device")
        with pytest.raises(RuntimeError, match="jpeg_writer='device' needs a GPU"):
            call(jpeg_restart_rows=1, jpeg_writer="device")
    assert drivers.JPEG_WRITERS == ("pil", "device")
    # the sink hands restart_rows= on only where it is not 0
    seen = []
    monkeypatch.setattr(jpeg_write, "save_jpeg_frames", lambda frames, paths, device, **kw: seen.append(("host", len(frames), list(paths), device, kw)))
    monkeypatch.setattr(jpeg_write, "save_jpeg_frames_device", lambda clip, paths, **kw: seen.append(("device", tuple(clip.shape), list(paths), kw)))
    out = tmp_path / "mixed"
    names = ["00001.jpg", "00002.png", "00003.JPEG"]
    frames = [rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8) for _ in names]
    plain, rst = dict(quality=95, subsampling="420"), dict(quality=95, subsampling="420", restart_rows=2)
    jpgs = [os.path.join(str(out), names[0]), os.path.join(str(out), names[2])]
    drivers.PngDirSink(str(out), names, "pil", "device", 2).save(frames, 0, "cuda:0")
    drivers.PngDirSink(str(out), names, "pil", "device", 0).save(frames, 0, "cuda:0")
    drivers.PngDirSink(str(out), names, "pil", "device").save(frames, 0, "cuda:0")
    assert seen == [("host", 2, jpgs, "cuda:0", rst), ("host", 2, jpgs, "cuda:0", plain), ("host", 2, jpgs, "cuda:0", plain)]
    seen.clear()
    clip = torch.from_numpy(np.stack(frames))
    drivers.PngDirSink(str(out), names, "pil", "device", jpeg_restart_rows=2).save(clip[1:], 1, "cuda:0")
    assert seen == [("device", (1, 8, 8, 3), [os.path.join(str(out), names[2])], rst)]
    seen.clear()
    masks = [os.path.join(str(tmp_path / "masks"), f"{i}.jpg") for i in (1, 2, 3)]
    drivers._write_clip(clip[:, :, :, 0], str(tmp_path / "masks"), ["1.jpg", "2.jpg", "3.jpg"], "pil", "device", 2)
    drivers._write_clip(clip[:, :, :, 0], str(tmp_path / "masks"), ["1.jpg", "2.jpg", "3.jpg"], "pil", "device", 0)
    assert seen == [("device", (3, 8, 8), masks, rst), ("device", (3, 8, 8), masks, plain)]
    assert drivers._v1_kw("pil", "device", 0, stretched_dir=None) == {"stretched_dir": None, "jpeg_writer": "device"}
    assert drivers._v1_kw("pil", "device", 1, stretched_dir=None) == {"stretched_dir": None, "jpeg_writer": "device", "jpeg_restart_rows": 1}
    assert drivers._v1_kw("device", "device", jpeg_restart_rows=3) == {"png_writer": "device", "jpeg_writer": "device", "jpeg_restart_rows": 3}


# ----------------------------------------------------------------------------- the kernels' text on the host
def test_the_encoder_header_walks_the_restart_corpus_under_the_sanitizers(tmp_path):
    """tools/jpeg_restart_check.cpp is a stand-alone program: it includes csrc/jpeg_encode.h, runs every case of the restart
    corpus through the very functions the kernels call, per (segment, block) with the segments out of order, over
    buffers of exactly the kernels' sizes, and compares coefficients and the bytes from SOS to EOI with the statement."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe, corpus = str(tmp_path / "jpeg_restart_check"), str(tmp_path / "corpus.bin")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tools", "jpeg_restart_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    S.dump(corpus)
    run = subprocess.run([exe, corpus], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"{len(S.cases())} cases, 0 failed" in run.stdout
