"""The JPEG writer without a GPU: the statement of tests/_jpeg_write_ref.py against PIL on libjpeg-turbo (tables, SOF0 /
SOS contents and the entropy-coded segment byte for byte), what its corpus contains, its mutants, the round trip through
the reader's statement, the host half of elvis_amd/jpeg_write.py, the argument checks before the library is touched, the
`jpeg_writer=` option of the directory drivers, and csrc/jpeg_encode.h walked on the host under the address and
undefined-behaviour sanitizers (tools/jpeg_encode_check.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _hooks
import _jpeg_ref as R
import _jpeg_write_ref as W
import elvis_amd
from elvis_amd import _build, _lib, drivers, frameio, jpeg_write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
turbo = pytest.mark.skipif(not R.have_turbo(), reason="PIL is not built on libjpeg-turbo")


# ----------------------------------------------------------------------------- the statement against PIL
def test_the_corpus_has_the_sizes_samplings_qualities_and_contents():
    cases = W.cases()
    assert len({c.name for c in cases}) == len(cases)
    sizes = {(c.w, c.h) for c in cases}
    assert {(w, h) for w in R.WIDTHS for h in R.HEIGHTS} | {(8, 24), (24, 8), (7, 72), (40, 8)} <= sizes
    for w, h in sizes - {(33, 17), (16, 16)}:
        assert {c.sampling for c in cases if (c.w, c.h) == (w, h)} == set(R.SAMPLINGS), (w, h)
    assert {c.quality for c in cases} == {30, 75, 95, 100}
    assert {c.kind for c in cases} == {"flat", "noise", "ramp", "checker", "white", "checker255"}
    for kind in W.EXTREMES:
        assert {c.sampling for c in cases if c.kind == kind and c.quality == 100} == set(R.SAMPLINGS)


@turbo
@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_statement_equals_pil_tables_frame_scan_and_segment(sampling):
    for c in (c for c in W.cases() if c.sampling == sampling):
        mine = R.walk(W.encoded(c.name).data)
        pil = R.walk(W.pil_encode(c.frame(), c.quality, c.subsampling))
        assert sorted(mine.qt) == sorted(pil.qt) and all(np.array_equal(mine.qt[t], pil.qt[t]) for t in pil.qt), c.name
        assert (mine.width, mine.height, mine.comps, mine.scan, mine.ri) == (pil.width, pil.height, pil.comps, pil.scan, 0), c.name
        assert mine.dc == pil.dc and mine.ac == pil.ac, c.name
        assert len(mine.segments) == len(pil.segments) == 1 and mine.segments[0] == pil.segments[0], c.name


def test_the_corpus_contains_what_could_pass_vacuously():
    enc = {c.name: W.encoded(c.name) for c in W.cases()}
    assert any(b"\xff\x00" in e.scan for e in enc.values())
    assert any(e.zrl for e in enc.values())
    assert any(e.last63 for e in enc.values())
    assert any((e.blocks[e.dummy][:, 0] != 0).any() for e in enc.values())
    # bottom padding in 4:2:0 at an odd and at an even height: the chroma plane is lengthened, and at the odd height the
    # last row is repeated once before the downsample as well
    padded = [c for c in W.cases() if c.sampling == "420" and c.h % 16 and -(-c.h // 2) % 8]
    assert any(c.h % 2 for c in padded) and any(c.h % 2 == 0 for c in padded)
    # the largest magnitude categories: DC 11 needs a difference of 1024 or more, AC 10 a coefficient of 512 or more
    top = np.concatenate([enc[c.name].blocks for c in W.cases() if c.kind in W.EXTREMES])
    assert np.abs(top[:, 1:]).max() >= 512 and np.abs(np.diff(top[:, 0])).max() >= 1024


MUTANT_CASES = {
    "h2v2_bias_swapped": "w53-h37-420-q95-noise",
    "bottom_rows_before_downsample": "w8-h24-420-q95-noise",
    "dummy_dc_zero": "w24-h8-420-q75-ramp",
    "quantise_round_down": "w53-h37-444-q75-noise",
    "dc_prediction_shared": "w53-h37-422-q75-ramp",
    "stuffing_off": "w53-h37-444-q100-noise",
    "final_fill_zero": "w53-h37-gray-q75-noise",
}


def test_every_mutant_is_tried():
    assert set(MUTANT_CASES) == set(W.MUTANTS) and len(W.MUTANTS) >= 7


@pytest.mark.parametrize("mutant", W.MUTANTS)
def test_mutants_change_the_bytes_of_their_case(mutant):
    c = W.case(MUTANT_CASES[mutant])
    want = W.encoded(c.name)
    got = W.encode(c.frame(), c.quality, c.subsampling, mutant=mutant)
    if mutant == "final_fill_zero":
        assert len(want.unstuffed) and want.scan != got.scan and want.scan[:-1] == got.scan[:-1]
    else:
        assert got.scan != want.scan


@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_statement_files_decode_to_the_pixels_pil_gives(sampling):
    for c in (c for c in W.cases() if c.sampling == sampling):
        data = W.encoded(c.name).data
        got = R.decode(data, "rgb", c.channels)
        assert got.status == R.OK and got.pixels.shape == (c.h, c.w, c.channels), c.name
        if R.have_turbo():
            assert np.array_equal(got.pixels, R.decode_with_pil(data, "rgb", c.channels)), c.name
            assert np.array_equal(got.pixels, R.decode_with_pil(W.pil_encode(c.frame(), c.quality, c.subsampling), "rgb", c.channels)), c.name


def test_channel_order_is_a_relabelling():
    c = W.case("w53-h37-420-q95-noise")
    assert W.encoded(c.name, "bgr").data == W.encoded(c.name).data
    assert W.encode(c.frame(), c.quality, c.subsampling, "bgr").scan != W.encoded(c.name).scan


# ----------------------------------------------------------------------------- the host half of the package
def test_quant_tables_header_and_code_tables_equal_the_statement():
    for q in (1, 10, 30, 49, 50, 75, 95, 100):
        for mine, want in zip(jpeg_write.jpeg_quant_tables(q), W.quant_tables(q)):
            assert mine.dtype == np.uint16 and np.array_equal(mine, want), q
    for c in (W.case("w53-h37-420-q95-noise"), W.case("w53-h37-422-q30-ramp"), W.case("w53-h37-444-q75-flat"), W.case("w53-h37-gray-q100-checker")):
        e = W.encoded(c.name)
        head = jpeg_write.jpeg_file_header(c.w, c.h, c.channels, c.quality, c.subsampling)
        assert head + e.scan + b"\xff\xd9" == e.data, c.name
    _, dc, ac = R.std_tables()
    tab = jpeg_write.encode_tables()
    assert tab.shape == (2, jpeg_write.HUFF_WORDS) and tab.dtype == np.uint32
    for t in range(2):
        assert (list(jpeg_write.STD_DC[t][0]), list(jpeg_write.STD_DC[t][1])) == (list(dc[t][0]), list(dc[t][1]))
        assert (list(jpeg_write.STD_AC[t][0]), list(jpeg_write.STD_AC[t][1])) == (list(ac[t][0]), list(ac[t][1]))
        want = np.zeros(jpeg_write.HUFF_WORDS, np.uint32)
        for bits, sym in R.code_strings(*dc[t]).items():
            want[sym] = int(bits, 2) << 5 | len(bits)
        for bits, sym in R.code_strings(*ac[t]).items():
            want[16 + sym] = int(bits, 2) << 5 | len(bits)
        assert np.array_equal(tab[t], want)
    with pytest.raises(ValueError, match="quality"):
        jpeg_write.jpeg_quant_tables(0)
    with pytest.raises(ValueError, match="channels"):
        jpeg_write.jpeg_file_header(8, 8, 2)
    with pytest.raises(ValueError, match="65535"):
        jpeg_write.jpeg_file_header(65536, 8)


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
        with pytest.raises(ValueError, match="order"):
            fn(order="gbr")
        for q in (0, 101, 95.0, True, None):
            with pytest.raises(ValueError, match="quality"):
                fn(quality=q)
        for s in ("411", 420, None, "4:2:0"):
            with pytest.raises(ValueError, match="subsampling"):
                fn(subsampling=s)
    for fn in calls[:2] + calls[3:]:
        with pytest.raises(ValueError, match="resident on the device"):
            fn()
    for bad, match in ((clip.float(), "uint8"), (clip[0, 0], "n,H,W"), (torch.zeros((1, 8, 8, 2), dtype=torch.uint8), "channels"),
                       (torch.zeros((1, 0, 8, 3), dtype=torch.uint8), "empty")):
        with pytest.raises(ValueError, match=match):
            jpeg_write.encode_jpeg_device(bad)
    with pytest.raises(ValueError, match="path"):
        jpeg_write.save_jpeg_frames_device(clip, paths[:1])
    with pytest.raises(ValueError, match="frame"):
        jpeg_write.save_jpeg_frames(clip.numpy(), paths[:1], "cuda:0")
    with pytest.raises(ValueError, match="chunk_frames"):
        jpeg_write.save_jpeg_frames(clip.numpy(), paths, "cuda:0", chunk_frames=0)
    with pytest.raises(ValueError, match="uint8"):
        jpeg_write.save_jpeg_frames([np.zeros((8, 8, 3), np.float32)], paths[:1], "cuda:0")
    with pytest.raises(RuntimeError, match="MI355X"):
        jpeg_write.save_jpeg_frames(clip.numpy(), paths, "cpu")
    assert not os.listdir(tmp_path)


def test_entry_points_validate_before_any_launch(built_lib):
    h = _lib.lib()
    for c in (W.case("w53-h37-420-q95-noise"), W.case("w53-h37-422-q30-ramp"), W.case("w53-h37-444-q75-flat"), W.case("w53-h37-gray-q100-checker"),
              W.case("w7-h72-420-q95-noise"), W.case("w1-h1-422-q95-flat")):
        assert h.elvis_jpeg_frame_blocks(c.h, c.w, c.channels, W.SUBSAMPLINGS.index(c.subsampling)) == len(W.encoded(c.name).blocks), c.name
    assert h.elvis_jpeg_frame_blocks(8, 8, 2, 0) == 0 and h.elvis_jpeg_frame_blocks(0, 8, 3, 0) == 0 and h.elvis_jpeg_frame_blocks(8, 8, 3, 3) == 0
    assert h.elvis_jpeg_frame_blocks(65535, 65535, 3, 2) == 0
    ok = dict(n=1, h=16, w=16, channels=3, order=1, quality=95, sampling=2)

    def fdct(frames=16, coef=16, **kw):
        a = dict(ok, **kw)
        return h.elvis_jpeg_fdct(frames, coef, a["n"], a["h"], a["w"], a["channels"], a["order"], a["quality"], a["sampling"], None)

    for kw, word in ((dict(frames=None), b"null"), (dict(coef=None), b"null"), (dict(coef=8), b"aligned"), (dict(n=-1), b"shape"),
                     (dict(n=65536), b"shape"), (dict(h=0), b"shape"), (dict(w=65536), b"shape"), (dict(channels=2), b"channels"),
                     (dict(order=2), b"order"), (dict(quality=0), b"quality"), (dict(quality=101), b"quality"), (dict(sampling=3), b"sampling"),
                     (dict(sampling=-1), b"sampling"), (dict(h=65535, w=65535), b"blocks")):
        assert fdct(**kw) == -1 and word in h.elvis_last_error(), kw
    assert fdct(n=0, frames=None, coef=None) == 0
    assert h.elvis_jpeg_bits(None, 16, 16, 1, 16, 16, 3, 2, None) == -1 and b"null" in h.elvis_last_error()
    assert h.elvis_jpeg_bits(16, 16, 16, 1, 16, 16, 4, 2, None) == -1 and b"channels" in h.elvis_last_error()
    assert h.elvis_jpeg_pack(16, 16, 16, 16, 16, 4, 16, 0, 16, 1, 16, 16, 3, 2, None) == -1 and b"chunks" in h.elvis_last_error()
    assert h.elvis_jpeg_pack(16, 16, 16, 16, 16, -1, 16, 1, 16, 1, 16, 16, 3, 2, None) == -1 and b"total_words" in h.elvis_last_error()
    assert h.elvis_jpeg_pack(16, 16, 16, 16, None, 4, 16, 1, 16, 1, 16, 16, 3, 2, None) == -1 and b"null" in h.elvis_last_error()
    assert h.elvis_jpeg_pack(16, 16, 16, 12, 16, 4, 16, 1, 16, 1, 16, 16, 3, 2, None) == -1 and b"aligned" in h.elvis_last_error()
    assert h.elvis_jpeg_stuff(16, 16, 16, 4, 16, 1, 16, None, 8, 1, 16, 16, 3, 2, None) == -1 and b"null" in h.elvis_last_error()
    assert h.elvis_jpeg_stuff(16, 16, 16, 4, 16, 1, 16, 16, -8, 1, 16, 16, 3, 2, None) == -1 and b"out_bytes" in h.elvis_last_error()
    assert h.elvis_jpeg_stuff(16, 16, 16, 4, 16, 1, 16, 16, 8, 1, 16, 16, 3, 7, None) == -1 and b"sampling" in h.elvis_last_error()
    if not torch.cuda.is_available():
        # without a GPU a launch fails with the library's usual code, -2, and nothing is dereferenced on the host
        frames = np.zeros((16, 16, 3), np.uint8)
        coef = np.zeros(6 * 64 + 8, np.int16)
        at = (coef.ctypes.data + 15) // 16 * 16
        assert h.elvis_jpeg_fdct(frames.ctypes.data, at, 1, 16, 16, 3, 1, 95, 2, None) == -2


def test_source_list_exports_and_the_named_chunks():
    assert "jpeg_write.hip" in _build.SOURCES
    for name in ("encode_jpeg_device", "save_jpeg_frames_device", "save_jpeg_frames", "jpeg_quant_tables", "jpeg_file_header",
                 "jpeg_roundtrip_device"):
        assert getattr(elvis_amd, name) is getattr(jpeg_write, name)
    header = open(os.path.join(ROOT, "include", "elvis_amd.h")).read()
    assert f"#define ELVIS_JPEG_SCAN_CHUNK {jpeg_write.SCAN_CHUNK_BLOCKS}\n" in header
    assert f"#define ELVIS_JPEG_STUFF_CHUNK {jpeg_write.STUFF_CHUNK_BYTES}\n" in header
    assert os.path.isfile(os.path.join(ROOT, "elvis_amd", "csrc", "jpeg_encode.h"))
    assert drivers.PNG_WRITERS == ("pil", "device", "device-rle") and drivers.JPEG_WRITERS == ("pil", "device")
    assert (drivers.JPEG_QUALITY, drivers.JPEG_SUBSAMPLING) == (95, "420")


# ----------------------------------------------------------------------------- the drivers
def _write_jpg_clip(d, n, h=16, w=24, seed=0):
    rng = np.random.default_rng(seed)
    for i in range(n):
        frameio.save_frame(rng.integers(0, 250, size=(h, w, 3), dtype=np.uint8), os.path.join(d, f"{i + 1:05d}.jpg"))


def test_jpeg_writer_option_of_the_drivers(tmp_path, monkeypatch):
    src = tmp_path / "src"
    _write_jpg_clip(str(src), 3)
    maps = np.ones((3, 2, 3), np.int32)
    calls = (
        lambda j: drivers.restore_downsampled_with_sinsr(str(src), str(tmp_path / "out"), maps, 8, devices=["cpu"], jpeg_writer=j,
                                                         _shard_fn=_hooks.plus_device_tag),
        lambda j: drivers.restore_downsampled_with_realesrgan(str(src), str(tmp_path / "out"), maps, 8, devices=["cpu"], jpeg_writer=j,
                                                              _shard_fn=_hooks.plus_device_tag),
        lambda j: drivers.restore_blur_adaptive(str(src), maps, 8, devices=["cpu"], jpeg_writer=j, _shard_fn=_hooks.plus_device_tag),
        lambda j: drivers.restore_dct_adaptive(str(src), maps, 8, devices=["cpu"], jpeg_writer=j, _shard_fn=_hooks.plus_device_tag),
    )
    for call in calls:
        with pytest.raises(ValueError, match="jpeg_writer"):
            call("gpu")
        with pytest.raises(RuntimeError, match="jpeg_writer='device' needs a GPU"):
            call("device")
    v1 = tmp_path / "v1"
    v1.mkdir()
    for i in range(3):
        frameio.save_frame(np.zeros((16, 24, 3), np.uint8), v1 / f"{i + 1:05d}.png")
    frameio.save_block_masks(np.zeros((3, 2, 3), np.uint8), tmp_path / "masks.npz")
    for fn in (lambda j: drivers.stretch_shrunk_frames(str(v1), str(tmp_path / "masks.npz"), 8, out_dir=str(tmp_path / "s"), devices=["cpu"],
                                                       jpeg_writer=j, _shard_fn=_hooks.plus_device_tag),
               lambda j: drivers.restore_shrunk_frames(str(v1), str(tmp_path / "masks.npz"), 8, out_dir=str(tmp_path / "r"), devices=["cpu"],
                                                       jpeg_writer=j, _shard_fn=_hooks.plus_device_tag)):
        with pytest.raises(ValueError, match="jpeg_writer"):
            fn("gpu")
        with pytest.raises(RuntimeError, match="jpeg_writer='device' needs a GPU"):
            fn("device")
    # the sink of a "device" JPEG writer hands the .jpg / .jpeg names to jpeg_write.py and every other name to `writer`
    seen = []
    monkeypatch.setattr(jpeg_write, "save_jpeg_frames", lambda frames, paths, device, **kw: seen.append(("host", len(frames), list(paths), device, kw)))
    monkeypatch.setattr(jpeg_write, "save_jpeg_frames_device", lambda clip, paths, **kw: seen.append(("device", tuple(clip.shape), list(paths), kw)))
    out = tmp_path / "mixed"
    names = ["00001.jpg", "00002.png", "00003.JPEG"]
    rng = np.random.default_rng(1)
    frames = [rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8) for _ in names]
    drivers.PngDirSink(str(out), names, "pil", "device").save(frames, 0, "cuda:0")
    kw = dict(quality=95, subsampling="420")
    assert seen == [("host", 2, [os.path.join(str(out), names[0]), os.path.join(str(out), names[2])], "cuda:0", kw)]
    assert os.listdir(out) == ["00002.png"] and np.array_equal(frameio.load_frame(out / "00002.png"), frames[1])
    seen.clear()
    clip = torch.from_numpy(np.stack(frames))
    drivers.PngDirSink(str(out), names, "pil", "device").save(clip[1:], 1, "cuda:0")
    assert seen == [("device", (1, 8, 8, 3), [os.path.join(str(out), names[2])], kw)]
    seen.clear()
    drivers._write_clip(clip[:, :, :, 0], str(tmp_path / "masks"), ["1.jpg", "2.jpg", "3.jpg"], "pil", "device")
    assert seen == [("device", (3, 8, 8), [os.path.join(str(tmp_path / "masks"), f"{i}.jpg") for i in (1, 2, 3)], kw)]
    # the default is "pil", and a .jpg directory is written as before: PIL's own bytes for the frames the restorer returns
    seen.clear()
    drivers.restore_downsampled_with_sinsr(str(src), str(tmp_path / "out"), maps, 8, devices=["cpu"], _shard_fn=_hooks.plus_device_tag)
    assert not seen and sorted(os.listdir(tmp_path / "out")) == [f"{i + 1:05d}.jpg" for i in range(3)]
    restored = _hooks.plus_device_tag([frameio.load_frame(src / f"{i + 1:05d}.jpg") for i in range(3)], maps, 8, "cpu", 0)
    for i, f in enumerate(restored):
        frameio.save_frame(f, tmp_path / "want" / f"{i + 1:05d}.jpg")
        assert (tmp_path / "want" / f"{i + 1:05d}.jpg").read_bytes() == (tmp_path / "out" / f"{i + 1:05d}.jpg").read_bytes()
    assert drivers._v1_kw("pil", "pil", stretched_dir=None) == {"stretched_dir": None}
    assert drivers._v1_kw("pil", "device", stretched_dir=None) == {"stretched_dir": None, "jpeg_writer": "device"}


# ----------------------------------------------------------------------------- the kernels' text on the host
def test_the_encoder_header_walks_the_corpus_under_the_sanitizers(tmp_path):
    """tools/jpeg_encode_check.cpp is a stand-alone program: it includes csrc/jpeg_encode.h, runs every case of the corpus
    through the very functions the kernels call, over buffers of exactly the kernels' sizes, and compares coefficients
    and scans with the statement."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe, corpus = str(tmp_path / "jpeg_encode_check"), str(tmp_path / "corpus.bin")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tools", "jpeg_encode_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    W.dump(corpus)
    run = subprocess.run([exe, corpus], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"{len(W.cases())} cases, 0 failed" in run.stdout
