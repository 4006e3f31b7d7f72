"""The PNG reader's statement (tests/_png_read_ref.py) against its oracles, zlib and PIL, and the reader's host side
(elvis_amd/png.py: parse_png, the argument checks, `png_reader=` of the drivers) - no GPU.  The mutants show that the
corpus tells the statement from its near misses."""
import os
import zlib

import numpy as np
import pytest

import _hooks
import _png_read_ref as R
from elvis_amd import _build, drivers, frameio, png


def _zlib_accepts(stream: bytes, cap: int) -> bool:
    try:
        return len(zlib.decompress(stream)) == cap
    except zlib.error:
        return False


def test_statement_inflater_equals_zlib_on_every_stream():
    for sc in R.good_streams():
        want = zlib.decompress(sc.stream)
        got = R.inflated(sc.name)
        assert got.status == R.OK and got.out == want and len(want) == sc.cap, sc.name
        assert got.adler == zlib.adler32(want), sc.name
        d = zlib.decompressobj()
        d.decompress(sc.stream)
        assert got.consumed == len(sc.stream) - len(d.unused_data), sc.name


def test_statement_status_is_nonzero_exactly_where_zlib_raises():
    for sc in R.malformed_streams():
        got = R.inflated(sc.name)
        assert got.status == sc.status != R.OK, (sc.name, got.status)
        assert not _zlib_accepts(sc.stream, sc.cap), sc.name
    for sc in R.good_streams():
        assert _zlib_accepts(sc.stream, sc.cap), sc.name


def test_handbuilt_stream_reaches_the_limits():
    stream, content = R.handbuilt()
    assert zlib.decompress(stream) == content and (len(stream), len(content)) == (34818, 36933)
    got = R.inflated("handbuilt")
    assert got.status == R.OK and got.out == content and got.tokens == 32768 + 49 + 56 + 5


@pytest.mark.parametrize("index", range(len(R.files())), ids=R.FILE_IDS)
def test_statement_decode_equals_pil(index):
    fc = R.files()[index]
    for order in ("bgr", "rgb"):
        got = R.decode(fc.data, order)
        assert got.status == R.OK and np.array_equal(got.pixels, R.decode_with_pil(fc.data, order)), order
    if fc.c == 1:
        assert np.array_equal(R.decode(fc.data, "bgr", 1).pixels, R.decode_with_pil(fc.data, "bgr", 1))


def test_corpus_covers_what_it_claims():
    names = " ".join(R.FILE_IDS)
    for w in R.WIDTHS:
        for h in R.HEIGHTS:
            assert f"shape-w{w}-h{h}-" in names
    for token in [f"-f{f}-" for f in R.FILTERS] + [f"-{s}-cut" for s in R.STREAMS] + [f"-cut{c}" for c in R.CUTS] + list(R.CONTENTS):
        assert token in names, token
    long = next(f for f in R.files() if f.name == "stored-long")
    assert len(R.walk(long.data).stream) > 65535 + 11
    assert R.inflated("stored-long").tokens == 0


def test_malformed_files_have_the_stated_status():
    for bf in R.malformed_files():
        if bf.status:
            assert R.decode(bf.data).status == bf.status, bf.name


def test_parse_png_raises_as_the_contract_says(tmp_path):
    for fc in R.files()[:8]:
        info = png.parse_png(fc.data)
        assert (info.height, info.width, info.bpp) == (fc.h, fc.w, fc.c)
        assert sum(idat for _, _, idat in info.chunks) >= 1 and info.chunks[0][:2] == (12, 13)
    for bf in R.malformed_files():
        if bf.error is ValueError:
            with pytest.raises(ValueError, match=bf.match) as err:
                png.parse_png(bf.data, "some/file.png")
            assert "some/file.png" in str(err.value)
        elif bf.status == 0:
            with pytest.raises(IOError, match="Failed to load frame: some/file.png"):
                png.parse_png(bf.data, "some/file.png")
        else:
            png.parse_png(bf.data)                     # only the device can tell
    with pytest.raises(ValueError, match="signature"):
        png.parse_png(b"")


def test_argument_checks_before_the_library_is_touched(tmp_path):
    good = R.files()[0].data
    colour = next(f for f in R.files() if f.c == 3).data
    for fn in (lambda **kw: png.decode_png_device([good], "cuda:0", **kw), lambda **kw: png.load_frames_device([tmp_path / "x.png"], "cuda:0", **kw)):
        with pytest.raises(ValueError, match="order"):
            fn(order="gbr")
        with pytest.raises(ValueError, match="channels"):
            fn(channels=2)
    with pytest.raises(ValueError, match="chunk_frames"):
        png.load_frames_device([tmp_path / "x.png"], "cuda:0", chunk_frames=0)
    with pytest.raises(ValueError, match="no files"):
        png.decode_png_device([], "cuda:0")
    with pytest.raises(ValueError, match="no paths"):
        png.load_frames_device([], "cuda:0")
    other = next(f for f in R.files() if (f.h, f.w) != (R.files()[0].h, R.files()[0].w)).data
    with pytest.raises(ValueError, match="the files before it"):
        png.decode_png_device([good, other], "cuda:0")
    with pytest.raises(ValueError, match="gray files only"):
        png.decode_png_device([colour], "cuda:0", channels=1)
    with pytest.raises(ValueError, match="palette"):
        png.decode_png_device([next(b for b in R.malformed_files() if b.name == "palette").data], "cuda:0")
    with pytest.raises(RuntimeError, match="MI355X"):
        png.decode_png_device([good], "cpu")
    with pytest.raises(ValueError, match="size"):
        png.inflate_device([b"x"], [1, 2], "cuda:0")


def _write_clip(d, n, h=16, w=24, seed=0):
    rng = np.random.default_rng(seed)
    for i in range(n):
        frameio.save_frame(rng.integers(0, 250, size=(h, w, 3), dtype=np.uint8), os.path.join(d, f"{i + 1:05d}.png"))


def test_png_reader_option_of_the_drivers(tmp_path):
    src = tmp_path / "src"
    _write_clip(str(src), 3)
    maps = np.ones((3, 2, 3), np.int32)
    calls = (
        lambda r: drivers.restore_downsampled_with_sinsr(str(src), str(tmp_path / "out"), maps, 8, devices=["cpu"], png_reader=r,
                                                         _shard_fn=_hooks.plus_device_tag),
        lambda r: drivers.restore_blur_adaptive(str(src), maps, 8, devices=["cpu"], png_reader=r, _shard_fn=_hooks.plus_device_tag),
        lambda r: drivers.restore_dct_adaptive(str(src), maps, 8, devices=["cpu"], png_reader=r, _shard_fn=_hooks.plus_device_tag),
    )
    for call in calls:
        with pytest.raises(ValueError, match="png_reader"):
            call("gpu")
        with pytest.raises(RuntimeError, match="png_reader='device' needs a GPU"):
            call("device")
    before = [frameio.load_frame(src / f"{i + 1:05d}.png") for i in range(3)]
    frameio.save_block_masks(np.zeros((3, 2, 3), np.uint8), tmp_path / "masks.npz")
    for fn, extra in ((drivers.stretch_shrunk_frames, {"out_dir": str(tmp_path / "s")}), (drivers.restore_shrunk_frames, {"out_dir": str(tmp_path / "r")})):
        with pytest.raises(ValueError, match="png_reader"):
            fn(str(src), str(tmp_path / "masks.npz"), 8, devices=["cpu"], png_reader="gpu", _shard_fn=_hooks.plus_device_tag, **extra)
        with pytest.raises(RuntimeError, match="png_reader='device' needs a GPU"):
            fn(str(src), str(tmp_path / "masks.npz"), 8, devices=["cpu"], png_reader="device", _shard_fn=_hooks.plus_device_tag, **extra)
    # the refused calls wrote nothing over the inputs, and the default is PIL
    assert all(np.array_equal(frameio.load_frame(src / f"{i + 1:05d}.png"), b) for i, b in enumerate(before))
    drivers.restore_downsampled_with_sinsr(str(src), str(tmp_path / "out"), maps, 8, devices=["cpu"], _shard_fn=_hooks.plus_device_tag)
    assert sorted(os.listdir(tmp_path / "out")) == [f"{i + 1:05d}.png" for i in range(3)]


def test_source_list_and_exports():
    import elvis_amd
    assert "png_read.hip" in _build.SOURCES
    assert elvis_amd.decode_png_device is png.decode_png_device and elvis_amd.load_frames_device is png.load_frames_device


# ----------------------------------------------------------------------------- mutants of the statement
def _file(name: str) -> R.FileCase:
    return next(f for f in R.files() if f.name.startswith(name))


@pytest.mark.parametrize("mutant, case", [("paeth_tie", "filter-4-c3"), ("average_round", "filter-3-c3")])
def test_unfilter_mutants_give_other_pixels(mutant, case):
    fc = _file(case)
    assert not np.array_equal(R.decode(fc.data, mutant=mutant).pixels, R.decode_with_pil(fc.data))


@pytest.mark.parametrize("mutant", ["no_wrap", "dist_extra_first", "code_not_reversed"])
def test_inflate_mutants_give_other_bytes_or_a_status(mutant):
    sc = next(s for s in R.good_streams() if s.name == "handbuilt")
    got = R.inflate(sc.stream, sc.cap, mutant)
    assert got.status != R.OK or got.out != zlib.decompress(sc.stream)
