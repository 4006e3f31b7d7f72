"""The JPEG reader's statement (tests/_jpeg_ref.py) against its oracle, PIL on libjpeg-turbo, and the reader's host side
(elvis_amd/jpeg.py: parse_jpeg, the layout, the argument checks, `load_images_device`'s dispatch, `png_reader=` of the
drivers) - no GPU.  The mutants show that the corpus tells the statement from its near misses."""
import os

import numpy as np
import pytest

import _hooks
import _jpeg_ref as R
from elvis_amd import _build, drivers, frameio, jpeg, png

turbo = pytest.mark.skipif(not R.have_turbo(), reason="PIL is not built on libjpeg-turbo: an IJG libjpeg 7+ upsamples differently; "
                                                      "the statement stands alone")
NOT_FOR_PIL = ("ff00-first-and-last",)       # a code of all 1 bits: libjpeg refuses the table


@turbo
@pytest.mark.parametrize("index", range(len(R.pil_files())), ids=[f.name for f in R.pil_files()])
def test_statement_equals_pil_on_every_pil_written_file(index):
    fc = R.pil_files()[index]
    for order in ("rgb", "bgr"):
        got = R.decoded(fc.name, order)
        assert got.status == R.OK and all(s == (R.OK, n) for s, n in zip(got.seg_status, _mcus(fc)))
        assert np.array_equal(got.pixels, R.decode_with_pil(fc.data, order)), order
    if fc.c == 1:
        assert np.array_equal(R.decoded(fc.name, "bgr", 1).pixels, R.decode_with_pil(fc.data, "bgr", 1))


def _mcus(fc):
    info = jpeg.parse_jpeg(fc.data)
    return [s[3] for s in info.segments]


@pytest.mark.parametrize("index", range(len(R.written_files())), ids=[f.name for f in R.written_files()])
def test_statement_decodes_the_writers_streams(index):
    fc = R.written_files()[index]
    got = R.decoded(fc.name)
    assert got.status == R.OK and got.pixels.shape == (fc.h, fc.w, 3)
    if R.have_turbo() and fc.name not in NOT_FOR_PIL:
        assert np.array_equal(got.pixels, R.decode_with_pil(fc.data))


def test_writers_streams_hold_what_they_claim():
    by = {f.name: f for f in R.written_files()}
    w = R.walk(by["code-16-bits"].data)
    assert w.dc[0][0][15] == 1 and w.ac[0][0][15] == 1
    codes = R.code_strings(*w.dc[0])
    assert "1" * 15 + "0" in codes and codes["1" * 15 + "0"] == 11        # category 11 has the 16-bit code ...
    assert R.decoded("code-16-bits").coef[0, 0] == 1500                   # ... and the first block uses it
    assert R.decoded("zrl-runs").coef[0, R.ZIGZAG[51]] == -7 * R.walk(by["zrl-runs"].data).qt[0][R.ZIGZAG[51]]
    assert (R.decoded("no-eob").coef[:4, 63] != 0).all()
    w = R.walk(by["ff00-first-and-last"].data)
    assert all(s[:2] == b"\xff\x00" and s[-2:] == b"\xff\x00" for s in w.segments) and len(w.segments) == 4
    for name, fill in (("fill-and-wrap", 2), ("wrap-444", 1)):
        data = by[name].data
        assert data.count(b"\xff" * (fill + 1) + b"\xd0") == 2 and data.endswith(b"\xff" * (fill + 1) + b"\xd9")
        assert len(R.walk(data).segments) >= 9
    data = by["sof1-16-bit-table"].data
    assert b"\xff\xc1" in data and data[data.index(b"\xff\xdb") + 4] == 0x10
    assert [c[0] for c in R.walk(by["other-ids-and-tables"].data).comps] == [7, 1, 4]


def test_corpus_covers_what_it_claims():
    names = " ".join(f.name for f in R.files())
    for w in R.WIDTHS:
        for h in R.HEIGHTS:
            assert f"shape-w{w}-h{h}-" in names
    for s in R.SAMPLINGS:
        for q in R.QUALITIES:
            for c in R.CONTENTS:
                assert f"full-{s}-q{q}-{c}" in names
        for token in (f"optimize-{s}", f"restart-blocks1-{s}", f"restart-blocks3-{s}", f"restart-rows1-{s}"):
            assert token in names
    # both clamps of the IDCT's range limit and of the colour conversion are reached
    reached = set()
    for fc in R.pil_files():
        reached |= R.decoded(fc.name).clamps
    assert reached == {"idct-low", "idct-high", "colour-low", "colour-high"}
    assert any(jpeg.parse_jpeg(f.data).restart_interval for f in R.pil_files())


def test_malformed_streams_have_the_stated_status():
    seen = set()
    for bf in R.device_bad_files():
        got = R.decoded(bf.name)
        assert got.status == bf.status != R.OK, (bf.name, got.seg_status)
        seen.add(bf.status)
    assert seen == {R.E_CODE, R.E_INDEX, R.E_BITS, R.E_RANGE}
    two = R.decoded("two-defects")
    assert [c for c, _ in two.seg_status if c] == [R.E_INDEX, R.E_CODE] and two.status == R.E_INDEX


def test_parse_jpeg_agrees_with_the_statements_walk():
    for fc in R.files() + R.extra_files():
        info, w = jpeg.parse_jpeg(fc.data, fc.name), R.walk(fc.data)
        assert (info.width, info.height, len(info.components)) == (fc.w, fc.h, fc.c)
        assert [(c.id, c.h, c.v, c.tq) for c in info.components] == w.comps
        assert [(c.td, c.ta) for c in info.components] == [(d, a) for _, d, a in w.scan]
        assert info.restart_interval == w.ri
        assert [fc.data[o:o + n] for o, n, _, _ in info.segments] == w.segments
        for t, table in w.qt.items():
            assert np.array_equal(info.qtables[t], table)
        for cls, tabs in ((0, w.dc), (1, w.ac)):
            for t, (counts, values) in tabs.items():
                assert (list(info.huffman[(cls, t)][0]), list(info.huffman[(cls, t)][1])) == (counts, values)
        g = R.geometry(fc.w, fc.h, w.comps)
        total = g.mcux * g.mcuy
        assert sum(s[3] for s in info.segments) == total and [s[2] for s in info.segments] == list(range(0, total, w.ri or total))
        plan = jpeg.plan_clip([info], [len(fc.data)])
        assert plan.stride_blocks == g.blocks == int(plan.fd[0, 5]) and [int(plan.fd[0, 10 + 8 * c]) for c in range(fc.c)] == g.base


def test_parse_jpeg_raises_as_the_contract_says():
    refused = {b.name for b in R.malformed_files() if b.error is ValueError}
    assert refused >= {"progressive", "lossless", "arithmetic", "twelve-bit", "two-components", "four-components", "sampling-1x2",
                       "two-scans", "dnl", "height-0", "adobe-transform-0", "rgb-ids"}
    broken = {b.name for b in R.malformed_files() if b.error is IOError and not b.status}
    assert broken >= {"no-soi", "no-sof", "no-sos", "no-eoi", "length-past-the-end", "quantisation-table-not-defined",
                      "huffman-table-not-defined", "huffman-over-subscribed", "huffman-more-than-256", "rst-out-of-sequence",
                      "segment-count"}
    for bf in R.malformed_files():
        if bf.error is ValueError:
            with pytest.raises(ValueError, match=bf.match) as err:
                jpeg.parse_jpeg(bf.data, "some/file.jpg")
            assert "some/file.jpg" in str(err.value), bf.name
        elif bf.status == 0:
            with pytest.raises(IOError, match="Failed to load frame: some/file.jpg"):
                jpeg.parse_jpeg(bf.data, "some/file.jpg")
        else:
            jpeg.parse_jpeg(bf.data)                    # only the device can tell
    with pytest.raises(IOError):
        jpeg.parse_jpeg(b"")


def test_exif_orientation_is_ignored():
    from PIL import Image
    import io
    img = Image.fromarray(R.make_content("ramp", 16, 24, 3, 1))
    exif = Image.Exif()
    exif[0x0112] = 6
    buf = io.BytesIO()
    img.save(buf, "JPEG", exif=exif)
    info = jpeg.parse_jpeg(buf.getvalue())
    assert (info.height, info.width) == (16, 24)
    if R.have_turbo():
        assert np.array_equal(R.decode(buf.getvalue()).pixels, R.decode_with_pil(buf.getvalue()))


def test_argument_checks_before_the_library_is_touched(tmp_path):
    gray = next(f for f in R.files() if f.c == 1)
    colour = next(f for f in R.files() if f.c == 3)
    for fn in (lambda **kw: jpeg.decode_jpeg_device([gray.data], "cuda:0", **kw),
               lambda **kw: jpeg.load_jpeg_frames_device([tmp_path / "x.jpg"], "cuda:0", **kw),
               lambda **kw: jpeg.load_images_device([tmp_path / "x.jpg"], "cuda:0", **kw)):
        with pytest.raises(ValueError, match="order"):
            fn(order="gbr")
        with pytest.raises(ValueError, match="channels"):
            fn(channels=2)
    with pytest.raises(ValueError, match="chunk_frames"):
        jpeg.load_jpeg_frames_device([tmp_path / "x.jpg"], "cuda:0", chunk_frames=0)
    with pytest.raises(ValueError, match="no files"):
        jpeg.decode_jpeg_device([], "cuda:0")
    with pytest.raises(ValueError, match="no paths"):
        jpeg.load_jpeg_frames_device([], "cuda:0")
    with pytest.raises(ValueError, match="no paths"):
        jpeg.load_images_device([], "cuda:0")
    other = next(f for f in R.files() if (f.h, f.w) != (gray.h, gray.w))
    with pytest.raises(ValueError, match="the files before it"):
        jpeg.decode_jpeg_device([gray.data, other.data], "cuda:0")
    with pytest.raises(ValueError, match="gray files only"):
        jpeg.decode_jpeg_device([colour.data], "cuda:0", channels=1)
    with pytest.raises(ValueError, match="progressive"):
        jpeg.decode_jpeg_device([next(b for b in R.malformed_files() if b.name == "progressive").data], "cuda:0")
    with pytest.raises(RuntimeError, match="MI355X"):
        jpeg.decode_jpeg_device([gray.data], "cpu")
    with pytest.raises(IOError, match="Failed to load frame: .*missing.jpg"):
        jpeg.load_images_device([tmp_path / "missing.jpg"], "cuda:0")


def test_load_images_device_dispatches_by_the_first_bytes(tmp_path, monkeypatch):
    rng = np.random.default_rng(0)
    pngs = [tmp_path / f"{i}.png" for i in range(3)]
    for p in pngs:
        frameio.save_frame(rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8), p)
    jpg_as_png = tmp_path / "jpeg-inside.png"
    jpg_as_png.write_bytes(R.files()[0].data)
    calls = []
    monkeypatch.setattr(png, "load_frames_device", lambda *a, **kw: calls.append(("png", a, kw)) or "png clip")
    monkeypatch.setattr(jpeg, "load_jpeg_frames_device", lambda *a, **kw: calls.append(("jpeg", a, kw)) or "jpeg clip")
    # a list that is all PNG is exactly one call of png.load_frames_device, looked up at the call
    assert jpeg.load_images_device(pngs, "cuda:0", "rgb", 3, 2) == "png clip"
    assert calls == [("png", (pngs, "cuda:0", "rgb", 3, 2), {})]
    calls.clear()
    assert jpeg.load_images_device([jpg_as_png], "cuda:0") == "jpeg clip"
    assert calls == [("jpeg", ([jpg_as_png], "cuda:0", "bgr", 3, None), {})]
    text = tmp_path / "notes.png"
    text.write_bytes(b"plain text")
    with pytest.raises(ValueError, match="neither a PNG nor a JPEG"):
        jpeg.load_images_device([pngs[0], text], "cuda:0")


def _write_jpg_clip(d, n, h=16, w=24, seed=0):
    rng = np.random.default_rng(seed)
    for i in range(n):
        frameio.save_frame(rng.integers(0, 250, size=(h, w, 3), dtype=np.uint8), os.path.join(d, f"{i + 1:05d}.jpg"))


def test_png_reader_option_of_the_drivers_on_a_jpg_directory(tmp_path, monkeypatch):
    src = tmp_path / "src"
    _write_jpg_clip(str(src), 3)
    maps = np.ones((3, 2, 3), np.int32)
    calls = (
        lambda r: drivers.restore_downsampled_with_sinsr(str(src), str(tmp_path / "out"), maps, 8, devices=["cpu"], png_reader=r,
                                                         _shard_fn=_hooks.plus_device_tag),
        lambda r: drivers.restore_blur_adaptive(str(src), maps, 8, devices=["cpu"], png_reader=r, _shard_fn=_hooks.plus_device_tag),
    )
    for call in calls:
        with pytest.raises(ValueError, match="png_reader"):
            call("gpu")
        with pytest.raises(RuntimeError, match="png_reader='device' needs a GPU"):
            call("device")
    # the v1 drivers take their frames under the names 00001.png ...: JPEG data under those names
    v1 = tmp_path / "v1"
    v1.mkdir()
    for i in range(3):
        (v1 / f"{i + 1:05d}.png").write_bytes((src / f"{i + 1:05d}.jpg").read_bytes())
    frameio.save_block_masks(np.zeros((3, 2, 3), np.uint8), tmp_path / "masks.npz")
    with pytest.raises(RuntimeError, match="png_reader='device' needs a GPU"):
        drivers.restore_shrunk_frames(str(v1), str(tmp_path / "masks.npz"), 8, out_dir=str(tmp_path / "r"), devices=["cpu"],
                                      png_reader="device", _shard_fn=_hooks.plus_device_tag)
    # the source of a "device" reader hands its paths to load_images_device, .jpg files included
    seen = []
    monkeypatch.setattr(jpeg, "load_images_device", lambda paths, device: seen.append((list(paths), device)) or "clip")
    source = drivers.PngDirSource(str(src), [f"{i + 1:05d}.jpg" for i in range(3)], "device")
    assert source.load(1, 3, "cuda:0") == "clip"
    assert seen == [([os.path.join(str(src), "00002.jpg"), os.path.join(str(src), "00003.jpg")], "cuda:0")]
    # the default is PIL, and it reads the .jpg directory as before
    drivers.restore_downsampled_with_sinsr(str(src), str(tmp_path / "out"), maps, 8, devices=["cpu"], _shard_fn=_hooks.plus_device_tag)
    assert sorted(os.listdir(tmp_path / "out")) == [f"{i + 1:05d}.jpg" for i in range(3)]


def test_source_list_and_exports():
    import elvis_amd
    assert "jpeg_read.hip" in _build.SOURCES
    for name in ("parse_jpeg", "decode_jpeg_device", "load_jpeg_frames_device", "load_images_device"):
        assert getattr(elvis_amd, name) is getattr(jpeg, name)
    assert elvis_amd.load_frames_device is png.load_frames_device
    assert jpeg.TABLE_BYTES == 1312 and "#define ELVIS_JPEG_TABLE_BYTES 1312" in open(
        os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "elvis_amd.h")).read()


# ----------------------------------------------------------------------------- mutants of the statement
MUTANT_CASES = {
    "h2v2_round_swapped": "full-420-q75-noise",
    "h2v1_first": "full-422-q75-noise",
    "column_no_round": "full-444-q75-noise",
    "g_no_round": "full-444-q95-noise",
    "extend_off_by_one": "full-gray-q75-noise",
    "dc_no_reset": "restart-blocks1-420",
    "zigzag_transposed": "full-422-q95-ramp",
}


def test_every_mutant_is_tried():
    assert set(MUTANT_CASES) == set(R.MUTANTS) and len(R.MUTANTS) >= 6


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_give_other_pixels_or_a_status(mutant):
    fc = next(f for f in R.files() if f.name == MUTANT_CASES[mutant])
    want = R.decoded(fc.name)
    got = R.decode(fc.data, mutant=mutant)
    assert want.status == R.OK
    assert got.status != R.OK or not np.array_equal(got.pixels, want.pixels)
