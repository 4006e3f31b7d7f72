"""The run-length stream of the device PNG writer (`deflate="rle"`) without a GPU: its statement (tests/_png_rle_ref.py)
against zlib and PIL on every case of the matrix, the planner against the statement's offsets, the code builder on 257 bins
as before and on 286, the named mutants, the new arguments and the drivers' "device-rle" switch."""
import hashlib
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import _png_ref as R
import _png_rle_ref as S
from elvis_amd import drivers, frameio, png
from test_png_host import BUILDER_HISTS


# ----------------------------------------------------------------------------- the statement against zlib and PIL
@pytest.mark.parametrize("index", range(len(S.CASES)), ids=S.CASE_IDS)
def test_statement_decodes_with_zlib_and_pil(index):
    case = S.CASES[index]
    frames = case.frames()
    for frame, enc in zip(frames, S.expected(index)):
        assert zlib.decompress(b"".join(enc.payloads)) == enc.stream
        assert np.array_equal(R.decode_with_pil(enc.file, case.order).reshape(frame.shape), frame)
        chunks = R.parse_chunks(enc.file)
        assert [k for k, _, _, _ in chunks] == [b"IHDR"] + [b"IDAT"] * len(enc.payloads) + [b"IEND"]
        for kind, body, crc, _ in chunks:
            assert zlib.crc32(kind + body) == crc


def test_token_rule_on_the_run_edges():
    """The rule itself, token by token, on the lengths where it changes."""
    m258 = (285, 0, 0)
    for length, want in {1: [], 2: [7], 3: [7, 7], 4: [(257, 0, 0)], 259: [m258], 260: [m258, 7], 261: [m258, 7, 7],
                         262: [m258, (257, 0, 0)], 517: [m258, m258], 518: [m258, m258, 7], 519: [m258, m258, 7, 7],
                         520: [m258, m258, (257, 0, 0)], 258: [(284, 30, 5)], 14: [(266, 0, 1)], 15: [(266, 1, 1)]}.items():
        got = S.span_tokens(np.full(length, 7, dtype=np.uint8))
        assert got[0] == (0, 7, 0, 0)
        assert [t[1:] if t[1] > 256 else t[1] for t in got[1:]] == want, length
    # nothing crosses a span or a type byte: a flat row of 4096 + 3 bytes whose type byte equals them
    row = np.full(1 + 4096 + 3, 1, dtype=np.uint8)
    tokens = S.row_tokens(row)
    assert tokens[0] == (0, 1, 0, 0) and tokens[1] == (0, 1, 0, 0)
    assert sum(S.LENGTH_BASE[t[1] - 257] + t[2] if t[1] > 256 else 1 for t in tokens) == row.size
    assert [t[1] for t in tokens[-3:]] == [1, 1, 1], "the second span's 3 bytes are a literal and a remainder of 2"
    assert [S.length_symbol(n)[0] for n in (3, 10, 11, 12, 13, 257, 258)] == [257, 264, 265, 265, 266, 284, 285]


def test_matrix_reaches_every_edge():
    names = set(S.CASE_IDS)
    assert {f"run-w{w}" for w in (1, 2, 3, 4, 258, 259, 260, 261, 262, 517, 518, 519, 520)} <= names
    assert {f"span-w{w}" for w in (4095, 4096, 4097, 4098, 4099, 4355)} <= names and "span-rgb-1366" in names
    for h in (1, 15, 16, 17, 33):
        assert {c.segment_rows for c in S.CASES if c.h == h and c.name.startswith("seg-")} == {1, 16, h + 1}
    assert {c.content for c in S.CASES} >= {"zeros", "full", "rect", "noise", "hramp", "vramp", "diag", "period9"}
    assert {c.filt for c in S.CASES} == {"adaptive", 0, 1, 2, 3, 4} and {c.order for c in S.CASES} == {"bgr", "rgb"}
    assert {c.n for c in S.CASES} >= {1, 3} and {c.offset for c in S.CASES} == {0, 1, 2, 3}
    assert max(c.w * c.c for c in S.CASES) == 4355, "the widest case is one 4 355-byte row"
    used, ends = set(), set()
    for i in range(len(S.CASES)):
        for enc in S.expected(i):
            used.update(np.flatnonzero(enc.lengths[257:]) + 257)
            ends.update((off + 12 + len(p)) % 4 for off, p in zip(enc.chunk_offsets, enc.payloads))
    assert {257, 285} <= used and len(used) >= 12, "short, long and extra-bit matches all occur"
    assert 0 in ends and ends - {0}, "both dword-aligned and unaligned segment ends must occur"
    # noise has no matches; a forced type 1 on a ramp of step 1 makes a type byte equal the run behind it
    noise = S.expected(S.CASE_IDS.index("content-noise-f0"))[0]
    assert not noise.lengths[257:].any()
    ones = S.expected(S.CASE_IDS.index("type-byte-run"))[0]
    assert (np.frombuffer(ones.stream, dtype=np.uint8) == 1).all() and len(ones.stream) == 3 * 301


def test_size_of_flat_frames_and_masks():
    """The statement meets the size conditions the device files are held to (they equal it bit for bit)."""
    for value in (0, 255):
        enc = S.encode(np.full((64, 96, 3), value, dtype=np.uint8), "bgr", "adaptive", 16)
        assert len(enc.stream) == 18496 and len(enc.file) < 1156, len(enc.file)
        assert len(R.encode(np.full((64, 96, 3), value, dtype=np.uint8), "bgr", "adaptive", 16).file) >= 2312
    enc = S.encode(S.make_content("rect", 1, 64, 96, 1, 0)[0], "bgr", "adaptive", 16)
    assert len(enc.stream) == 6208 and len(enc.file) < 6208 // 4, len(enc.file)


# ----------------------------------------------------------------------------- the code builder, the header, the planner
@pytest.mark.parametrize("name", list(BUILDER_HISTS))
def test_code_builder_on_257_bins_is_unchanged(name):
    """Recorded from the builder before it took the alphabet size: (length: how many symbols have it, SHA-1 of the uint8
    lengths)."""
    recorded = {
        "fibonacci-30": ({0: 226, 2: 2, 3: 2, 4: 2, 5: 2, 6: 2, 7: 2, 8: 2, 9: 2, 10: 2, 11: 2, 12: 2, 13: 2, 14: 1, 15: 6},
                         "f2340e083e7aec4f4b06c1d3f5f977b3e350717f"),
        "one-symbol-and-eob": ({0: 255, 1: 2}, "1ba6763193b678cdb47973fd82069413a943617a"),
        "all-257-equal": ({8: 255, 9: 2}, "9164a65bb91ee2430bf022185ea75a198f988048"),
        "six-million-zeros": ({0: 252, 1: 1, 2: 1, 3: 1, 4: 2}, "9c57425494cb6459e619df80bdb8b038206a3a3e"),
    }
    hist = BUILDER_HISTS[name]
    lens = png.limited_code_lengths(hist)
    assert np.array_equal(lens, png.limited_code_lengths(hist, symbols=257)) and lens.shape == (257,) and lens.dtype == np.uint8
    counts = {int(l): int((lens == l).sum()) for l in np.unique(lens)}
    assert counts == recorded[name][0]
    assert hashlib.sha1(lens.tobytes()).hexdigest() == recorded[name][1]
    # the same counts in a 286-bin histogram whose length symbols are unused give the same code
    wide = png.limited_code_lengths(np.concatenate([hist, np.zeros(29, dtype=np.int64)]), symbols=286)
    assert wide.shape == (286,) and np.array_equal(wide[:257], lens) and not wide[257:].any()
    with pytest.raises(ValueError):
        png.limited_code_lengths(hist, symbols=286)
    with pytest.raises(ValueError):
        png.limited_code_lengths(np.zeros(286), symbols=257)


def test_code_builder_on_286_bins():
    hist = np.zeros(286, dtype=np.int64)
    hist[[0, 255, 256, 257, 270, 285]] = [40, 3, 4, 9, 1, 6000]
    lens = png.limited_code_lengths(hist, symbols=286)
    assert np.array_equal(lens > 0, hist > 0) and sum(2 ** (15 - int(l)) for l in lens[lens > 0]) == 2 ** 15
    assert lens[285] == 1 and lens[270] == lens.max()


def test_header_agrees_with_the_statement():
    hist = np.zeros(286, dtype=np.int64)
    hist[[0, 9, 256, 260, 285]] = [500, 3, 2, 7, 90]
    lens = png.limited_code_lengths(hist, symbols=286)
    for final in (False, True):
        acc, n = png.block_header_bits_rle(lens, final)
        w = R.BitWriter()
        S.header(w, lens, final)
        assert n == w.n == png.RLE_HEADER_BITS == 1222 and acc == w.acc
    assert (png.RLE_HEADER_BITS + 31) // 32 == png.RLE_HEADER_WORDS == 39
    assert png.RLE_TAB_HEADER + png.RLE_HEADER_WORDS <= png.RLE_FRAME_TAB and png.RLE_STATS_STRIDE == 286 + 4
    assert tuple(png.RLE_LENGTH_EXTRA) == S.LENGTH_EXTRA and png.RLE_SPAN == S.SPAN
    with pytest.raises(ValueError):
        png.block_header_bits_rle(lens[:257])


@pytest.mark.parametrize("name", ["content-rect-fadaptive", "content-zeros-f0", "content-noise-f4", "run-w261", "span-w4355",
                                  "span-rgb-1366", "seg-h33-s16", "seg-h17-s1"])
def test_planner_against_the_statement(name):
    index = S.CASE_IDS.index(name)
    case, encs = S.CASES[index], S.expected(index)
    stats = np.stack([S.segment_stats(e, case.h, case.w * case.c + 1, case.segment_rows) for e in encs])
    plan = png.plan_layout_rle(stats)
    nseg = len(encs[0].payloads)
    for f, enc in enumerate(encs):
        assert int(plan.file_offsets[f + 1] - plan.file_offsets[f]) == len(enc.file)
        assert int(plan.adler[f]) == zlib.adler32(enc.stream) == struct.unpack(">I", enc.payloads[-1][-4:])[0]
        assert np.array_equal(plan.lengths[f], enc.lengths)
        for s in range(nseg):
            off, dl = plan.chunks[f * nseg + s]
            assert int(off - plan.file_offsets[f]) == enc.chunk_offsets[s] and int(dl) == len(enc.payloads[s])
        words = plan.frame_tab[f, png.RLE_TAB_HEADER:png.RLE_TAB_HEADER + png.RLE_HEADER_WORDS]
        assert sum(int(wd) << (32 * k) for k, wd in enumerate(words)) == png.block_header_bits_rle(enc.lengths)[0]
        assert int(plan.frame_tab[f, png.RLE_TAB_ADLER]) == int(plan.adler[f])
        assert np.array_equal(plan.frame_tab[f, :286], png.code_entries(enc.lengths))
    with pytest.raises(ValueError):
        png.plan_layout_rle(np.zeros((1, 2, png.STATS_STRIDE), dtype=np.uint32))
    with pytest.raises(ValueError):
        png.plan_layout(np.zeros((1, 2, png.RLE_STATS_STRIDE), dtype=np.uint32))


# ----------------------------------------------------------------------------- mutants
def _accepted(enc) -> bool:
    """True when zlib inflates the joined IDAT data to the filtered stream."""
    try:
        return zlib.decompress(b"".join(enc.payloads)) == enc.stream
    except zlib.error:
        return False


def _mutant_frame(mutant):
    if mutant == "runs_cross_type_byte":       # forced type 1 on a ramp of step 1: the type byte equals the run behind it
        return S.make_content("step1", 1, 5, 40, 1, 0)[0], 1
    a = S.make_content("period9", 1, 17, 300, 1, 0)[0]      # runs of 3 (a remainder of 2) and of 4 (a match)
    a[3:9, 20:290] = 255
    return a, 0


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_named_mutants_are_caught(mutant):
    frame, filt = _mutant_frame(mutant)
    good = S.encode(frame, "rgb", filt, 16)
    bad = S.encode(frame, "rgb", filt, 16, mutant=mutant)
    assert _accepted(good) and np.array_equal(R.decode_with_pil(good.file, "rgb").reshape(frame.shape), frame)
    assert good.lengths[257:].any(), "the frame has matches"
    assert bad.file != good.file, f"the mutant {mutant} gives the same bytes"
    if mutant != "runs_cross_type_byte":       # that one is a valid stream of the same pixels, only not this contract's bytes
        assert not _accepted(bad), f"zlib accepts the mutant {mutant}"


# ----------------------------------------------------------------------------- arguments and the drivers' switch
def test_deflate_argument_before_the_library_is_touched(built_lib, tmp_path, monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(png, "lib", touched)
    ok = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    for bad in ("x", "RLE", None, 1, b"rle"):
        with pytest.raises(ValueError, match="deflate"):
            png.encode_png_device(ok, deflate=bad)
        with pytest.raises(ValueError, match="deflate"):
            png.save_frames_device(ok, [tmp_path / "a.png"], deflate=bad)
        with pytest.raises(ValueError, match="deflate"):
            png.save_frames([np.zeros((4, 4, 3), np.uint8)], [tmp_path / "a.png"], "cuda:0", deflate=bad)
    with pytest.raises(ValueError, match="resident"):
        png.encode_png_device(ok, deflate="rle")                            # the other checks still come first
    assert not os.path.exists(tmp_path / "a.png")
    assert png.DEFLATES == ("literal", "rle")


def test_c_boundary_of_the_rle_entry_points(built_lib):
    h = png.lib()
    assert h.elvis_png_stats_rle(16, 16, 16, 1, 4, 4, 2, 0, -1, 16, None) == -1 and b"channels" in h.elvis_last_error()
    assert h.elvis_png_stats_rle(16, 16, 16, 1, 0, 4, 3, 0, -1, 16, None) == -1
    assert h.elvis_png_stats_rle(16, 16, 16, 1, 4, 0, 3, 0, -1, 16, None) == -1
    assert h.elvis_png_stats_rle(16, 16, 16, 1, 4, 4, 3, 2, -1, 16, None) == -1 and b"order" in h.elvis_last_error()
    assert h.elvis_png_stats_rle(16, 16, 16, 1, 4, 4, 3, 0, 5, 16, None) == -1 and b"filter" in h.elvis_last_error()
    assert h.elvis_png_stats_rle(16, 16, 16, 1, 4, 4, 3, 0, -1, 0, None) == -1 and b"segment_rows" in h.elvis_last_error()
    assert h.elvis_png_stats_rle(16, 16, 16, 2, 32768, 10923, 3, 0, -1, 16, None) == -1 and b"2^31" in h.elvis_last_error()
    assert h.elvis_png_stats_rle(None, 16, 16, 1, 4, 4, 3, 0, -1, 16, None) == -1 and b"null" in h.elvis_last_error()
    assert b"elvis_png_stats_rle" in h.elvis_last_error()
    assert h.elvis_png_stats_rle(None, None, None, 0, 4, 4, 3, 0, -1, 16, None) == 0                 # n = 0: nothing to do
    assert h.elvis_png_pack_rle(16, 16, 16, 16, 16, 100, 1, 4, 4, 3, 0, 0, None) == -1
    assert h.elvis_png_pack_rle(16, 16, 16, 16, 18, 100, 1, 4, 4, 3, 0, 16, None) == -1 and b"aligned" in h.elvis_last_error()
    assert h.elvis_png_pack_rle(16, 16, None, 16, 16, 100, 1, 4, 4, 3, 0, 16, None) == -1
    assert h.elvis_png_pack_rle(None, None, None, None, None, 0, 0, 4, 4, 3, 0, 16, None) == 0


def _plus_one(frames, maps, block_size, device, first_frame_index, **kw):
    return [f + 1 for f in frames]


def test_device_rle_writer_needs_a_gpu_and_writes_nothing(tmp_path):
    assert drivers.PNG_WRITERS == ("pil", "device", "device-rle")
    src = tmp_path / "src"
    rng = np.random.default_rng(2)
    for i in range(3):
        frameio.save_frame(rng.integers(0, 200, size=(16, 24, 3), dtype=np.uint8), os.path.join(src, f"{i + 1:05d}.png"))
    maps = np.ones((3, 2, 3), dtype=np.int32)
    frameio.save_block_masks(np.zeros((3, 2, 3), dtype=np.uint8), str(tmp_path / "m.npz"))
    calls = [
        lambda **k: drivers.restore_downsampled_with_sinsr(str(src), str(tmp_path / "o"), maps, 8, devices=["cpu"], _shard_fn=_plus_one, **k),
        lambda **k: drivers.restore_blur_adaptive(str(src), maps, 8, devices=["cpu"], _shard_fn=_plus_one, **k),
        lambda **k: drivers.restore_dct_adaptive(str(src), maps, 8, devices=["cpu"], _shard_fn=_plus_one, **k),
        lambda **k: drivers.stretch_shrunk_frames(str(src), str(tmp_path / "m.npz"), 8, devices=["cpu"], _shard_fn=_plus_one, **k),
        lambda **k: drivers.restore_shrunk_frames(str(src), str(tmp_path / "m.npz"), 8, str(tmp_path / "o2"), devices=["cpu"],
                                                  _shard_fn=_plus_one, **k),
    ]
    before = [open(src / f"{i + 1:05d}.png", "rb").read() for i in range(3)]
    for call in calls:
        with pytest.raises(RuntimeError, match="device-rle"):
            call(png_writer="device-rle")                   # a CPU device: there is no CPU path
        with pytest.raises(ValueError, match="png_writer"):
            call(png_writer="rle")
    assert before == [open(src / f"{i + 1:05d}.png", "rb").read() for i in range(3)], "a refused call must write nothing"
    for d in ("o", "o2"):
        assert not os.path.exists(tmp_path / d) or not os.listdir(tmp_path / d)
