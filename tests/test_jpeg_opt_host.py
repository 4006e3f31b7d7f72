"""Per-frame optimised Huffman tables of the JPEG writer without a GPU: the statement of tests/_jpeg_opt_ref.py against
PIL with `optimize=True` on libjpeg-turbo (the DHT segments, their position and everything behind SOS, byte for byte,
restart intervals included), what its corpus contains, the generated fixture that reaches the length-limit branch, its
mutants, the size condition, the library's host table builder through ctypes against the statement, the host half of
elvis_amd/jpeg_write.py (`jpeg_optimal_tables`, `jpeg_file_header(huffman=)`), the argument checks before the library is
touched, the `jpeg_optimize=` option of the directory drivers, and csrc/jpeg_encode.h - the tally sink, the table builder,
the bit count and the pack with a frame's own tables - walked over the corpus on the host under the address and
undefined-behaviour sanitizers (tools/jpeg_opt_check.cpp)."""
import inspect
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _hooks
import _jpeg_opt_ref as O
import _jpeg_ref as R
import _jpeg_restart_ref as S
import _jpeg_roi_ref as X
import elvis_amd
from elvis_amd import _lib, drivers, frameio, handoff, jpeg_write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
turbo = pytest.mark.skipif(not R.have_turbo(), reason="PIL is not built on libjpeg-turbo")


# ----------------------------------------------------------------------------- the corpus
def test_the_corpus_crosses_its_axes():
    cases = O.cases()
    assert len({c.name for c in cases}) == len(cases) >= 200
    assert O.SIZES == ((1, 1), (8, 8), (9, 17), (17, 33), (40, 56), (37, 53)) and O.QUALITIES == (30, 75, 95, 100)
    assert O.SETTINGS == ((0, 0), (1, 0), (2, 0), (0, 3)) and set(O.CONTENTS) == {"flat", "ramp", "noise", "smooth_noise"}
    axes = {"size": lambda c: (c.w, c.h), "sampling": lambda c: c.sampling, "quality": lambda c: c.quality, "kind": lambda c: c.kind,
            "restart": lambda c: (c.restart_rows, c.restart_mcus)}
    values = {"size": set(O.SIZES), "sampling": set(R.SAMPLINGS), "quality": set(O.QUALITIES), "kind": set(O.CONTENTS), "restart": set(O.SETTINGS)}
    for a, b in itertools.combinations(axes, 2):
        assert {(axes[a](c), axes[b](c)) for c in cases} == set(itertools.product(values[a], values[b])), (a, b)
    # restart intervals that cut a scan, and one whose last interval is short
    cut = [c for c in cases if O.encoded(c.name).ri and b"\xff\xd0" in O.encoded(c.name).scan]
    assert len(cut) > 60 and any(c.restart_mcus == 3 and (S.mcu_grid(c.w, c.h, c.channels, c.subsampling)[0] * S.mcu_grid(c.w, c.h, c.channels, c.subsampling)[1]) % 3
                                 for c in cut)
    # dummy blocks, ZRLs and a non-zero last coefficient all occur
    assert any(O.encoded(c.name).dummy.any() for c in cases)
    assert sum(int(O.encoded(c.name).hist[:, 16 + 0xF0].sum()) > 0 for c in cases) > 20
    assert any((O.encoded(c.name).blocks[:, 63] != 0).any() for c in cases)


def test_the_histogram_counts_the_symbols_of_the_scan_the_standard_file_holds():
    """The tally against two other walks: the number of symbols the reader's statement decodes from the Annex K file of the
    same frame, and the symbol writer of the reader's own test files, block by block, with the predictors kept here."""
    inverse = np.argsort(np.asarray(R.ZIGZAG))          # natural index -> zig-zag position
    for c in O.cases()[::5]:
        e = O.encoded(c.name)
        count = [0]
        R.entropy_decode(R.walk(e.standard), symbols=count)
        assert count[0] == int(e.hist.sum()), c.name
        _, _, bpm = S.mcu_grid(c.w, c.h, c.channels, c.subsampling)
        want = np.zeros((2, O.HUFF_WORDS), np.int64)
        pred = [0, 0, 0]
        for b, (blk, comp) in enumerate(zip(e.blocks.tolist(), e.comp.tolist())):
            if e.ri and b % (e.ri * bpm) == 0:
                pred = [0, 0, 0]
            symbols, pred[comp] = R.block_symbols([blk[inverse[k]] for k in range(64)], pred[comp])
            for kind, value, _, _ in symbols:
                want[min(comp, 1), (16 if kind == "ac" else 0) + value] += 1
        assert np.array_equal(e.hist, want), c.name


@turbo
@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_the_statement_equals_pil_with_optimize(sampling):
    mine = [c for c in O.cases() if c.sampling == sampling]
    assert len(mine) >= 50
    for c in mine:
        e = O.encoded(c.name)
        markers, dht, tail = O.dht_and_tail(e.data)
        pil_markers, pil_dht, pil_tail = O.dht_and_tail(O.pil_encode(c))
        want_markers = [0xC4] * (2 if c.channels == 1 else 4) + ([0xDD] if e.ri else []) + [0xDA]
        assert markers == pil_markers == want_markers, c.name
        assert dht == pil_dht == e.dht, c.name
        assert tail == pil_tail == e.scan + b"\xff\xd9", c.name
        # and PIL without optimize writes the standard file's scan: the two statements differ where PIL's two modes do
        assert O.dht_and_tail(O.pil_encode(c, optimize=False))[2] == O.dht_and_tail(e.standard)[2], c.name


def test_the_optimised_files_decode_to_the_standard_files_pixels():
    for c in O.cases()[::5]:
        e = O.encoded(c.name)
        got, want = R.decode(e.data, "rgb", c.channels), R.decode(e.standard, "rgb", c.channels)
        assert got.status == R.OK and np.array_equal(got.coef, want.coef) and np.array_equal(got.pixels, want.pixels), c.name
        if R.have_turbo():
            assert np.array_equal(got.pixels, R.decode_with_pil(e.data, "rgb", c.channels)), c.name


def test_the_optimised_scan_is_no_longer_than_the_standard_one():
    shorter = 0
    for c in O.cases() + (O.FIXTURE,):
        e = O.encoded(c.name)
        mine, std = len(O.dht_and_tail(e.data)[2]), len(O.dht_and_tail(e.standard)[2])
        assert mine <= std, (c.name, mine, std)
        shorter += mine < std
        assert max(e.prelimit) <= 16 or c is O.FIXTURE
    assert shorter > 150
    c = next(c for c in O.cases() if (c.w, c.h, c.quality, c.kind, c.sampling) == (40, 56, 95, "noise", "420"))
    e = O.encoded(c.name)
    assert len(e.data) < len(e.standard)             # whole files too, where the frame is not tiny


# ----------------------------------------------------------------------------- the length limit
@pytest.mark.parametrize("fixture,side,longest", [(O.FIXTURE, 520, 17), (O.FIXTURE17, 664, 18)])
def test_the_generated_fixture_reaches_the_length_limit(fixture, side, longest):
    frame = fixture.frame()
    assert frame.shape == (side, side, 1) and fixture.quality == 75 and fixture.sampling == "gray"
    e = O.encoded(fixture.name)
    count = int(fixture.kind[7:])
    # every block holds one AC coefficient, of the symbols and in the numbers the fixture names
    ac = e.hist[0, 16:]
    want = np.zeros(256, np.int64)
    for (run, cat), n in zip(O.fixture_symbols(count), O.fibonacci(count)):
        want[run << 4 | cat] = n
    want[0] = (side // 8) ** 2                              # EOB: every block
    assert np.array_equal(ac, want) and O.fibonacci(5) == [1, 2, 3, 5, 8]
    assert e.prelimit[1] == longest > 16                    # the limit step ran
    assert sum(e.tables[1][0]) == count + 1 and e.tables[1][0][15] > 0
    assert O.gen_optimal_table(ac, "limit_without_j_plus_1")[0] != e.tables[1][0]
    if R.have_turbo():
        assert O.dht_and_tail(O.pil_encode(fixture)) == O.dht_and_tail(e.data)


# ----------------------------------------------------------------------------- mutants
MUTANT_CASES = {
    "ties_to_smallest_index": "w8-h8-gray-q75-ramp-rows1",
    "no_reserved_symbol": "w1-h1-gray-q30-flat-none",
    "limit_without_j_plus_1": "fixture16-gray-q75",
    "order_by_frequency": "w8-h8-gray-q95-noise-rows2",
    "dc_not_reset": "w9-h17-gray-q75-noise-rows1",
    "dummies_not_counted": "w1-h1-422-q95-flat-none",
    "zrl_not_counted": "w8-h8-444-q95-smooth_noise-rows1",
}


def test_every_mutant_is_tried():
    assert set(MUTANT_CASES) == set(O.MUTANTS) and len(O.MUTANTS) == 7


@pytest.mark.parametrize("mutant", sorted(MUTANT_CASES))
def test_mutants_change_the_tables_of_their_case(mutant):
    c = O.case(MUTANT_CASES[mutant])
    want = O.encoded(c.name)
    got = O.encode(c.frame(), c.quality, c.subsampling, "rgb", **c.restart, mutant=mutant)
    assert got.tables != want.tables and got.dht != want.dht
    if mutant in ("dc_not_reset", "dummies_not_counted", "zrl_not_counted"):
        assert not np.array_equal(got.hist, want.hist)
    else:
        assert np.array_equal(got.hist, want.hist)
    if R.have_turbo():
        assert O.dht_and_tail(O.pil_encode(c))[1] == want.dht != got.dht


# ----------------------------------------------------------------------------- the library's builder
def _assert_builder_equals_statement(hist: np.ndarray, channels: int, what):
    tables, ehuff = jpeg_write.jpeg_optimal_tables(hist, channels)
    want, _ = O.frame_tables(hist, channels)
    assert tables == want, what
    assert ehuff.dtype == np.uint32 and np.array_equal(ehuff, O.code_words(want, channels)), what
    return tables


def test_the_c_abi_builder_equals_the_statement(built_lib):
    assert elvis_amd.jpeg_optimal_tables is jpeg_write.jpeg_optimal_tables
    assert _lib.SIGNATURES["elvis_jpeg_optimal_tables"] == [_lib.vp, _lib.i32, _lib.i32, _lib.vp, _lib.vp, _lib.vp, _lib.vp]
    for c in O.cases() + (O.FIXTURE, O.FIXTURE17):
        e = O.encoded(c.name)
        assert _assert_builder_equals_statement(e.hist, c.channels, c.name) == e.tables
    # a batch is its frames, each on its own
    batch = np.stack([O.encoded(c.name).hist for c in O.cases() if c.channels == 3][:40])
    tables, ehuff = jpeg_write.jpeg_optimal_tables(batch, 3)
    assert len(tables) == 40 and ehuff.shape == (40, 2, 272)
    for f in range(40):
        assert tables[f] == O.frame_tables(batch[f], 3)[0] and np.array_equal(ehuff[f], O.code_words(tables[f], 3))
    # random histograms: sparse and dense, small counts (many ties) and large ones
    rng = np.random.default_rng(5)
    for trial in range(60):
        hist = np.zeros((2, 272), np.int64)
        top = (3, 40, 1 << 12, 1 << 26)[trial % 4]
        for t in range(2):
            hist[t, :12] = rng.integers(0, top + 1, size=12) * (rng.random(12) < 0.7)
            hist[t, 16:] = rng.integers(0, top + 1, size=256) * (rng.random(256) < (0.05, 0.4, 1.0)[trial % 3])
            hist[t, 0] += 1
            hist[t, 16] += 1
        _assert_builder_equals_statement(hist, 3, trial)
    # Fibonacci counts: every length before limiting up to 32, DC tables up to 16
    for n in range(2, 33):
        hist = np.zeros((2, 272), np.int64)
        hist[0, 16:] = O.fibonacci_histogram(n)
        hist[0, :16] = O.fibonacci_histogram(min(n, 16), 16)
        assert O.gen_optimal_table(hist[0, 16:])[2] == n and O.gen_optimal_table(hist[0, :16])[2] == min(n, 16)
        tables = _assert_builder_equals_statement(hist, 1, n)
        assert sum(tables[1][0]) == n and len(tables[1][1]) == n
    # one symbol gets the code 0, two get 0 and 10: the reserved symbol keeps the all-ones codes
    hist = np.zeros((2, 272), np.int64)
    hist[0, 3], hist[0, 16 + 0x21] = 9, 1
    tables, ehuff = jpeg_write.jpeg_optimal_tables(hist, 1)
    assert tables == (((1,) + (0,) * 15, (3,)), ((1,) + (0,) * 15, (0x21,))) and ehuff[0, 3] == 1 and ehuff[0, 16 + 0x21] == 1
    assert not ehuff[1].any() and np.count_nonzero(ehuff[0]) == 2
    hist[0, 7], hist[0, 16] = 9, 500
    tables, ehuff = _assert_builder_equals_statement(hist, 1, "two"), jpeg_write.jpeg_optimal_tables(hist, 1)[1]
    assert tables == (((1, 1) + (0,) * 14, (3, 7)), ((1, 1) + (0,) * 14, (0x00, 0x21)))
    assert [int(ehuff[0, k]) for k in (3, 7, 16, 16 + 0x21)] == [1, 2 << 5 | 2, 1, 2 << 5 | 2]


def test_the_c_abi_builder_refuses_what_it_cannot_build(built_lib):
    h = _lib.lib()
    counts, symbols, nsym, ehuff = np.zeros(64, np.uint8), np.zeros(1024, np.uint8), np.zeros(4, np.int32), np.zeros(544, np.uint32)

    def call(hist, n=1, channels=1):
        return h.elvis_jpeg_optimal_tables(hist.ctypes.data, n, channels, counts.ctypes.data, symbols.ctypes.data, nsym.ctypes.data, ehuff.ctypes.data)

    empty = np.zeros((2, 272), np.uint32)
    assert call(empty) == -1 and b"no symbol" in h.elvis_last_error() and b"DC table 0" in h.elvis_last_error()
    dc_only = empty.copy()
    dc_only[0, 0] = 4
    assert call(dc_only) == -1 and b"AC table 0" in h.elvis_last_error()
    gray = dc_only.copy()
    gray[0, 16] = 4
    assert call(gray) == 0 and call(gray, channels=3) == -1 and b"DC table 1" in h.elvis_last_error()          # a gray clip builds tables 0 only
    too_many = gray.copy()
    too_many[0, 20] = (1 << 26) + 1
    assert call(too_many) == -1 and b"2^26" in h.elvis_last_error()
    assert call(gray, channels=2) == -1 and call(gray, n=-1) == -1 and call(gray, n=0) == 0
    assert h.elvis_jpeg_optimal_tables(None, 1, 1, counts.ctypes.data, symbols.ctypes.data, nsym.ctypes.data, ehuff.ctypes.data) == -1
    # a code that would pass 32 bits before limiting
    deep = empty.copy()
    deep[0, 0] = 1
    deep[0, 16:16 + 33] = O.fibonacci(33)
    assert call(deep) == -1
    with pytest.raises(ValueError, match="no symbol"):
        jpeg_write.jpeg_optimal_tables(empty, 1)
    for bad, match in ((empty.astype(np.float32), "integer"), (np.zeros((2, 271), np.uint32), "272"), (np.zeros((1, 3, 272), np.uint32), "272"),
                       (-np.ones((2, 272), np.int64), "2\\^26")):
        with pytest.raises(ValueError, match=match):
            jpeg_write.jpeg_optimal_tables(bad, 1)
    with pytest.raises(ValueError, match="channels"):
        jpeg_write.jpeg_optimal_tables(gray, 2)
    assert jpeg_write.jpeg_optimal_tables(np.zeros((0, 2, 272), np.uint32), 3)[0] == []
    header = open(os.path.join(ROOT, "include", "elvis_amd.h")).read()
    for word in ("jchuff.c", "jpeg_gen_optimal_table", "elvis_jpeg_tally", "elvis_jpeg_optimal_tables", "elvis_jpeg_bits_ftab", "elvis_jpeg_pack_ftab", "HOST ONLY"):
        assert word in header, word
    for name, count in (("elvis_jpeg_tally", 9), ("elvis_jpeg_bits_ftab", 10), ("elvis_jpeg_pack_ftab", 16)):
        assert len(_lib.SIGNATURES[name]) == count, name


# ----------------------------------------------------------------------------- the header
def test_the_file_header_takes_a_frames_own_tables():
    for name in ("w37-h53-420-q95-noise-rows1", "w40-h56-gray-q75-ramp-none", "w17-h33-444-q30-flat-mcus3"):
        c = O.case(next(k.name for k in O.cases() if k.name.startswith(name.rsplit("-", 3)[0]) and k.sampling == name.split("-")[2]))
        e = O.encoded(c.name)
        head = jpeg_write.jpeg_file_header(c.w, c.h, c.channels, c.quality, c.subsampling, e.ri, huffman=e.tables)
        assert head + e.scan + b"\xff\xd9" == e.data, c.name
        std = jpeg_write.jpeg_file_header(c.w, c.h, c.channels, c.quality, c.subsampling, e.ri)
        assert std == jpeg_write.jpeg_file_header(c.w, c.h, c.channels, c.quality, c.subsampling, e.ri, huffman=None) and std + O.dht_and_tail(e.standard)[2] == e.standard
        assert [m for m, _ in O.walk(head + b"\xff\xd9")[0]] == [m for m, _ in O.walk(std + b"\xff\xd9")[0]]
    # the Annex K tables handed in are the default header
    annex = (jpeg_write.STD_DC[0], jpeg_write.STD_AC[0], jpeg_write.STD_DC[1], jpeg_write.STD_AC[1])
    assert jpeg_write.jpeg_file_header(33, 17, 3, huffman=annex) == jpeg_write.jpeg_file_header(33, 17, 3)
    assert jpeg_write.jpeg_file_header(33, 17, 1, huffman=annex[:2]) == jpeg_write.jpeg_file_header(33, 17, 1)
    assert inspect.signature(jpeg_write.jpeg_file_header).parameters["huffman"].default is None


def test_a_bad_huffman_argument_is_a_value_error():
    dc, ac = jpeg_write.STD_DC[0], jpeg_write.STD_AC[0]
    one = ((1,) + (0,) * 15, (0,))
    bad = (
        ((dc, ac), 3), ((dc, ac, dc, ac), 1), ((dc,), 1), (5, 1), ((dc, 5), 1), (((dc[0], "ab"), ac), 1),          # the number and the shape
        (((dc[0][:15], dc[1]), ac), 1), ((((256,) + dc[0][1:], dc[1]), ac), 1), (((dc[0], dc[1][:11]), ac), 1),  # counts that do not add up
        ((((0,) * 16, ()), ac), 1),                                                                                # an empty table
        (((dc[0], (0,) * 12), ac), 1), (((dc[0], tuple(range(1, 13))), ac), 1), ((dc, (ac[0], (300,) + ac[1][1:])), 1),   # symbols twice, or out of range
        ((((2,) + (0,) * 15, (0, 1)), ac), 1), ((((1, 2) + (0,) * 14, (0, 1, 2)), ac), 1),                         # an all-ones code
        ((((3,) + (0,) * 15, (0, 1, 2)), ac), 1), ((one, ((0, 5) + (0,) * 14, (1, 2, 3, 4, 5))), 1),               # more codes than a length has
    )
    for huffman, channels in bad:
        with pytest.raises(ValueError, match="huffman"):
            jpeg_write.jpeg_file_header(16, 16, channels, huffman=huffman)
    assert jpeg_write.jpeg_file_header(16, 16, 1, huffman=(one, ((1, 1) + (0,) * 14, (0, 0x11))))          # small codes pass


# ----------------------------------------------------------------------------- argument checks, exports
def test_optimize_must_be_a_bool_before_the_library_is_touched(monkeypatch, tmp_path):
    def touched(*a, **kw):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(jpeg_write, "lib", touched)
    monkeypatch.setattr(handoff, "lib", touched)
    clip = torch.zeros((2, 17, 33, 3), dtype=torch.uint8)
    paths = [tmp_path / "a.jpg", tmp_path / "b.jpg"]
    imp = [np.ones((2, 4)), np.zeros((2, 4))]
    calls = (lambda **kw: jpeg_write.encode_jpeg_device(clip, **kw),
             lambda **kw: jpeg_write.save_jpeg_frames_device(clip, paths, **kw),
             lambda **kw: jpeg_write.save_jpeg_frames(clip.numpy(), paths, "cuda:0", **kw),
             lambda **kw: jpeg_write.jpeg_roundtrip_device(clip, **kw),
             lambda **kw: jpeg_write.jpeg_encoded_sizes_device(clip, **kw),
             lambda **kw: jpeg_write.jpeg_quality_for_bytes(clip, 1000, **kw),
             lambda **kw: jpeg_write.jpeg_roundtrip_at_bytes_device(clip, 1000, **kw),
             lambda **kw: handoff.encode_with_roi_device(clip, imp, 8, **kw))
    for fn in calls:
        for bad in (1, 0, None, "yes", 1.0):
            with pytest.raises(ValueError, match="optimize must be a bool"):
                fn(optimize=bad)
    # a good value goes on to the next check: the clip is not resident
    for fn in calls[:2] + calls[3:]:
        for good in (True, False, np.bool_(True)):
            with pytest.raises(ValueError, match="resident on the device"):
                fn(optimize=good)
    assert not os.listdir(tmp_path)


def test_the_new_names_are_exported_and_the_defaults_stand():
    assert elvis_amd.jpeg_optimal_tables is jpeg_write.jpeg_optimal_tables
    for fn in (jpeg_write.encode_jpeg_device, jpeg_write.save_jpeg_frames_device, jpeg_write.save_jpeg_frames, jpeg_write.jpeg_roundtrip_device,
               jpeg_write.jpeg_encoded_sizes_device, jpeg_write.jpeg_quality_for_bytes, jpeg_write.jpeg_roundtrip_at_bytes_device,
               handoff.encode_with_roi_device):
        p = inspect.signature(fn).parameters["optimize"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, fn.__name__
    assert inspect.signature(jpeg_write._encode_clip).parameters["optimize"].default is False
    for fn in (drivers.restore_downsampled_with_sinsr, drivers.restore_downsampled_with_realesrgan, drivers.restore_blur_adaptive, drivers.restore_dct_adaptive,
               drivers.stretch_shrunk_frames, drivers.restore_shrunk_frames):
        assert inspect.signature(fn).parameters["jpeg_optimize"].default is False, fn.__name__
    assert "third synchronisation" in jpeg_write._encode_clip.__doc__ and "THIRD SYNCHRONISATION" in jpeg_write.__doc__
    # the default probe of the search is the call it always was
    seen = []

    def fake_sizes(frames_d, quality=95, subsampling="420", order="bgr", **kw):
        seen.append(kw)
        return np.asarray([quality], np.int64)

    real = jpeg_write.jpeg_encoded_sizes_device
    jpeg_write.jpeg_encoded_sizes_device = fake_sizes
    try:
        jpeg_write.jpeg_quality_for_bytes(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 50)
        assert all("optimize" not in kw for kw in seen) and seen
        seen.clear()
        assert jpeg_write.jpeg_quality_for_bytes(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 50, optimize=True)[0] == 50
        assert all(kw["optimize"] is True for kw in seen) and seen
    finally:
        jpeg_write.jpeg_encoded_sizes_device = real


# ----------------------------------------------------------------------------- the drivers
def test_jpeg_optimize_option_of_the_drivers(tmp_path, monkeypatch):
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
        for kw in (dict(jpeg_optimize=True), dict(jpeg_optimize=True, jpeg_writer="pil")):
            with pytest.raises(ValueError, match=r"jpeg_optimize.*jpeg_writer"):
                call(**kw)
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match="jpeg_optimize must be a bool"):
                call(jpeg_optimize=bad, jpeg_writer="device")
        with pytest.raises(RuntimeError, match="jpeg_writer='device' needs a GPU"):
            call(jpeg_optimize=True, jpeg_writer="device")
    # the sink hands optimize= on only where it is set
    seen = []
    monkeypatch.setattr(jpeg_write, "save_jpeg_frames", lambda frames, paths, device, **kw: seen.append(("host", len(frames), list(paths), device, kw)))
    monkeypatch.setattr(jpeg_write, "save_jpeg_frames_device", lambda clip, paths, **kw: seen.append(("device", tuple(clip.shape), list(paths), kw)))
    out = tmp_path / "mixed"
    names = ["00001.jpg", "00002.png", "00003.JPEG"]
    frames = [rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8) for _ in names]
    plain, opt = dict(quality=95, subsampling="420"), dict(quality=95, subsampling="420", optimize=True)
    both = dict(quality=95, subsampling="420", restart_rows=2, optimize=True)
    jpgs = [os.path.join(str(out), names[0]), os.path.join(str(out), names[2])]
    drivers.PngDirSink(str(out), names, "pil", "device", 0, True).save(frames, 0, "cuda:0")
    drivers.PngDirSink(str(out), names, "pil", "device", 0, False).save(frames, 0, "cuda:0")
    drivers.PngDirSink(str(out), names, "pil", "device", jpeg_restart_rows=2, jpeg_optimize=True).save(frames, 0, "cuda:0")
    assert seen == [("host", 2, jpgs, "cuda:0", opt), ("host", 2, jpgs, "cuda:0", plain), ("host", 2, jpgs, "cuda:0", both)]
    seen.clear()
    clip = torch.from_numpy(np.stack(frames))
    drivers._write_clip(clip[:, :, :, 0], str(tmp_path / "masks"), ["1.jpg"] * 3, "pil", "device", 0, True)
    assert seen == [("device", (3, 8, 8), [os.path.join(str(tmp_path / "masks"), "1.jpg")] * 3, opt)]
    assert drivers._v1_kw("pil", "device", 0, True, stretched_dir=None) == {"stretched_dir": None, "jpeg_writer": "device", "jpeg_optimize": True}
    assert drivers._v1_kw("pil", "device", 1, stretched_dir=None) == {"stretched_dir": None, "jpeg_writer": "device", "jpeg_restart_rows": 1}


# ----------------------------------------------------------------------------- the kernels' text on the host
def test_the_encoder_header_walks_the_corpus_with_its_own_tables_under_the_sanitizers(tmp_path):
    """tools/jpeg_opt_check.cpp is a stand-alone program: it includes csrc/jpeg_encode.h and runs every case of the corpus
    and the length-limit fixture through the very functions the kernels and the host entry point call - the tally sink
    over a histogram a workgroup, the table builder into exact-size outputs, the bit count and the pack with the frame's
    own code words over exactly the words the host plans - and compares the histograms, the tables and the scan with the
    statement's.  Nothing is loaded into this process."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe, corpus = str(tmp_path / "jpeg_opt_check"), str(tmp_path / "corpus.bin")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tools", "jpeg_opt_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    O.dump(corpus)
    run = subprocess.run([exe, corpus], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "builder edges ok" in run.stdout and f"{len(O.cases()) + 1} cases, 0 failed" in run.stdout


def test_the_statement_takes_the_roi_dead_zone_and_the_channel_order():
    c = next(k for k in X.cases() if (k.w, k.sampling, k.kind, k.map_kind) == (53, "420", "noise", "all48"))
    frame, levels = c.frame(), c.levels()
    e = O.encode(frame, c.quality, c.subsampling, "rgb", levels=levels, B=c.B, restart_rows=1)
    assert e.standard == X.encode(frame, c.quality, c.subsampling, "rgb", levels, c.B, restart_rows=1).data
    assert np.array_equal(e.blocks, X.encoded(c.name).blocks) and len(e.data) < len(e.standard)
    got = R.decode(e.data, "rgb", c.channels)
    assert got.status == R.OK and np.array_equal(got.pixels, R.decode(e.standard, "rgb", c.channels).pixels)
    plain = O.encode(frame, c.quality, c.subsampling, "rgb", restart_rows=1)
    assert not np.array_equal(plain.hist, e.hist) and plain.tables != e.tables
    bgr = O.encode(frame[:, :, ::-1], c.quality, c.subsampling, "bgr", levels=levels, B=c.B, restart_rows=1)
    assert bgr.data == e.data
