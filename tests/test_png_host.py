"""The device PNG writer's host side (elvis_amd/png.py) and its statement (tests/_png_ref.py), without a GPU: the literal-code
builder's properties, every case of the matrix through the statement against zlib and PIL, the Adler combine and the layout
planner against zlib and the statement's offsets, the named mutants, the argument checks and the drivers' switch."""
import heapq
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import _png_ref as R
from elvis_amd import _build, drivers, frameio, png


# ----------------------------------------------------------------------------- the code builder
def _fibonacci(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f


def _hist(pairs, eob):
    h = np.zeros(257, dtype=np.int64)
    for s, n in pairs:
        h[s] = n
    h[256] = eob
    return h


BUILDER_HISTS = {
    "fibonacci-30": _hist(list(enumerate(_fibonacci(30))), 1),
    "one-symbol-and-eob": _hist([(77, 1000)], 3),
    "all-257-equal": np.full(257, 5, dtype=np.int64),
    "six-million-zeros": _hist([(0, 6_000_000), (9, 1), (100, 1), (255, 1)], 68),
}


def _plain_huffman_depth(hist):
    heap = [(int(n), i, 0) for i, n in enumerate(hist) if n]
    heapq.heapify(heap)
    tick = len(hist)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], tick, max(a[2], b[2]) + 1))
        tick += 1
    return heap[0][2]


@pytest.mark.parametrize("name", list(BUILDER_HISTS))
def test_code_builder_is_limited_complete_and_deterministic(name):
    hist = BUILDER_HISTS[name]
    lens = png.limited_code_lengths(hist)
    assert lens.shape == (257,) and int(lens.max()) <= 15
    used = lens[lens > 0]
    assert sum(2 ** (15 - int(l)) for l in used) == 2 ** 15            # Kraft sum exactly 1, in integers
    assert np.array_equal(lens > 0, hist > 0)                           # every used symbol is coded, no other
    assert np.array_equal(lens, png.limited_code_lengths(hist.copy()))  # deterministic
    # a rarer symbol never gets a shorter code
    order = np.argsort(hist[hist > 0], kind="stable")
    assert np.all(np.diff(lens[hist > 0][order].astype(int)) <= 0)
    # equal counts: ties go by symbol value - the lengths do not grow with the symbol among equals
    if name == "all-257-equal":
        assert set(lens.tolist()) == {8, 9} and int((lens == 9).sum()) == 2


def test_code_builder_limits_where_huffman_would_not():
    assert _plain_huffman_depth(BUILDER_HISTS["fibonacci-30"]) > 15
    assert _plain_huffman_depth(BUILDER_HISTS["six-million-zeros"]) <= 15
    lens = png.limited_code_lengths(BUILDER_HISTS["fibonacci-30"])
    assert int(lens.max()) == 15
    # one used byte value: EOB is the second symbol, one bit each
    lens = png.limited_code_lengths(BUILDER_HISTS["one-symbol-and-eob"])
    assert lens[77] == 1 and lens[256] == 1 and int((lens > 0).sum()) == 2
    # EOB is coded even where the histogram forgets it; EOB alone gets literal 0 for company
    lens = png.limited_code_lengths(_hist([(5, 10), (6, 1)], 0))
    assert lens[256] > 0
    lens = png.limited_code_lengths(_hist([], 4))
    assert lens[0] == 1 and lens[256] == 1
    with pytest.raises(ValueError):
        png.limited_code_lengths(np.zeros(256))
    with pytest.raises(ValueError):
        png.limited_code_lengths(_hist([(1, -1)], 1))


def test_canonical_codes_and_header_agree_with_the_statement():
    lens = png.limited_code_lengths(BUILDER_HISTS["fibonacci-30"])
    assert png.canonical_codes(lens).tolist() == R.canonical(lens)
    ent = png.code_entries(lens)
    for s in np.flatnonzero(lens):
        assert ent[s] & 15 == lens[s] and ent[s] >> 4 == R.rev(R.canonical(lens)[s], int(lens[s]))
    for final in (False, True):
        acc, n = png.block_header_bits(lens, final)
        seg = R.pack_segment(np.zeros(0, dtype=np.uint8), lens, final)
        whole = int.from_bytes(seg, "little")
        assert n == png.HEADER_BITS == 1106 and whole & ((1 << n) - 1) == acc


# ----------------------------------------------------------------------------- the statement against zlib and PIL
@pytest.mark.parametrize("index", range(len(R.CASES)), ids=R.CASE_IDS)
def test_statement_decodes_with_zlib_and_pil(index):
    case = R.CASES[index]
    frames = case.frames()
    for frame, enc in zip(frames, R.expected(index)):
        assert zlib.decompress(b"".join(enc.payloads)) == enc.stream
        assert np.array_equal(R.decode_with_pil(enc.file, case.order).reshape(frame.shape), frame)
        kinds = [k for k, _, _, _ in R.parse_chunks(enc.file)]
        assert kinds == [b"IHDR"] + [b"IDAT"] * len(enc.payloads) + [b"IEND"]
        for kind, body, crc, _ in R.parse_chunks(enc.file):
            assert zlib.crc32(kind + body) == crc


def test_matrix_reaches_every_filter_type_alignment_and_axis_value():
    chosen, ends, forced = set(), set(), set()
    for i, case in enumerate(R.CASES):
        for enc in R.expected(i):
            if case.filt == "adaptive":
                chosen.update(enc.types.tolist())
            else:
                forced.add(case.filt)
            ends.update((off + 12 + len(p)) % 4 for off, p in zip(enc.chunk_offsets, enc.payloads))
    assert chosen == {0, 1, 2, 3, 4}, "the adaptive cases must select every filter type at least once"
    assert forced == {0, 1, 2, 3, 4}
    assert 0 in ends and ends - {0}, "both dword-aligned and unaligned segment ends must occur"
    assert {c.w for c in R.CASES} >= set(R.WIDTHS) and {c.h for c in R.CASES} >= set(R.HEIGHTS)
    assert {c.c for c in R.CASES} == {1, 3} and {c.order for c in R.CASES} == {"bgr", "rgb"} and {c.n for c in R.CASES} >= {1, 3}
    assert {c.content for c in R.CASES} == set(R.CONTENTS) and {c.offset for c in R.CASES} == {0, 1, 2, 3}
    for h in R.HEIGHTS:
        assert {c.segment_rows for c in R.CASES if c.h == h} >= {1, 2, 16, h + 1}
    # the frame whose histogram forces length limiting does, and noise expands
    limit = R.CASE_IDS.index("limit-colour")
    enc = R.expected(limit)[0]
    hist = np.bincount(np.frombuffer(enc.stream, dtype=np.uint8), minlength=257)
    hist[256] = len(enc.payloads)
    assert _plain_huffman_depth(hist) > 15 and int(enc.lengths.max()) == 15
    noise = R.CASE_IDS.index("long-segment-noise")
    assert len(R.expected(noise)[0].file) > R.CASES[noise].frames()[0].size
    assert len(set(np.frombuffer(R.expected(noise)[0].stream, dtype=np.uint8).tolist())) == 256


# ----------------------------------------------------------------------------- Adler combine and the planner
def _stats_from_statement(encs, segment_rows, h, rowlen):
    """What phase 1 leaves: u32 [n, segments, 260] from the statement's filtered streams."""
    nseg = (h + segment_rows - 1) // segment_rows
    st = np.zeros((len(encs), nseg, png.STATS_STRIDE), dtype=np.uint32)
    for f, enc in enumerate(encs):
        stream = np.frombuffer(enc.stream, dtype=np.uint8).reshape(h, rowlen)
        for s in range(nseg):
            d = stream[s * segment_rows:(s + 1) * segment_rows].reshape(-1).astype(np.int64)
            st[f, s, :256] = np.bincount(d, minlength=256)
            st[f, s, 256] = d.sum() % 65521
            st[f, s, 257] = int(((d.size - np.arange(d.size)) * d).sum() % 65521)
            st[f, s, 258] = d.size
    return st


def test_adler_combine_against_zlib():
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, size=200_001, dtype=np.uint8)
    data[1000:90_000] = 255                      # sums far past 65521
    cuts = [0, 1, 2, 70_000, 70_001, 199_000, 200_001]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        d = data[a:b].astype(np.int64)
        parts.append((int(d.sum() % 65521), int(((d.size - np.arange(d.size)) * d).sum() % 65521), d.size))
    assert png.adler_combine(parts) == zlib.adler32(data.tobytes())
    assert png.adler_combine([]) == zlib.adler32(b"") == 1


@pytest.mark.parametrize("name", ["content-noise-fadaptive", "content-zeros-f0", "limit-colour", "shape-w1-h1", "shape-w257-h33",
                                  "long-segment-noise"])
def test_planner_against_the_statement(name):
    index = R.CASE_IDS.index(name)
    case, encs = R.CASES[index], R.expected(index)
    plan = png.plan_layout(_stats_from_statement(encs, case.segment_rows, case.h, case.w * case.c + 1))
    nseg = len(encs[0].payloads)
    for f, enc in enumerate(encs):
        assert int(plan.file_offsets[f + 1] - plan.file_offsets[f]) == len(enc.file)
        assert int(plan.adler[f]) == zlib.adler32(enc.stream) == struct.unpack(">I", enc.payloads[-1][-4:])[0]
        assert np.array_equal(plan.lengths[f], enc.lengths)
        for s in range(nseg):
            off, dl = plan.chunks[f * nseg + s]
            assert int(off - plan.file_offsets[f]) == enc.chunk_offsets[s] and int(dl) == len(enc.payloads[s])
        acc = sum(int(wd) << (32 * k) for k, wd in enumerate(plan.frame_tab[f, png.TAB_HEADER:png.TAB_HEADER + png.HEADER_WORDS]))
        assert acc == png.block_header_bits(enc.lengths)[0]
        assert int(plan.frame_tab[f, png.TAB_ADLER]) == int(plan.adler[f])
    assert png.FILE_HEAD == len(png.PNG_SIGNATURE + png.ihdr_chunk(case.w, case.h, case.c)) == encs[0].chunk_offsets[0]
    assert encs[0].file[:png.FILE_HEAD] == png.PNG_SIGNATURE + png.ihdr_chunk(case.w, case.h, case.c)
    with pytest.raises(ValueError):
        png.plan_layout(np.zeros((1, 2, 7), dtype=np.uint32))


# ----------------------------------------------------------------------------- mutants
def _decodes_to(data, frame, order):
    """True when PIL and zlib both accept `data` and PIL gives back `frame`."""
    try:
        idat = b"".join(body for kind, body, _, _ in R.parse_chunks(data) if kind == b"IDAT")
        zlib.decompress(idat)
        return np.array_equal(R.decode_with_pil(data, order).reshape(frame.shape), frame)
    except Exception:
        return False


MUTANT_CASES = {
    "paeth_tie": dict(filt=4, content="noise"),
    "average_round": dict(filt=3, content="noise"),
    "no_flush": dict(filt="adaptive", content="diag"),
    "bfinal_wrong": dict(filt="adaptive", content="diag"),
    "code_not_reversed": dict(filt="adaptive", content="diag"),
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_named_mutants_are_caught(mutant):
    spec = MUTANT_CASES[mutant]
    frame = R.make_content(spec["content"], 1, 33, 65, 3, 3)[0]
    good = R.encode(frame, "bgr", spec["filt"], 16)
    bad = R.encode(frame, "bgr", spec["filt"], 16, mutant=mutant)
    assert _decodes_to(good.file, frame, "bgr")
    assert bad.file != good.file
    assert not _decodes_to(bad.file, frame, "bgr"), f"the mutant {mutant} still decodes to the input"


# ----------------------------------------------------------------------------- arguments, without a GPU
def test_argument_checks_before_any_launch(built_lib):
    ok = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="resident"):
        png.encode_png_device(ok)                                            # not on the device
    with pytest.raises(ValueError, match="uint8"):
        png.encode_png_device(ok.float())
    with pytest.raises(ValueError, match="uint8"):
        png.encode_png_device(np.zeros((1, 4, 4, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="order"):
        png.encode_png_device(ok, order="gbr")
    for bad in ("none", 5, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="filter"):
            png.encode_png_device(ok, filter=bad)
    for bad in (0, -3, 1.5, None):
        with pytest.raises(ValueError, match="segment_rows"):
            png.encode_png_device(ok, segment_rows=bad)
    with pytest.raises(ValueError):
        png.encode_png_device(torch.zeros((4, 4), dtype=torch.uint8))
    # shape, contiguity and size are checked on a meta tensor's word alone: nothing here needs a device
    with pytest.raises(ValueError, match="paths|path"):
        png.save_frames([np.zeros((4, 4, 3), np.uint8)], [], "cuda:0")
    with pytest.raises(ValueError, match="uint8"):
        png.save_frames([np.zeros((4, 4, 3), np.float32)], ["a.png"], "cuda:0")
    with pytest.raises(ValueError, match="chunk_frames"):
        png.save_frames([np.zeros((4, 4, 3), np.uint8)], ["a.png"], "cuda:0", chunk_frames=0)
    with pytest.raises(RuntimeError):
        png.save_frames([np.zeros((4, 4, 3), np.uint8)], ["a.png"], "cpu")       # no CPU path
    # the C boundary
    h = png.lib()
    assert h.elvis_png_stats(16, 16, 16, 1, 4, 4, 2, 0, -1, 16, None) == -1 and b"channels" in h.elvis_last_error()
    assert h.elvis_png_stats(16, 16, 16, 1, 0, 4, 3, 0, -1, 16, None) == -1
    assert h.elvis_png_stats(16, 16, 16, 1, 4, 0, 3, 0, -1, 16, None) == -1
    assert h.elvis_png_stats(16, 16, 16, 1, 4, 4, 3, 2, -1, 16, None) == -1 and b"order" in h.elvis_last_error()
    assert h.elvis_png_stats(16, 16, 16, 1, 4, 4, 3, 0, 5, 16, None) == -1 and b"filter" in h.elvis_last_error()
    assert h.elvis_png_stats(16, 16, 16, 1, 4, 4, 3, 0, -1, 0, None) == -1 and b"segment_rows" in h.elvis_last_error()
    assert h.elvis_png_stats(16, 16, 16, 2, 32768, 10923, 3, 0, -1, 16, None) == -1 and b"2^31" in h.elvis_last_error()
    assert h.elvis_png_stats(None, 16, 16, 1, 4, 4, 3, 0, -1, 16, None) == -1 and b"null" in h.elvis_last_error()
    assert h.elvis_png_stats(None, None, None, 0, 4, 4, 3, 0, -1, 16, None) == 0                     # n = 0: nothing to do
    assert h.elvis_png_pack(16, 16, 16, 16, 16, 100, 1, 4, 4, 3, 0, 0, None) == -1
    assert h.elvis_png_pack(16, 16, 16, 16, 18, 100, 1, 4, 4, 3, 0, 16, None) == -1 and b"aligned" in h.elvis_last_error()
    assert h.elvis_png_pack(16, 16, None, 16, 16, 100, 1, 4, 4, 3, 0, 16, None) == -1
    assert "png.hip" in _build.SOURCES


# ----------------------------------------------------------------------------- the drivers' switch
def _plus_one(frames, maps, block_size, device, first_frame_index, **kw):
    return [f + 1 for f in frames]


def _write_dir(d, n=3, h=16, w=24):
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 200, size=(h, w, 3), dtype=np.uint8) for _ in range(n)]
    for i, f in enumerate(frames):
        frameio.save_frame(f, os.path.join(d, f"{i + 1:05d}.png"))
    return frames


def test_png_writer_switch_of_the_drivers(tmp_path):
    src = tmp_path / "src"
    frames = _write_dir(str(src))
    maps = np.ones((3, 2, 3), dtype=np.int32)
    calls = [
        lambda **k: drivers.restore_downsampled_with_sinsr(str(src), str(tmp_path / "o"), maps, 8, devices=["cpu"], _shard_fn=_plus_one, **k),
        lambda **k: drivers.restore_blur_adaptive(str(src), maps, 8, devices=["cpu"], _shard_fn=_plus_one, **k),
        lambda **k: drivers.restore_dct_adaptive(str(src), maps, 8, devices=["cpu"], _shard_fn=_plus_one, **k),
        lambda **k: drivers.stretch_shrunk_frames(str(src), str(tmp_path / "m.npz"), 8, devices=["cpu"], _shard_fn=_plus_one, **k),
        lambda **k: drivers.restore_shrunk_frames(str(src), str(tmp_path / "m.npz"), 8, str(tmp_path / "o2"), devices=["cpu"],
                                                  _shard_fn=_plus_one, **k),
    ]
    frameio.save_block_masks(np.zeros((3, 2, 3), dtype=np.uint8), str(tmp_path / "m.npz"))
    before = [open(src / f"{i + 1:05d}.png", "rb").read() for i in range(3)]
    for call in calls:
        with pytest.raises(ValueError, match="png_writer"):
            call(png_writer="x")
        with pytest.raises(RuntimeError):
            call(png_writer="device")                       # a CPU device: there is no CPU path
    assert before == [open(src / f"{i + 1:05d}.png", "rb").read() for i in range(3)], "a refused call must write nothing"
    # the default path writes what frameio.save_frame writes, byte for byte
    drivers.restore_downsampled_with_sinsr(str(src), str(tmp_path / "out"), maps, 8, devices=["cpu"], _shard_fn=_plus_one)
    drivers.restore_downsampled_with_sinsr(str(src), str(tmp_path / "out_pil"), maps, 8, devices=["cpu"], _shard_fn=_plus_one,
                                           png_writer="pil")
    for i, f in enumerate(frames):
        frameio.save_frame(f + 1, str(tmp_path / "want.png"))
        want = open(tmp_path / "want.png", "rb").read()
        assert open(tmp_path / "out" / f"{i + 1:05d}.png", "rb").read() == want
        assert open(tmp_path / "out_pil" / f"{i + 1:05d}.png", "rb").read() == want


def test_exports():
    import elvis_amd
    for name in ("encode_png_device", "save_frames_device", "save_frames"):
        assert getattr(elvis_amd, name) is getattr(png, name)
