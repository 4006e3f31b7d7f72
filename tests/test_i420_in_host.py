"""The decoder hand-off without a GPU: the inverse conversion's statement against its own mutants and against the forward
statement, the Y4M parser, the raw clip's size check, the clip-file driver's argument errors and the new C entry's
validation."""
import os
import re

import numpy as np
import pytest

import _handoff_ref as F
import _i420_in_ref as R
from elvis_amd import _lib, drivers, handoff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the statement
def test_constants_and_sums_fit_int32():
    """Black, white and the primaries of BT.601 studio swing come back; the extreme sums are the ones the header
    quotes and fit int32."""
    assert R.extreme_sums() == (560_969_128, -159_811_307)
    assert -2 ** 31 <= R.extreme_sums()[1] and R.extreme_sums()[0] < 2 ** 31

    def one(y, u, v):
        return R.i420_to_rgb(np.asarray([[[y, y], [y, y], [u, v]]], np.uint8))[0, 0, 0].tolist()

    assert one(16, 128, 128) == [0, 0, 0] and one(235, 128, 128) == [255, 255, 255]
    assert one(0, 128, 128) == [0, 0, 0] and one(255, 128, 128) == [255, 255, 255]
    # red by hand: G = (66 * 1220542 + (1 << 19) - 852492 * 112 + 409993 * 38) >> 20 = 1 180 690 >> 20 = 1
    assert one(82, 90, 240) == [255, 1, 0]
    for yuv, rgb in (((145, 54, 34), (0, 255, 0)), ((41, 240, 110), (0, 0, 255))):       # within the round trip's 2
        assert max(abs(a - b) for a, b in zip(one(*yuv), rgb)) <= 2
    bgr = R.i420_to_rgb(np.asarray([[[82, 82], [82, 82], [90, 240]]], np.uint8), "bgr")
    assert bgr[0, 0, 0].tolist() == [0, 1, 255]


def test_layout_and_replication():
    """A 4x2 frame by hand: the planes are Y, then U, then V, and both pixels rows of a quad take the quad's chroma."""
    planes = np.asarray([[[81, 82, 145, 146], [83, 84, 147, 148], [90, 54, 240, 34]]], np.uint8)
    out = R.i420_to_rgb(planes)
    assert out.shape == (1, 2, 4, 3)
    assert out[0, :, :2, 0].min() >= 250 and out[0, :, :2, 1:].max() <= 8          # the left quad is red
    assert out[0, :, 2:, 1].min() >= 250 and out[0, :, 2:, ::2].max() <= 8         # the right quad is green


def _bands(frame, band=256):
    """The exhaustive frame as frames of `band` rows: the same quads, a fraction of the memory."""
    side = frame.shape[2]
    y, u, v = frame[0, :side], frame[0, side:side * 5 // 4].reshape(side // 2, side // 2), frame[0, side * 5 // 4:].reshape(side // 2, side // 2)
    for at in range(0, side, band):
        part = np.concatenate([y[at:at + band].reshape(-1), u[at // 2:(at + band) // 2].reshape(-1), v[at // 2:(at + band) // 2].reshape(-1)])
        yield part.reshape(1, band * 3 // 2, side)


@pytest.mark.parametrize("name", sorted(set(R.MUTANTS) - {"truncation_toward_zero"}))
def test_every_mutant_is_told_apart(name):
    """Each mutant changes one clause and gives other bytes than the statement on the exhaustive frame - read in bands of
    256 rows until the first band that differs."""
    for part in _bands(R.every_yuv_frame()):
        if not np.array_equal(R.i420_to_rgb(part, **R.MUTANTS[name]), R.i420_to_rgb(part)):
            return
    raise AssertionError(f"{name} equals the statement on every (Y, U, V)")


def test_truncation_mutant_changes_the_sum_but_no_byte():
    """Truncation toward zero in place of the floor shift is a real change of the clause - the values before sat8 differ
    wherever a sum is negative and no multiple of 2^20 - but it can change no byte: it differs from the floor by exactly
    one, only below zero, and sat8 sends both to 0.  So the bytes cannot pin this clause; what the device test pins is
    that negative sums come out as 0 (about a fifth of the exhaustive frame's outputs)."""
    part = next(_bands(R.every_yuv_frame()))
    y, u, v = R._planes(part)
    u, v = (np.repeat(np.repeat(p, 2, 1), 2, 2) for p in (u, v))
    floor = R.rgb_of(y, u, v, saturate=False)
    trunc = R.rgb_of(y, u, v, saturate=False, **R.MUTANTS["truncation_toward_zero"])
    for a, b in zip(floor, trunc):
        d = b - a
        assert d.max() == 1 and d.min() == 0 and (a[d == 1] < 0).all() and (b[d == 1] <= 0).all()
    assert np.array_equal(R.i420_to_rgb(part, **R.MUTANTS["truncation_toward_zero"]), R.i420_to_rgb(part))
    assert len(R.MUTANTS) == 5


def test_exhaustive_frame_holds_every_triple_once():
    frame = R.every_yuv_frame()
    y, u, v = R._planes(frame)
    code = (y[0] << 16) | (np.repeat(np.repeat(u[0], 2, 0), 2, 1) << 8) | np.repeat(np.repeat(v[0], 2, 0), 2, 1)
    assert np.array_equal(np.sort(code.reshape(-1)), np.arange(1 << 24))


def test_forward_then_inverse_stays_within_two():
    """tests/_handoff_ref.py's forward statement, then the inverse, on quad-constant colour: every channel of every one
    of the 2^24 colours comes back within 2."""
    counts = np.zeros(8, np.int64)
    for r in range(0, 256, 32):
        c = np.arange(r << 16, (r + 32) << 16, dtype=np.int32)
        rgb = np.stack([c >> 16, (c >> 8) & 255, c & 255], axis=-1)                   # [2^21, 3]
        # a quad of one colour has that colour's Y four times and its U, V once: element by element is the whole frame
        back = np.stack(R.rgb_of(*F.yuv_of(rgb)), axis=-1)
        err = np.abs(back - rgb).max(axis=-1)
        assert err.max() < 8
        counts += np.bincount(err, minlength=8)
    assert counts.tolist() == [2_657_757, 14_036_315, 83_144, 0, 0, 0, 0, 0]
    # and through both layouts: a frame of quad-constant colour
    colours = np.random.default_rng(3).integers(0, 256, (2, 3, 5, 3), dtype=np.uint8)
    quads = np.repeat(np.repeat(colours, 2, axis=1), 2, axis=2)
    back = R.i420_to_rgb(F.rgb_to_i420(quads))
    assert np.array_equal(back, np.repeat(np.repeat(back[:, ::2, ::2], 2, axis=1), 2, axis=2))
    assert np.array_equal(back[:, ::2, ::2], np.stack(R.rgb_of(*F.yuv_of(colours)), axis=-1))
    assert np.abs(back.astype(int) - quads).max() <= 2
    mirrored = np.ascontiguousarray(quads[..., ::-1])
    assert np.array_equal(R.i420_to_rgb(F.rgb_to_i420(mirrored, "bgr"), "bgr"), back[..., ::-1])


# ----------------------------------------------------------------------------- parse_y4m
W, H, FB = 6, 4, 36


def _payloads(n, seed=0):
    return [np.random.default_rng(seed + i).integers(0, 256, FB, dtype=np.uint8).tobytes() for i in range(n)]


def _write(tmp_path, data, name="clip.y4m"):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def test_parse_file_from_y4m_header(tmp_path):
    data = handoff.y4m_header(W, H, 29.97) + b"".join(b"FRAME\n" + p for p in _payloads(3))
    info = handoff.parse_y4m(_write(tmp_path, data))
    assert isinstance(info, handoff.Y4MInfo)
    assert (info.width, info.height, info.fps_num, info.fps_den) == (W, H, 29970, 1000)
    assert (info.interlace, info.aspect, info.colourspace, info.frame_count) == ("p", "1:1", "420", 3)
    assert list(info.frame_offsets) == R.y4m_walk(data)[2] and info.frame_bytes == FB and info.framerate == 29.97
    empty = handoff.parse_y4m(_write(tmp_path, handoff.y4m_header(W, H, 30), "empty.y4m"))
    assert empty.frame_count == 0 and empty.frame_offsets == ()


def test_parse_tokens_reordered_and_unknown_ignored(tmp_path):
    data = b"YUV4MPEG2 XYSCSS=420JPEG C420jpeg A128:117 I? F24000:1001 H4 XCOLORRANGE=LIMITED W6\n" + b"".join(b"FRAME\n" + p for p in _payloads(2))
    info = handoff.parse_y4m(_write(tmp_path, data))
    assert (info.width, info.height, info.fps_num, info.fps_den, info.interlace, info.aspect, info.colourspace) == \
        (6, 4, 24000, 1001, "?", "128:117", "420jpeg")
    assert list(info.frame_offsets) == R.y4m_walk(data)[2] and info.frame_count == 2


def test_parse_frame_lines_with_parameters(tmp_path):
    lines = [b"FRAME Ip\n", b"FRAME\n", b"FRAME Ixyz XFOO=1\n"]
    data = b"YUV4MPEG2 W6 H4 F30:1\n" + b"".join(line + p for line, p in zip(lines, _payloads(3)))
    info = handoff.parse_y4m(_write(tmp_path, data))
    assert list(info.frame_offsets) == R.y4m_walk(data)[2] and info.frame_count == 3
    assert info.frame_offsets[1] - info.frame_offsets[0] == FB + 6 and info.frame_offsets[0] == 22 + 9


@pytest.mark.parametrize("token", ["C420", "C420jpeg", "C420mpeg2", "C420paldv", None])
def test_parse_accepted_colourspaces(tmp_path, token):
    head = b"YUV4MPEG2 W6 H4 F25:1" + (b" " + token.encode() if token else b"") + b"\n"
    data = head + b"FRAME\n" + _payloads(1)[0]
    info = handoff.parse_y4m(_write(tmp_path, data))
    assert info.colourspace == (token[1:] if token else "420") and info.interlace == "?" and info.aspect == "0:0"
    assert list(info.frame_offsets) == [len(head) + 6]


def test_parse_never_reads_a_payload_byte(tmp_path, monkeypatch):
    """Every read of the walk lies inside the header or a FRAME line."""
    import builtins
    lines = [b"FRAME\n", b"FRAME Ip\n", b"FRAME\n"]
    head = b"YUV4MPEG2 W6 H4 F30:1\n"
    data = head + b"".join(line + p for line, p in zip(lines, _payloads(3)))
    path = _write(tmp_path, data)
    allowed, pos = set(range(len(head))), len(head)
    for line in lines:
        allowed |= set(range(pos, pos + len(line)))
        pos += len(line) + FB
    touched = set()
    real_open = builtins.open

    class Spy:
        def __init__(self, f):
            self.f = f

        def read(self, k=-1):
            at = self.f.tell()
            got = self.f.read(k)
            touched.update(range(at, at + len(got)))
            return got

        def __getattr__(self, name):
            return getattr(self.f, name)

        def __enter__(self):
            return self

        def __exit__(self, *a):
            self.f.close()

    monkeypatch.setattr(builtins, "open", lambda *a, **k: Spy(real_open(*a, **k)))
    info = handoff.parse_y4m(path)
    monkeypatch.undo()
    assert info.frame_count == 3 and touched and touched <= allowed


@pytest.mark.parametrize("head,word", [
    (b"YUV4MPEG3 W6 H4 F30:1\n", "YUV4MPEG2"), (b"RIFF W6 H4\n", "YUV4MPEG2"),
    (b"YUV4MPEG2 H4 F30:1\n", "width"), (b"YUV4MPEG2 W6 F30:1\n", "height"), (b"YUV4MPEG2 W0 H4\n", "width"),
    (b"YUV4MPEG2 W6 H-4\n", "height"), (b"YUV4MPEG2 Wsix H4\n", "width"),
    (b"YUV4MPEG2 W7 H4\n", "width"), (b"YUV4MPEG2 W6 H5\n", "height"),
    (b"YUV4MPEG2 W6 H4 C422\n", "C422"), (b"YUV4MPEG2 W6 H4 C444\n", "C444"), (b"YUV4MPEG2 W6 H4 Cmono\n", "Cmono"),
    (b"YUV4MPEG2 W6 H4 C420p10\n", "C420p10"), (b"YUV4MPEG2 W6 H4 C444alpha\n", "C444alpha"),
    (b"YUV4MPEG2 W6 H4 It\n", "It"), (b"YUV4MPEG2 W6 H4 Ib\n", "Ib"), (b"YUV4MPEG2 W6 H4 Im\n", "Im"),
])
def test_parse_refuses(tmp_path, head, word):
    path = _write(tmp_path, head + b"FRAME\n" + _payloads(1)[0], "bad.y4m")
    with pytest.raises(ValueError) as e:
        handoff.parse_y4m(path)
    assert "bad.y4m" in str(e.value) and word in str(e.value)


def test_parse_truncated_and_displaced(tmp_path):
    head = handoff.y4m_header(W, H, 30)
    p = _payloads(3)
    cut = head + b"FRAME\n" + p[0] + b"FRAME\n" + p[1] + b"FRAME\n" + p[2][:-1]
    with pytest.raises(IOError) as e:
        handoff.parse_y4m(_write(tmp_path, cut, "cut.y4m"))
    assert not isinstance(e.value, ValueError) and "cut.y4m" in str(e.value) and "frame 2" in str(e.value)
    moved = head + b"FRAME\n" + p[0] + b"\x00FRAME\n" + p[1]
    with pytest.raises(IOError) as e:
        handoff.parse_y4m(_write(tmp_path, moved, "moved.y4m"))
    assert "moved.y4m" in str(e.value) and "frame 1" in str(e.value)
    short = head + b"FRAME\n" + p[0] + b"FRA"
    with pytest.raises(IOError) as e:
        handoff.parse_y4m(_write(tmp_path, short, "short.y4m"))
    assert "frame 1" in str(e.value)


# ----------------------------------------------------------------------------- raw clips and the driver, before any device use
def test_load_yuv420p_size_check(tmp_path):
    raw = b"".join(_payloads(3))
    path = _write(tmp_path, raw, "clip.yuv")
    assert handoff.yuv420p_frame_count(len(raw), W, H) == 3
    for source in (raw[:-1], _write(tmp_path, raw + b"\x00", "long.yuv")):
        with pytest.raises(ValueError, match="whole number"):
            handoff.load_yuv420p_device(source, W, H, "cpu")
    with pytest.raises(ValueError, match="whole number"):
        handoff.load_yuv420p_device(path, W + 2, H, "cpu")                          # the usual cause: a wrong width
    for w, h in ((5, 4), (6, 3), (0, 4), (6, -4)):
        with pytest.raises(ValueError, match="even"):
            handoff.load_yuv420p_device(raw, w, h, "cpu")
    with pytest.raises(ValueError, match="within"):
        handoff.load_yuv420p_device(raw, W, H, "cpu", start=2, count=2)
    with pytest.raises(ValueError, match="order"):
        handoff.load_yuv420p_device(raw, W, H, "cpu", "yuv")
    with pytest.raises(RuntimeError, match="MI355X only"):                              # the checks pass: the device is asked for
        handoff.load_yuv420p_device(raw, W, H, "cpu")


def test_restore_yuv_clip_argument_errors(tmp_path, monkeypatch):
    """Every argument error is raised before a device is asked for."""
    def no_device(*a, **k):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(drivers, "resolve_device_list", no_device)
    y4m = _write(tmp_path, handoff.y4m_header(W, H, 30) + b"".join(b"FRAME\n" + p for p in _payloads(3)), "in.y4m")
    norate = _write(tmp_path, b"YUV4MPEG2 W6 H4\n" + b"".join(b"FRAME\n" + p for p in _payloads(3)), "norate.y4m")
    raw = _write(tmp_path, b"".join(_payloads(3)), "in.yuv")
    out, maps = str(tmp_path / "out.y4m"), np.ones((3, 2, 3), np.int32)
    cases = [
        (dict(kind="vsr"), "kind"),
        (dict(input_path=str(tmp_path / "in.mp4")), "input_path"),
        (dict(output_path=str(tmp_path / "out.png")), "output_path"),
        (dict(output_path=y4m), "different files"),
        (dict(output_path=os.path.join(str(tmp_path), ".", "in.y4m")), "different files"),
        (dict(input_path=raw), "width="),
        (dict(input_path=raw, width=W), "width="),
        (dict(input_path=raw, width=W + 2, height=H), "whole number"),
        (dict(input_path=raw, width=W, height=H), "framerate="),
        (dict(input_path=norate), "framerate="),
        (dict(width=8), "width=8"),
        (dict(maps=maps[:2]), r"blur_maps length \(2\) does not match frame count \(3\)\."),
        (dict(kind="sinsr", maps=maps[0]), r"Downscale maps length \(2\) does not match frame count \(3\)\."),
        (dict(kind="dct", maps=np.ones((4, 2, 3))), r"strength_maps length \(4\) does not match frame count \(3\)\."),
        (dict(batch_size=0), "batch_size"),
        (dict(input_path=_write(tmp_path, handoff.y4m_header(W, H, 30), "empty.y4m"), maps=maps[:0]), "No frames found"),
    ]
    for change, message in cases:
        args = dict(kind="blur", input_path=y4m, output_path=out, maps=maps, block_size=2)
        args.update(change)
        kind, inp, outp, m, b = (args.pop(k) for k in ("kind", "input_path", "output_path", "maps", "block_size"))
        with pytest.raises(ValueError, match=message):
            drivers.restore_yuv_clip(kind, inp, outp, m, b, **args)
        assert not os.path.exists(out), change
    assert open(y4m, "rb").read().startswith(b"YUV4MPEG2")                              # the input was never opened for writing
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="GPU"):
        drivers.restore_yuv_clip("blur", y4m, out, maps, 2, devices=["cpu"])
    assert not os.path.exists(out)


# ----------------------------------------------------------------------------- the ABI and the exports
def test_abi_symbol_and_validation_without_gpu(built_lib):
    import elvis_amd
    from elvis_amd import _build
    assert "i420_in.hip" in _build.SOURCES
    header = open(os.path.join(ROOT, "include", "elvis_amd.h")).read()
    m = re.search(r"int\s+elvis_i420_to_rgb_u8\s*\(([^;]*)\)\s*;", header)
    assert m and len(m.group(1).split(",")) == 7 == len(_lib.SIGNATURES["elvis_i420_to_rgb_u8"])
    h = _lib.lib()
    # argument checks come before any launch, so they can be exercised without a device
    assert h.elvis_i420_to_rgb_u8(16, 16, 1, 3, 4, 0, None) == -1 and b"even" in h.elvis_last_error()
    assert h.elvis_last_error().startswith(b"elvis_i420_to_rgb_u8")
    assert h.elvis_i420_to_rgb_u8(16, 16, 1, 4, 6 + 1, 0, None) == -1 and b"even" in h.elvis_last_error()
    assert h.elvis_i420_to_rgb_u8(16, 16, -1, 4, 4, 0, None) == -1 and b"bad shape" in h.elvis_last_error()
    assert h.elvis_i420_to_rgb_u8(None, 16, 1, 4, 4, 0, None) == -1 and b"null" in h.elvis_last_error()
    assert h.elvis_i420_to_rgb_u8(16, None, 1, 4, 4, 1, None) == -1 and b"null" in h.elvis_last_error()
    assert h.elvis_i420_to_rgb_u8(16, 16, 1 << 30, 1 << 30, 16, 0, None) == -1 and b"more than one launch holds" in h.elvis_last_error()
    assert h.elvis_i420_to_rgb_u8(None, None, 0, 4, 4, 0, None) == 0
    assert h.elvis_i420_to_rgb_u8(None, None, 3, 0, 4, 0, None) == 0 and h.elvis_i420_to_rgb_u8(None, None, 3, 4, 0, 1, None) == 0
    for name in ("i420_to_rgb_device", "parse_y4m", "Y4MInfo", "load_y4m_device", "load_yuv420p_device", "read_y4m"):
        assert getattr(elvis_amd, name) is getattr(handoff, name)
    assert elvis_amd.restore_yuv_clip is drivers.restore_yuv_clip
    from elvis_amd import restore
    for name in ("restore_frames_sinsr_device", "restore_frames_blur_device", "restore_frames_dct_device"):
        assert getattr(elvis_amd, name) is getattr(restore, name)
