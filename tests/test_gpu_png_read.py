"""The PNG reader on the device (csrc/png_read.hip, csrc/inflate.h, elvis_amd/png.py) against zlib, PIL and its statement
(tests/_png_read_ref.py): the inflater alone on every stream of the corpus, the whole decode on every file, the round trip
through the device writer, guard bytes around the work buffers, uploads 1..3 bytes off a dword, every malformed case in
a batch with good frames, independence of batch and chunk size, and the v1 directory drivers with both readers."""
import os
import zlib

import numpy as np
import pytest
import torch

import _png_read_ref as R
import elvis_amd
from elvis_amd import drivers, frameio, png

pytestmark = pytest.mark.gpu
GUARD = 64


def _guards_intact(buf: torch.Tensor, payload: int) -> bool:
    host = buf.cpu().numpy()
    return bool((host[:GUARD] == 0xA5).all() and (host[GUARD + payload:] == 0xA5).all()) and host.size == payload + 2 * GUARD


def _check_inflated(cases, buf, out_off, status):
    host = buf.cpu().numpy()[GUARD:]
    for i, sc in enumerate(cases):
        want = R.inflated(sc.name)
        code, produced, consumed, adler = (int(v) for v in status[i])
        assert code == want.status, (sc.name, code, want.status)
        assert produced == len(want.out) and adler == want.adler and consumed == want.consumed, sc.name
        assert host[int(out_off[i]):int(out_off[i]) + produced].tobytes() == want.out, sc.name
        if want.status == R.OK:
            assert want.out == zlib.decompress(sc.stream), sc.name


def test_inflate_every_stream_equals_zlib(gpu_device):
    cases = R.good_streams()
    buf, out_off, status = png._inflate_clip([c.stream for c in cases], [c.cap for c in cases], gpu_device, guard=GUARD)
    _check_inflated(cases, buf, out_off, status)
    assert _guards_intact(buf, max(int(out_off[-1]), 4))
    outs = png.inflate_device([c.stream for c in cases[:5]], [c.cap for c in cases[:5]], gpu_device)
    assert outs == [zlib.decompress(c.stream) for c in cases[:5]]
    assert png.inflate_device([], [], gpu_device) == []


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_inflate_uploads_off_a_dword(gpu_device, offset):
    cases = [c for c in R.good_streams() if c.name.startswith(("stream-", "cut-", "handbuilt", "stored-long"))]
    buf, out_off, status = png._inflate_clip([c.stream for c in cases], [c.cap for c in cases], gpu_device, guard=GUARD, upload_offset=offset)
    _check_inflated(cases, buf, out_off, status)
    assert _guards_intact(buf, max(int(out_off[-1]), 4))


def test_inflate_malformed_streams_give_the_statements_status(gpu_device):
    """Every malformed stream passed tools/png_inflate_check.cpp on the host before it came here."""
    good = [c for c in R.good_streams() if c.name.startswith("cut-")]
    cases = list(good[:2]) + list(R.malformed_streams()) + list(good[2:4])
    buf, out_off, status = png._inflate_clip([c.stream for c in cases], [c.cap for c in cases], gpu_device, guard=GUARD)
    _check_inflated(cases, buf, out_off, status)
    assert _guards_intact(buf, max(int(out_off[-1]), 4))
    with pytest.raises(IOError, match="stream 1: Adler-32 mismatch"):
        bad = next(c for c in R.malformed_streams() if c.name == "adler-flipped")
        png.inflate_device([good[0].stream, bad.stream], [good[0].cap, bad.cap], gpu_device)


def test_gather_concatenates_the_idat_payloads(gpu_device):
    """png_gather_kernel's only output, the zlib streams, through elvis_png_gather itself: every IDAT chunk's data land
    where the chunk table says, in file order; files of one and of many IDAT chunks, uploaded 0..3 bytes past a dword."""
    from elvis_amd._lib import check, lib, ptr, stream_handle
    cases = [fc for fc in R.files() if (fc.h, fc.w) in ((17, 63), (33, 65))]
    infos = [png.parse_png(fc.data, fc.name) for fc in cases]
    assert {sum(1 for c in i.chunks if c[2]) for i in infos} >= {1, 2} and max(sum(1 for c in i.chunks if c[2]) for i in infos) >= 3
    file_off = np.concatenate([[0], np.cumsum([len(fc.data) for fc in cases])])
    rows, want = [], b""
    for f, (fc, info) in enumerate(zip(cases, infos)):
        for off, length, idat in info.chunks:
            rows.append((int(file_off[f]) + off, length, len(want) if idat else -1))
            if idat:
                want += fc.data[off + 4:off + 4 + length]
    for upload_offset in range(4):
        host = np.concatenate([np.zeros(upload_offset, np.uint8)] + [np.frombuffer(fc.data, np.uint8) for fc in cases])
        files_d = torch.from_numpy(host).to(gpu_device)[upload_offset:]
        chunks_d = torch.from_numpy(np.asarray(rows, np.int64).reshape(-1)).to(gpu_device)
        buf = torch.full((len(want) + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=gpu_device)
        status_d = torch.full((len(rows),), 7, dtype=torch.int32, device=gpu_device)
        check(lib().elvis_png_gather(ptr(files_d), int(file_off[-1]), ptr(chunks_d), len(rows), ptr(buf) + GUARD, len(want), ptr(status_d),
                                     stream_handle(gpu_device)), gpu_device)
        assert buf.cpu().numpy()[GUARD:GUARD + len(want)].tobytes() == want, upload_offset
        assert _guards_intact(buf, len(want)) and not status_d.cpu().numpy().any()              # and every chunk's CRC holds


def _groups(only_gray=False):
    """The files of the corpus by size: one call decodes files of one size, of any colour type."""
    groups = {}
    for fc in R.files():
        if not only_gray or fc.c == 1:
            groups.setdefault((fc.h, fc.w), []).append(fc)
    return groups


@pytest.mark.parametrize("order", ["bgr", "rgb"])
def test_decode_every_file_equals_pil(gpu_device, order):
    for (h, w), group in _groups().items():
        frames, buf, filt_buf, codes = png._decode_clip([fc.data for fc in group], gpu_device, order, 3, guard=GUARD)
        assert codes == [0] * len(group), [(fc.name, c) for fc, c in zip(group, codes) if c]
        host = frames.cpu().numpy()
        assert host.shape == (len(group), h, w, 3)
        for i, fc in enumerate(group):
            assert np.array_equal(host[i], R.decode_with_pil(fc.data, order)), fc.name
        assert _guards_intact(buf, host.size), (h, w)
        assert _guards_intact(filt_buf, filt_buf.numel() - 2 * GUARD), (h, w)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_decode_uploads_off_a_dword(gpu_device, offset):
    """The file bytes start 1..3 bytes past a dword: the gather's and the CRC check's reads, every cut and colour type."""
    group = [fc for fc in R.files() if (fc.h, fc.w) == (17, 63)] + [fc for fc in R.files() if (fc.h, fc.w) == (33, 65)][:6]
    for size in ((17, 63), (33, 65)):
        files = [fc for fc in group if (fc.h, fc.w) == size]
        frames, buf, filt_buf, codes = png._decode_clip([fc.data for fc in files], gpu_device, "bgr", 3, guard=GUARD, upload_offset=offset)
        assert codes == [0] * len(files), [(fc.name, c) for fc, c in zip(files, codes) if c]
        host = frames.cpu().numpy()
        for i, fc in enumerate(files):
            assert np.array_equal(host[i], R.decode_with_pil(fc.data)), fc.name
        assert _guards_intact(buf, host.size) and _guards_intact(filt_buf, filt_buf.numel() - 2 * GUARD)
    bad = next(b for b in R.malformed_files() if b.name == "crc-off-by-one")
    good = _companion(9, 11, 3, 90 + offset)
    frames, _, _, codes = png._decode_clip([good, bad.data], gpu_device, "bgr", 3, upload_offset=offset)
    assert codes == [0, R.E_CRC] and np.array_equal(frames[0].cpu().numpy(), R.decode_with_pil(good))


def test_decode_gray_files_to_one_channel(gpu_device):
    for (h, w), group in _groups(only_gray=True).items():
        frames = png.decode_png_device([fc.data for fc in group], gpu_device, channels=1)
        assert frames.shape == (len(group), h, w, 1) and frames.is_contiguous() and frames.dtype == torch.uint8
        host = frames.cpu().numpy()
        for i, fc in enumerate(group):
            assert np.array_equal(host[i], R.decode_with_pil(fc.data, "bgr", 1)), fc.name


def test_round_trip_through_the_device_writer(gpu_device):
    for c, kind in ((3, "diag"), (3, "noise"), (1, "hot")):
        clip = R.make_content(kind, 3, 65, 129, c, 11)
        d = torch.from_numpy(clip).to(gpu_device)
        for order in ("bgr", "rgb"):
            files = png.encode_png_device(d, order)
            back = png.decode_png_device(files, gpu_device, order, channels=c)
            assert torch.equal(back, d), (c, kind, order)


def _companion(h, w, c, seed):
    return R.make_file(w, h, c, "diag", 4, "l6", "one", seed)


def test_malformed_files_in_a_batch_with_good_frames(gpu_device, tmp_path):
    for k, bf in enumerate(b for b in R.malformed_files() if b.status):
        info = png.parse_png(bf.data)
        first, last = _companion(info.height, info.width, info.bpp, 2 * k), _companion(info.height, info.width, info.bpp, 2 * k + 1)
        frames, buf, filt_buf, codes = png._decode_clip([first, bf.data, last], gpu_device, "bgr", 3, guard=GUARD)
        assert codes == [0, bf.status, 0], (bf.name, codes)
        host = frames.cpu().numpy()
        assert np.array_equal(host[0], R.decode_with_pil(first)) and np.array_equal(host[2], R.decode_with_pil(last)), bf.name
        assert _guards_intact(buf, host.size) and _guards_intact(filt_buf, filt_buf.numel() - 2 * GUARD), bf.name
        paths = [tmp_path / f"{k}-{i}.png" for i in range(3)]
        for p, data in zip(paths, (first, bf.data, last)):
            p.write_bytes(data)
        with pytest.raises(IOError, match=f"Failed to load frame: .*{k}-1.png"):
            png.load_frames_device(paths, gpu_device)
    for bf in R.malformed_files():
        if not bf.status:
            with pytest.raises(bf.error):
                png.decode_png_device([bf.data], gpu_device)


def test_same_bytes_alone_in_a_batch_and_at_any_chunk_size(gpu_device, tmp_path):
    datas = [R.make_file(65, 33, c, kind, filt, how, cut, 40 + i)
             for i, (c, kind, filt, how, cut) in enumerate(((3, "diag", "mix", "l6", 7), (4, "noise", 4, "huffman", "one"), (1, "hot", 3, "fixed", "empty-middle")))]
    batch = png.decode_png_device(datas, gpu_device)
    for i, data in enumerate(datas):
        assert torch.equal(png.decode_png_device([data], gpu_device)[0], batch[i]), "a frame decodes to other bytes alone"
        assert np.array_equal(batch[i].cpu().numpy(), R.decode_with_pil(data))
    paths = [tmp_path / f"{i}.png" for i in range(3)]
    for p, data in zip(paths, datas):
        p.write_bytes(data)
    for chunk in (1, 2, None):
        got = png.load_frames_device(paths, str(gpu_device), chunk_frames=chunk)
        assert got.is_contiguous() and torch.equal(got, batch), chunk
    for i, p in enumerate(paths):
        assert np.array_equal(frameio.load_frame(p), batch[i].cpu().numpy())


def _v1_directory(tmp_path, n=3, by=4, bx=6, b=8, k=2, seed=21):
    """A 3-frame 32x48 clip as the v1 client side receives it: shrunk frames 00001.png ... and the packed masks."""
    rng = np.random.default_rng(seed)
    masks = np.zeros((n, by, bx), np.uint8)
    for i in range(n):
        for r in range(by):
            masks[i, r, rng.choice(bx, k, replace=False)] = 1
    d = tmp_path / "frames"
    for i in range(n):
        frameio.save_frame(rng.integers(0, 256, size=(by * b, (bx - k) * b, 3), dtype=np.uint8), d / f"{i + 1:05d}.png")
    frameio.save_block_masks(masks, tmp_path / "masks.npz")
    return str(d), str(tmp_path / "masks.npz"), b, [f"{i + 1:05d}.png" for i in range(n)]


def _same_pixels(dir_a, dir_b, names):
    for name in names:
        assert np.array_equal(frameio.load_frame(os.path.join(dir_a, name)), frameio.load_frame(os.path.join(dir_b, name))), (dir_b, name)


def test_v1_drivers_with_both_readers(gpu_device, tmp_path):
    frames_dir, npz, b, names = _v1_directory(tmp_path)
    dirs = {}
    for reader, writer in (("pil", "pil"), ("device", "pil"), ("device", "device")):
        root = tmp_path / f"{reader}-{writer}"
        p = dirs[(reader, writer)] = {k: str(root / k) for k in ("stretch_out", "out", "stretched", "full")}
        drivers.stretch_shrunk_frames(frames_dir, npz, b, out_dir=p["stretch_out"], devices=[gpu_device], png_reader=reader, png_writer=writer)
        drivers.restore_shrunk_frames(frames_dir, npz, b, p["out"], stretched_dir=p["stretched"], fullres_masks_dir=p["full"],
                                      devices=[gpu_device], png_reader=reader, png_writer=writer)
        for k in p:
            assert sorted(os.listdir(p[k])) == names, (reader, writer, k)
    for key in (("device", "pil"), ("device", "device")):
        for k in ("stretch_out", "out", "stretched", "full"):
            _same_pixels(dirs[("pil", "pil")][k], dirs[key][k], names)
    assert frameio.load_frame(os.path.join(dirs[("device", "device")]["out"], names[0])).shape == (32, 48, 3)
    with pytest.raises(ValueError, match="png_reader"):
        drivers.restore_shrunk_frames(frames_dir, npz, b, str(tmp_path / "x"), devices=[gpu_device], png_reader="gpu")


def test_v1_shard_pixels_never_visit_the_host(gpu_device, tmp_path, monkeypatch):
    """With reader and writer on the device a v1 shard neither downloads a clip (`frames_to_host`) nor uploads frames
    (`save_frames`, `frames_to_device` of host arrays): only files go up and finished files come down."""
    from elvis_amd import recompose
    frames_dir, npz, b, names = _v1_directory(tmp_path)
    want = {k: str(tmp_path / "want" / k) for k in ("stretch_out", "out", "stretched")}
    drivers.stretch_shrunk_frames(frames_dir, npz, b, out_dir=want["stretch_out"], devices=[gpu_device])
    drivers.restore_shrunk_frames(frames_dir, npz, b, want["out"], stretched_dir=want["stretched"], devices=[gpu_device])

    def refuse(*args, **kw):
        raise AssertionError("pixels went through the host")

    real_to_device = recompose.frames_to_device
    monkeypatch.setattr(recompose, "frames_to_host", refuse)
    monkeypatch.setattr(png, "save_frames", refuse)
    monkeypatch.setattr(recompose, "frames_to_device", lambda frames, device: real_to_device(frames, device) if isinstance(frames, torch.Tensor) else refuse())
    got = {k: str(tmp_path / "got" / k) for k in want}
    drivers.stretch_shrunk_frames(frames_dir, npz, b, out_dir=got["stretch_out"], devices=[gpu_device], png_reader="device", png_writer="device")
    drivers.restore_shrunk_frames(frames_dir, npz, b, got["out"], stretched_dir=got["stretched"], devices=[gpu_device],
                                  png_reader="device", png_writer="device")
    monkeypatch.undo()
    for k in want:
        _same_pixels(want[k], got[k], names)


def test_resident_clip_passes_through_frames_to_device(gpu_device, tmp_path):
    from elvis_amd.recompose import frames_to_device
    frames_dir, _, _, names = _v1_directory(tmp_path)
    clip = png.load_frames_device([os.path.join(frames_dir, n) for n in names], gpu_device)
    assert frames_to_device(clip, gpu_device) is clip
    with pytest.raises(ValueError, match="resident clip"):
        frames_to_device(clip[:, :, ::2], gpu_device)


def test_exported(gpu_device):
    fc = R.files()[0]
    assert np.array_equal(elvis_amd.decode_png_device([fc.data], gpu_device)[0].cpu().numpy(), R.decode_with_pil(fc.data))
