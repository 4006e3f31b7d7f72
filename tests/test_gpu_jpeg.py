"""The JPEG reader on the device (csrc/jpeg_read.hip, csrc/jpeg_decode.h, elvis_amd/jpeg.py) against its statement
(tests/_jpeg_ref.py) and PIL on libjpeg-turbo, bit for bit: every file of the corpus in both orders with the entropy
kernel's coefficients and status words per segment, guard bytes around the work buffers, uploads 1..3 bytes off a dword,
segment counts around the width of a wave, one long serial segment, every malformed stream in a batch with good frames,
independence of batch and chunk size, mixed PNG + JPEG lists, and the directory drivers with both readers."""
import os

import numpy as np
import pytest
import torch

import _jpeg_ref as R
import elvis_amd
from elvis_amd import drivers, frameio, jpeg, png

pytestmark = pytest.mark.gpu
GUARD = 64
# streams of the statement's writer that libjpeg itself refuses: a code of all 1 bits
NOT_FOR_PIL = ("ff00-first-and-last",)


def _guards_intact(buf: torch.Tensor) -> bool:
    host = buf.cpu().numpy()
    return bool((host[:GUARD] == 0xA5).all() and (host[-GUARD:] == 0xA5).all())


def _check_clip(cases, got, order="rgb", channels=3, pil=True):
    """Pixels, per-segment status words, coefficients and guard bytes of one decoded clip against the statement."""
    host = got["frames"].cpu().numpy()
    plan = got["plan"]
    coef = got["coef_buf"].cpu().numpy()[GUARD:-GUARD].view(np.int16).reshape(len(cases), plan.stride_blocks, 64)
    planes = got["plane_buf"].cpu().numpy()[GUARD:-GUARD].reshape(len(cases), plan.stride_blocks * 64)
    for i, fc in enumerate(cases):
        want = R.decoded(fc.name, order, channels)
        mine = got["status"][plan.seg_frame == i]
        assert [tuple(int(v) for v in row) for row in mine] == want.seg_status, fc.name
        assert got["codes"][i] == want.status, fc.name
        blocks = want.coef.shape[0]
        assert np.array_equal(coef[i, :blocks], want.coef), fc.name
        assert not coef[i, blocks:].any(), fc.name
        if want.status == R.OK:
            # jpeg_idct_kernel's own output, the component planes, where the frame descriptor puts them
            for c, ref in enumerate(R.planes_from_blocks(R.idct_blocks(want.coef), want.geometry)):
                off, pitch = (int(v) for v in plan.fd[i, 8 + 8 * c + 3:8 + 8 * c + 5])
                assert pitch == ref.shape[1], fc.name
                assert np.array_equal(planes[i, off:off + ref.size].reshape(ref.shape), ref), f"{fc.name}: plane {c}"
            assert np.array_equal(host[i], want.pixels), fc.name
            if pil and R.have_turbo() and fc.name not in NOT_FOR_PIL:
                assert np.array_equal(host[i], R.decode_with_pil(fc.data, order, channels)), fc.name
    for key in ("frames_buf", "coef_buf", "plane_buf"):
        assert _guards_intact(got[key]), key


def _derived_table(spec: np.ndarray) -> bytes:
    """jpeg_decode.h's jpeg_build_table on one (16 counts, 256 values) specification: the 512-entry lookup by the next 9
    bits ((symbol << 4) | length, 0 = none), the counts as the canonical walk uses them, the values."""
    fast, count = np.zeros(512, np.uint16), np.zeros(16, np.uint16)
    code = k = 0
    for length in range(1, 17):
        n = max(0, min(int(spec[length - 1]), 256 - k, (1 << length) - code))
        count[length - 1] = n
        if length <= 9:
            for j in range(n):
                first = (code + j) << (9 - length)
                fast[first:first + (1 << (9 - length))] = int(spec[16 + ((k + j) & 255)]) << 4 | length
        code = (code + n) << 1
        k += n
    return fast.tobytes() + count.tobytes() + spec[16:272].tobytes()


def test_derived_code_tables_equal_their_statement(gpu_device):
    """jpeg_tables_kernel's only output: eight tables a frame, the undefined ones (all counts zero) included."""
    seen = set()
    for (h, w), group in list(_groups(R.files()).items())[:4]:
        got = jpeg._decode_clip([fc.data for fc in group], gpu_device, "rgb", 3)
        tables = got["tables"].cpu().numpy().reshape(len(group), 8, jpeg.TABLE_BYTES)
        for i, fc in enumerate(group):
            for t in range(8):
                assert tables[i, t].tobytes() == _derived_table(got["plan"].huff[i, t]), (fc.name, t)
                seen.add(bool(got["plan"].huff[i, t, :16].any()))
    assert seen == {False, True}


def _groups(cases):
    groups = {}
    for fc in cases:
        groups.setdefault((fc.h, fc.w), []).append(fc)
    return groups


@pytest.mark.parametrize("order", ["bgr", "rgb"])
def test_decode_every_file_equals_the_statement_and_pil(gpu_device, order):
    for (h, w), group in _groups(R.files()).items():
        got = jpeg._decode_clip([fc.data for fc in group], gpu_device, order, 3, guard=GUARD)
        assert got["frames"].shape == (len(group), h, w, 3) and got["frames"].is_contiguous()
        _check_clip(group, got, order)


def test_decode_gray_files_to_one_channel(gpu_device):
    for (h, w), group in _groups([fc for fc in R.files() if fc.c == 1]).items():
        got = jpeg._decode_clip([fc.data for fc in group], gpu_device, "bgr", 1, guard=GUARD)
        assert got["frames"].shape == (len(group), h, w, 1) and got["frames"].dtype == torch.uint8
        _check_clip(group, got, "bgr", 1)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_uploads_off_a_dword(gpu_device, offset):
    for size in ((37, 53), (17, 33)):
        group = [fc for fc in R.files() if (fc.h, fc.w) == size]
        got = jpeg._decode_clip([fc.data for fc in group], gpu_device, "rgb", 3, guard=GUARD, upload_offset=offset)
        _check_clip(group, got)


@pytest.mark.parametrize("count", R.SEGMENT_COUNTS)
def test_segment_counts_around_a_wave_in_one_launch(gpu_device, count):
    fc = next(f for f in R.extra_files() if f.name == f"segments-{count}")
    got = jpeg._decode_clip([fc.data], gpu_device, "rgb", 3, guard=GUARD)
    assert got["status"].shape == (count, 2)
    _check_clip([fc], got)


def test_one_long_serial_segment(gpu_device):
    fc = next(f for f in R.extra_files() if f.name == "long-segment")
    got = jpeg._decode_clip([fc.data], gpu_device, "bgr", 3, guard=GUARD)
    assert got["status"].shape == (1, 2) and int(got["status"][0, 1]) == 16 * 16
    _check_clip([fc], got, "bgr")


def _companion(h, w, seed):
    return R.pil_file(w, h, "420", 75, "noise", seed)


def test_malformed_streams_in_a_batch_with_good_frames(gpu_device, tmp_path):
    """Every malformed stream passed tools/jpeg_decode_check.cpp on the host before it came here."""
    for k, bf in enumerate(R.device_bad_files()):
        first, last = _companion(bf.h, bf.w, 2 * k), _companion(bf.h, bf.w, 2 * k + 1)
        got = jpeg._decode_clip([first, bf.data, last], gpu_device, "bgr", 3, guard=GUARD)
        want = R.decoded(bf.name)
        assert got["codes"] == [0, bf.status, 0] and want.status == bf.status, (bf.name, got["codes"])
        mine = got["status"][got["plan"].seg_frame == 1]
        assert [tuple(int(v) for v in row) for row in mine] == want.seg_status, bf.name
        coef = got["coef_buf"].cpu().numpy()[GUARD:-GUARD].view(np.int16).reshape(3, got["plan"].stride_blocks, 64)
        assert np.array_equal(coef[1, :want.coef.shape[0]], want.coef), bf.name
        host = got["frames"].cpu().numpy()
        assert np.array_equal(host[0], R.decode(first, "bgr").pixels) and np.array_equal(host[2], R.decode(last, "bgr").pixels), bf.name
        assert all(_guards_intact(got[key]) for key in ("frames_buf", "coef_buf", "plane_buf")), bf.name
        with pytest.raises(IOError, match="Failed to load frame: middle"):
            jpeg.decode_jpeg_device([first, bf.data, last], gpu_device, names=["first", "middle", "last"])
        paths = [tmp_path / f"{k}-{i}.jpg" for i in range(3)]
        for p, data in zip(paths, (first, bf.data, last)):
            p.write_bytes(data)
        with pytest.raises(IOError, match=f"Failed to load frame: .*{k}-1.jpg"):
            jpeg.load_jpeg_frames_device(paths, gpu_device)
    for bf in R.malformed_files():
        if not bf.status:
            with pytest.raises(bf.error):
                jpeg.decode_jpeg_device([bf.data], gpu_device)


def test_same_bytes_alone_in_a_batch_and_at_any_chunk_size(gpu_device, tmp_path):
    names = ("full-420-q75-noise", "full-444-q95-ramp", "full-gray-q30-checker")
    cases = [next(f for f in R.files() if f.name == n) for n in names]
    batch = jpeg.decode_jpeg_device([fc.data for fc in cases], gpu_device)
    for i, fc in enumerate(cases):
        assert torch.equal(jpeg.decode_jpeg_device([fc.data], gpu_device)[0], batch[i]), "a frame decodes to other bytes alone"
        assert np.array_equal(batch[i].cpu().numpy(), R.decoded(fc.name, "bgr").pixels)
    paths = [tmp_path / f"{i}.jpg" for i in range(3)]
    for p, fc in zip(paths, cases):
        p.write_bytes(fc.data)
    for chunk in (1, 2, None):
        got = jpeg.load_jpeg_frames_device(paths, str(gpu_device), chunk_frames=chunk)
        assert got.is_contiguous() and torch.equal(got, batch), chunk
    for i, p in enumerate(paths):
        assert np.array_equal(frameio.load_frame(p), batch[i].cpu().numpy())


def test_mixed_png_and_jpeg_lists(gpu_device, tmp_path):
    rng = np.random.default_rng(3)
    paths = []
    for i, suffix in enumerate((".png", ".jpg", ".jpeg", ".png", ".jpg")):
        p = tmp_path / f"{i:02d}{suffix}"
        frameio.save_frame(rng.integers(0, 256, size=(37, 53, 3), dtype=np.uint8), p)
        paths.append(p)
    os.rename(paths[1], tmp_path / "01.png")            # a JPEG under a PNG's name: the first bytes decide
    paths[1] = tmp_path / "01.png"
    for order in ("bgr", "rgb"):
        got = jpeg.load_images_device(paths, gpu_device, order)
        assert got.shape == (5, 37, 53, 3) and got.is_contiguous()
        for i, p in enumerate(paths):
            want = frameio.load_frame(p)
            assert np.array_equal(got[i].cpu().numpy(), want if order == "bgr" else want[:, :, ::-1]), (order, p.name)
    assert torch.equal(jpeg.load_images_device(paths[1:3], gpu_device), jpeg.load_jpeg_frames_device(paths[1:3], gpu_device))
    other = tmp_path / "other.jpg"
    frameio.save_frame(rng.integers(0, 256, size=(37, 54, 3), dtype=np.uint8), other)
    with pytest.raises(ValueError, match="37x54"):
        jpeg.load_images_device(paths + [other], gpu_device)
    with pytest.raises(ValueError, match="the files before it"):
        jpeg.load_images_device([paths[1], other], gpu_device)
    text = tmp_path / "notes.jpg"
    text.write_bytes(b"not an image")
    with pytest.raises(ValueError, match="neither a PNG nor a JPEG"):
        jpeg.load_images_device([paths[0], text], gpu_device)


def _v1_directory(tmp_path, n=3, by=4, bx=6, b=8, k=2, seed=21):
    """A 3-frame clip as the v1 client side receives it and the packed masks.  The v1 drivers take their frames under
    the names 00001.png ...; here those files hold JPEG data, which both readers tell by the first bytes."""
    rng = np.random.default_rng(seed)
    masks = np.zeros((n, by, bx), np.uint8)
    for i in range(n):
        for r in range(by):
            masks[i, r, rng.choice(bx, k, replace=False)] = 1
    d = tmp_path / "frames"
    for i in range(n):
        frameio.save_frame(rng.integers(0, 256, size=(by * b, (bx - k) * b, 3), dtype=np.uint8), d / f"{i + 1:05d}.jpg")
        os.rename(d / f"{i + 1:05d}.jpg", d / f"{i + 1:05d}.png")
        assert open(d / f"{i + 1:05d}.png", "rb").read(2) == b"\xff\xd8"
    frameio.save_block_masks(masks, tmp_path / "masks.npz")
    return str(d), str(tmp_path / "masks.npz"), b, [f"{i + 1:05d}.png" for i in range(n)]


def _same_files(dir_a, dir_b):
    assert sorted(os.listdir(dir_a)) == sorted(os.listdir(dir_b)) and os.listdir(dir_a)
    for name in os.listdir(dir_a):
        assert np.array_equal(frameio.load_frame(os.path.join(dir_a, name)), frameio.load_frame(os.path.join(dir_b, name))), (dir_b, name)


def test_v1_and_model_drivers_on_a_jpg_directory_with_both_readers(gpu_device, tmp_path):
    frames_dir, npz, b, names = _v1_directory(tmp_path)
    out = {}
    for reader in ("pil", "device"):
        out[reader] = str(tmp_path / f"v1-{reader}")
        drivers.restore_shrunk_frames(frames_dir, npz, b, out[reader], devices=[gpu_device], png_reader=reader)
        assert sorted(os.listdir(out[reader])) == names
    _same_files(out["pil"], out["device"])
    rounds = np.random.default_rng(12).integers(0, 3, size=(3, 4, 4)).astype(np.int32)
    # a model driver on a true .jpg directory: restored in place, so the "pil" writer writes JPEG files again
    jpgs = [n.replace(".png", ".jpg") for n in names]
    for reader in ("pil", "device"):
        d = tmp_path / f"dct-{reader}"
        d.mkdir()
        for name, jpg in zip(names, jpgs):
            (d / jpg).write_bytes(open(os.path.join(frames_dir, name), "rb").read())
        drivers.restore_dct_adaptive(str(d), rounds, 8, devices=[gpu_device], png_reader=reader)
        assert sorted(os.listdir(d)) == jpgs
    _same_files(str(tmp_path / "dct-pil"), str(tmp_path / "dct-device"))
    assert not np.array_equal(frameio.load_frame(tmp_path / "dct-pil" / jpgs[0]), frameio.load_frame(os.path.join(frames_dir, names[0])))


def test_v1_shard_pixels_never_visit_the_host(gpu_device, tmp_path, monkeypatch):
    """With reader and writer on the device a v1 shard over JPEG frames neither downloads a clip (`frames_to_host`)
    nor uploads frames (`save_frames`, `frames_to_device` of host arrays): only files go up and finished files come
    down."""
    from elvis_amd import recompose
    frames_dir, npz, b, names = _v1_directory(tmp_path)
    want = {k: str(tmp_path / "want" / k) for k in ("stretch_out", "out", "stretched")}
    drivers.stretch_shrunk_frames(frames_dir, npz, b, out_dir=want["stretch_out"], devices=[gpu_device], png_writer="device")
    drivers.restore_shrunk_frames(frames_dir, npz, b, want["out"], stretched_dir=want["stretched"], devices=[gpu_device], png_writer="device")

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
        _same_files(want[k], got[k])


def test_exported(gpu_device):
    fc = R.files()[0]
    assert np.array_equal(elvis_amd.decode_jpeg_device([fc.data], gpu_device, "rgb")[0].cpu().numpy(), R.decoded(fc.name).pixels)
