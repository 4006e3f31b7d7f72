"""ELVIS v1 shrink / stretch on the device: every public function against the reference's own outputs
(tests/golden/shrink.npz) and, on clips the goldens are too small for, against the numpy restatement
(tests/_shrink_ref.py).  Every comparison is exact equality on integers."""
import os

import numpy as np
import pytest
import torch

import _shrink_ref as R
import elvis_amd
from elvis_amd import _lib, drivers, frameio, shrink

pytestmark = pytest.mark.gpu


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _launch():
    return _lib.lib().elvis_last_launch().decode()


@pytest.fixture(scope="module")
def cases(golden_dir):
    with np.load(os.path.join(golden_dir, "shrink.npz"), allow_pickle=False) as z:
        return R.golden_cases(z)


def test_public_functions_equal_reference_outputs(gpu_device, cases):
    dev = str(gpu_device)
    for i, d in cases:
        b, amount, frame, scores = d["block"], d["amount"], d["frame"], d["scores"]
        f0, s0 = frame.copy(), scores.copy()
        by, bx = scores.shape
        if d["family"] == "elvis":
            shrunk, mask, coords = elvis_amd.apply_selective_removal(frame, scores, b, amount, device=dev)
            assert _same(shrunk, d["shrunk"]) and _same(mask, d["mask"]) and coords == d["coords"], i
            assert _same(elvis_amd.stretch_frame(d["shrunk"], d["mask"], b, device=dev), d["stretched"]), i
        elif d["family"] == "row_only":
            shrunk, mask = elvis_amd.shrink_frame_row_only(frame, scores, b, amount, device=dev)
            assert _same(shrunk, d["shrunk"]) and _same(mask, d["mask"]), i
            assert _same(elvis_amd.stretch_frame_row_only(d["shrunk"], d["mask"], b, device=dev), d["stretched"]), i
            outs, masks = elvis_amd.shrink_video_frames([frame, frame], [scores, scores], b, amount,
                                                        elvis_amd.shrink_frame_row_only, device=dev)
            assert all(_same(o, d["shrunk"]) for o in outs) and all(_same(m, d["mask"]) for m in masks), i
        else:
            shrunk, mask, pmap = elvis_amd.shrink_frame_position_map(frame, scores, b, amount, device=dev)
            assert _same(shrunk, d["shrunk"]) and _same(mask, d["mask"]) and _same(pmap, d["posmap"]), i
            shrunk2, mask2, ridx = elvis_amd.shrink_frame_removal_indices(frame, scores, b, amount, device=dev)
            assert _same(shrunk2, d["shrunk"]) and _same(mask2, d["mask"]), i
            assert len(ridx) == len(d["ridx"]) and all(_same(x, y) for x, y in zip(ridx, d["ridx"])), i
            assert _same(elvis_amd.stretch_frame_position_map(d["shrunk"], d["mask"], d["posmap"], b, device=dev), d["stretched"]), i
            assert _same(elvis_amd.stretch_frame_removal_indices(d["shrunk"], d["ridx"], by, bx, b, device=dev),
                         d["stretched_ridx"]), i
        got = elvis_amd.stretch_video_frames([d["shrunk"], d["shrunk"]], [d["mask"], d["mask"]], b, device=dev)
        assert len(got) == 2 and all(_same(g, d["stretched_presley"]) for g in got), i
        assert np.array_equal(frame, f0) and np.array_equal(scores, s0)


def _clip(rng, n, h, w, c):
    return rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)


def _scores(rng, n, by, bx, tied):
    if tied:
        return rng.integers(0, 50, size=(n, by, bx)).astype(np.float64) / 50
    return rng.random((n, by, bx))


@pytest.mark.parametrize("h,w,b,n,c,amount,tied", [
    (1080, 1920, 8, 1, 3, 0.25, False),        # whole row passes in the rows-only form, a partial column pass otherwise
    (1080, 1920, 8, 1, 3, 0.333, True),        # partial passes, tied scores
    (1072, 1920, 16, 7, 3, 0.4, True),
    (1072, 1920, 16, 1, 1, 0.95, False),       # deep sequence, one channel
    (1080, 1920, 8, 7, 1, 0.1, False),
])
def test_full_size_clips_equal_restatement(gpu_device, h, w, b, n, c, amount, tied):
    rng = np.random.default_rng(h + b + n + c)
    frames = _clip(rng, n, h, w, c)
    scores = _scores(rng, n, h // b, w // b, tied)
    fd = torch.from_numpy(frames).to(gpu_device)
    sd = torch.from_numpy(scores).to(gpu_device)
    by, bx = h // b, w // b
    # top-k needs whole blocks; with tied scores this checks the stated tie rule (the lower column first)
    if h % b == 0 and w % b == 0:
        out, mask, src_of = shrink.shrink_topk_device(fd, sd, b, amount)
        for i in range(n):
            m, so = R.topk_select(scores[i], R.topk_count(amount, bx))
            assert _same(mask[i].cpu().numpy(), m) and _same(src_of[i].cpu().numpy(), so)
            assert _same(out[i].cpu().numpy(), R.gather_blocks(frames[i], so, b))
        back, full = shrink.stretch_device(out, mask, b, "flat", fullres_mask=True)
        for i in range(n):
            m = mask[i].cpu().numpy()
            assert _same(back[i].cpu().numpy(), R.stretch_frame(out[i].cpu().numpy(), m, b))
            assert _same(full[i].cpu().numpy(), np.repeat(np.repeat(m.astype(np.uint8) * 255, b, 0), b, 1))
            keep = np.repeat(np.repeat(m == 0, b, 0), b, 1)
            assert np.array_equal(back[i].cpu().numpy()[keep], frames[i][keep])        # round trip on the kept blocks
    for mode, rows_only in (("rows", True), ("rows_cols", False)):
        out, mask, src_of, ridx, counts = shrink.shrink_passes_device(fd, sd, b, amount, mode)
        ridx_h = ridx.cpu().numpy()
        for i in range(n):
            m, origin, passes = R.passes_select(scores[i], int(by * bx * amount), rows_only)
            assert _same(mask[i].cpu().numpy(), m) and _same(src_of[i].cpu().numpy(), origin)
            assert counts == [len(p) for p in passes]
            assert _same(ridx_h[i], np.concatenate(passes) if passes else np.zeros(0, np.int32))
            assert _same(out[i].cpu().numpy(), R.gather_blocks(frames[i], origin, b, (by, bx)))
        if rows_only:
            back = shrink.stretch_device(out, mask, b, "rows")
            for i in range(n if n == 1 else 2):
                o, m = out[i].cpu().numpy(), mask[i].cpu().numpy()
                got = back[i].cpu().numpy()
                assert _same(got, R.stretch_frame_row_only(o, m, b))
                # the original on every block that is neither removed nor past the shrunk width (the row-only quirk)
                ok = (~m) & (np.cumsum(~m, axis=1) <= o.shape[1] // b)
                ok = np.repeat(np.repeat(ok, b, 0), b, 1)
                assert np.array_equal(got[ok], frames[i][:by * b, :bx * b][ok])
                assert not got[~ok].any()
    assert torch.equal(fd.cpu(), torch.from_numpy(frames)) and torch.equal(sd.cpu(), torch.from_numpy(scores))


@pytest.mark.parametrize("h,w,b,c,kernel", [
    (64, 96, 16, 3, "<16>"),         # 48-byte segments, 288-byte rows
    (64, 96, 16, 1, "<16>"),
    (40, 104, 8, 3, "<8>"),          # 24-byte segments
    (40, 104, 8, 1, "<8>"),
    (36, 60, 4, 3, "<4>"),           # 12-byte segments
    (35, 55, 5, 3, "<1>"),           # odd block sizes: per byte
    (21, 33, 3, 1, "<1>"),
    (28, 49, 7, 3, "<1>"),
    (67, 99, 16, 3, "<1>"),          # 16-byte segments would fit, the 297-byte source pitch does not
    (12, 20, 1, 3, "<1>"),           # one-pixel blocks
])
def test_gather_vector_and_per_byte_paths(gpu_device, h, w, b, c, kernel):
    rng = np.random.default_rng(h * w + b)
    n = 3
    frames = _clip(rng, n, h, w, c)
    by, bx = h // b, w // b
    fd = torch.from_numpy(frames).to(gpu_device)
    # an arbitrary map onto a destination grid of another size: repeats, holes and out-of-range indices
    dby, dbx = by + 1, max(1, bx - 2)
    src_of = rng.integers(-3, by * bx + 2, size=(n, dby, dbx)).astype(np.int32)
    out, full = shrink.block_gather_device(fd, torch.from_numpy(src_of).to(gpu_device), b, fullres_mask=True)
    assert _launch().endswith(kernel)
    for i in range(n):
        holes = np.where((src_of[i] < 0) | (src_of[i] >= by * bx), -1, src_of[i])
        assert _same(out[i].cpu().numpy(), R.gather_blocks(frames[i], src_of[i], b, (by, bx)))
        assert _same(full[i].cpu().numpy(), R.fullres_mask(holes, b))
    # shrink + stretch through the same kernel, into a caller's buffer
    scores = torch.from_numpy(rng.random((n, by, bx))).to(gpu_device)
    shrunk, mask, _, _, _ = shrink.shrink_passes_device(fd, scores, b, 0.3, "rows_cols")
    buf = torch.full((n, by * b, bx * b, c), 7, dtype=torch.uint8, device=gpu_device)
    got = shrink.stretch_device(shrunk, mask, b, "flat", out=buf)
    assert got is buf
    for i in range(n):
        assert _same(buf[i].cpu().numpy(), R.stretch_video_frames([shrunk[i].cpu().numpy()], [mask[i].cpu().numpy()], b)[0])
    assert torch.equal(fd.cpu(), torch.from_numpy(frames))


def test_clip_forms_do_not_depend_on_the_split(gpu_device):
    rng = np.random.default_rng(11)
    n, h, w, b = 6, 96, 160, 8
    frames = torch.from_numpy(_clip(rng, n, h, w, 3)).to(gpu_device)
    scores = torch.from_numpy(_scores(rng, n, h // b, w // b, True)).to(gpu_device)
    for fn in (lambda f, s: shrink.shrink_topk_device(f, s, b, 0.3)[:3],
               lambda f, s: shrink.shrink_passes_device(f, s, b, 0.37, "rows")[:4],
               lambda f, s: shrink.shrink_passes_device(f, s, b, 0.37, "rows_cols")[:4]):
        whole = fn(frames, scores)
        for cuts in ((0, 1, 6), (0, 4, 5, 6)):
            parts = [fn(frames[a:z].contiguous(), scores[a:z].contiguous()) for a, z in zip(cuts[:-1], cuts[1:])]
            for k, t in enumerate(whole):
                assert torch.equal(t, torch.cat([p[k] for p in parts]))
    shrunk, mask, _ = shrink.shrink_topk_device(frames, scores, b, 0.3)
    whole = shrink.stretch_device(shrunk, mask, b, "flat", fullres_mask=True)
    parts = [shrink.stretch_device(shrunk[a:z].contiguous(), mask[a:z].contiguous(), b, "flat", fullres_mask=True)
             for a, z in ((0, 2), (2, 6))]
    for k in range(2):
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts]))


def test_errors_on_the_device_surface(gpu_device):
    f = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=gpu_device)
    with pytest.raises(ValueError, match="float32 or float64"):
        shrink.shrink_topk_device(f, torch.zeros((1, 2, 2), dtype=torch.float16, device=gpu_device), 8, 0.5)
    with pytest.raises(ValueError, match="block grid"):
        shrink.shrink_passes_device(f, torch.zeros((1, 2, 3), dtype=torch.float64, device=gpu_device), 8, 0.5)
    with pytest.raises(ValueError, match="out must have"):
        shrink.stretch_device(f, torch.zeros((1, 2, 3), dtype=torch.uint8, device=gpu_device), 8, out=f)
    with pytest.raises(ValueError, match="C in"):
        shrink.block_gather_device(torch.zeros((1, 16, 16, 2), dtype=torch.uint8, device=gpu_device),
                                   torch.zeros((1, 2, 2), dtype=torch.int32, device=gpu_device), 8)
    with pytest.raises(RuntimeError, match="MI355X only"):
        elvis_amd.stretch_frame(np.zeros((8, 8, 3), np.uint8), np.zeros((1, 1), np.int8), 8, device="cpu")


def test_directory_driver_equals_frame_functions(gpu_device, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(5)
    n, by, bx, b = 5, 4, 6, 8
    d = tmp_path / "stretched"
    d.mkdir()
    masks, shrunk = [], []
    for i in range(n):
        frame = rng.integers(0, 256, size=(by * b, bx * b, 3), dtype=np.uint8)
        s, m, _ = elvis_amd.apply_selective_removal(frame, rng.random((by, bx)), b, 0.34, device=str(gpu_device))
        frameio.save_frame(s, d / f"{i + 1:05d}.png")
        shrunk.append(s)
        masks.append(m)
    frameio.save_block_masks(np.stack(masks), tmp_path / "shrink_masks_8.npz")
    full, blk = tmp_path / "removal_masks_fullres", tmp_path / "removal_masks"
    got = drivers.stretch_shrunk_frames(str(d), str(tmp_path / "shrink_masks_8.npz"), b, fullres_masks_dir=str(full),
                                        block_masks_dir=str(blk), devices=[gpu_device])
    assert np.array_equal(got, np.stack(masks))
    names = [f"{i + 1:05d}.png" for i in range(n)]
    assert sorted(os.listdir(d)) == sorted(os.listdir(full)) == sorted(os.listdir(blk)) == names
    for i, name in enumerate(names):
        assert np.array_equal(frameio.load_frame(d / name), elvis_amd.stretch_frame(shrunk[i], masks[i], b, device=str(gpu_device)))
        with Image.open(full / name) as im:
            assert np.array_equal(np.asarray(im), np.repeat(np.repeat(masks[i].astype(np.uint8) * 255, b, 0), b, 1))
        with Image.open(blk / name) as im:
            assert np.array_equal(np.asarray(im), masks[i].astype(np.uint8) * 255)
