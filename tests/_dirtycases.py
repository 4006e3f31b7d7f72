"""The ledger of the dirty-allocation matrix: every place the package asks for uninitialised memory (`_dirty.sites()`)
and what shows that nothing depends on what that memory held.

SITES maps each site to one of
  ("case", id)                      a case below reaches it under poison (tests/test_gpu_dirty.py checks that it did),
  ("prefilled", "file::test", how)  an existing GPU test already hands the kernel that very buffer with chosen contents,
  ("host", why)                     the tensor never reaches a kernel as scratch.
A site that several cases reach names one of them; the others still run it.

CASES holds, per id, where the case comes from (the family's own reference module: no shape is invented here), how the
surface is run, the statement's value and the comparison.  Nothing in this module touches the GPU at import, and the
references are computed on first use, so the CPU ledger (tests/test_dirty_ledger.py) can read the table.

Integer-typed sites: a poisoned index that a kernel used before writing it would be an out-of-bounds access, so every
integer site's reason says where each element is written before it is read (read from the kernels, not tried out).
"""
import importlib
from dataclasses import dataclass
from typing import Callable, Tuple

import numpy as np
import torch

MAX_H, MAX_W, MAX_FRAMES = 136, 284, 8


@dataclass(frozen=True)
class Case:
    id: str
    family: str
    clip: Tuple[int, int, int]          # (frames, h, w) of the largest clip the case uploads; (0, 0, 0): no frames at all
    source: str                         # the reference module / test the case is borrowed from
    run: Callable                       # (device) -> {name: tensor | ndarray | bytes}, run under poison
    expected: Callable                  # () -> whatever `compare` takes, from the statement only
    compare: Callable                   # (got: {name: ndarray | bytes}, want) -> None, raises AssertionError
    min_frames: int = 0                 # the surface's own minimum clip length where that is above MAX_FRAMES
    prepare: Callable = None            # (device) -> None, before the poison: what the case needs from an unpoisoned device


CASES = {}


def _add(case: Case):
    assert case.id not in CASES, case.id
    CASES[case.id] = case


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)     # a copy: the shared inputs are read-only


def _once(fn):
    box = []

    def get():
        if not box:
            box.append(fn())
        return box[0]
    return get


def _exact(got, want):
    """Byte for byte: every named array has the statement's shape and contents."""
    assert set(got) == set(want), (sorted(got), sorted(want))
    for name, ref in want.items():
        g = got[name]
        if isinstance(ref, bytes):
            assert g == ref, f"{name}: the bytes differ"
            continue
        ref = np.asarray(ref)
        assert tuple(g.shape) == tuple(ref.shape), f"{name}: shape {g.shape}, the statement's {ref.shape}"
        diff = g.astype(np.int64) != ref.astype(np.int64)
        assert not diff.any(), (f"{name}: {int(diff.sum())} of {diff.size} differ, first at {tuple(np.argwhere(diff)[0])}: "
                                f"{g[diff][0]} against the statement's {ref[diff][0]}")


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    return float(np.where(np.isnan(err), np.inf, err).max()) if got.size else 0.0      # a NaN is never within a bar


# ----------------------------------------------------------------------------------------------------------- segment
def _segment(name, clip):
    R = importlib.import_module("_segment_ref")
    cases = _once(R.cases)
    stages = ("red", "sad", "shift", "M", "S", "Mn", "Sn", "F", "thr", "pre")       # tests/test_gpu_segment.py STAGES

    def run(dev):
        from elvis_amd import segment
        frames, order, kw = cases()[name]
        masks, det = segment.foreground_masks_device(_up(frames, dev), order, segment.SegmentConfig(**kw), details=True)
        return dict({s: det[s] for s in stages}, masks=masks)

    def expected():
        frames, order, kw = cases()[name]
        masks, det = R.segment(frames, order, R.SegmentConfig(**kw), details=True)
        return dict({s: det[s] for s in stages}, masks=masks)

    _add(Case(f"segment_{name}", "segment", clip, "_segment_ref.cases", run, expected, _exact))


_segment("21x23_n3", (3, 21, 23))
_segment("48x64_n5", (5, 48, 64))
_segment("21x23_n1", (1, 21, 23))            # one frame: `shift` is read by the terms kernel and never computed
_segment("flat_40x52_n3", (3, 40, 52))       # histogram and count stay at their cleared values


# ----------------------------------------------------------------------------------------------------------- LPIPS
def _lpips(cid, clip):
    R = importlib.import_module("_lpips_ref")

    def run(dev):
        from elvis_amd import lpips
        case = R.BY_ID[cid]
        a, b, m = R.inputs(case)
        model = lpips.LpipsAlex(None, dev)
        return {"score": lpips.lpips_device(_up(a, dev), _up(b, dev), model, masks=_up(m, dev), rect=case.rect, order=case.order)}

    def compare(got, want):
        err = R.rel(got["score"], want)
        assert got["score"].dtype == np.float64 and err <= R.DEVICE_BAR, (cid, got["score"], want, err)

    _add(Case(f"lpips_{cid}", "lpips", clip, "_lpips_ref.CASES", run, lambda: R.expected(cid), compare))


_lpips("rect_odd_masked", (2, 70, 90))
_lpips("min_31x31", (1, 31, 31))


def _lpips_distance():
    """tests/test_gpu_lpips.py::test_distance_per_tap, tap 0: 135 pixels, three workgroups, the last one ragged.  First
    accumulate=False into a poisoned `out`, then accumulate=True into an `out` the caller filled with 7."""
    R = importlib.import_module("_lpips_ref")
    tap, n, h, w = 0, 2, 5, 27
    c = R.TAP_CHANNELS[tap]

    def inputs():
        g = torch.Generator().manual_seed(tap)
        x, y = torch.relu(torch.randn(n, h, w, c, generator=g)), torch.relu(torch.randn(n, h, w, c, generator=g))
        x[0, 2, 3] = 0.0
        y[1, 4, 26] = x[1, 4, 26]
        return x, y

    def run(dev):
        from elvis_amd import lpips
        x, y = inputs()
        model = lpips.LpipsAlex(None, dev)
        fresh = torch.empty(n, dtype=torch.float64, device=dev)                 # poisoned: this call runs under poison
        lpips.distance_device(x.to(dev), y.to(dev), c, model.lin[tap], fresh, accumulate=False)
        filled = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
        lpips.distance_device(x.to(dev), y.to(dev), c, model.lin[tap], filled, accumulate=True)
        return {"fresh": fresh, "filled": filled}

    def expected():
        x, y = inputs()
        lin = R.weights()[f"lin{tap}.model.1.weight"].reshape(-1)
        xd, yd = x.permute(0, 3, 1, 2).double(), y.permute(0, 3, 1, 2).double()
        tol = importlib.import_module("test_gpu_lpips").distance_tolerance(xd, yd, lin)
        return R.tap_distance(xd, yd, lin).numpy(), tol

    def compare(got, want):
        d, tol = want
        assert (np.abs(got["fresh"] - d) <= tol).all(), (got["fresh"], d, tol)
        assert np.array_equal(got["filled"], 7.0 + got["fresh"]), (got["filled"], got["fresh"])     # one float64 add, as the kernel's

    _add(Case("lpips_distance_tap0", "lpips", (0, 0, 0), "test_gpu_lpips.py::test_distance_per_tap", run, expected, compare))


_lpips_distance()


# ----------------------------------------------------------------------------------------------------------- SSIM
def _ssim(cid, clip):
    K = importlib.import_module("_qualitycases")

    def run(dev):
        from elvis_amd import _lib, metrics
        case = K.BY_ID[cid]
        a, b, m = K.inputs(case)
        rects = None if case.rects is None else torch.tensor(case.rects, dtype=torch.int32, device=dev)
        C1, C2 = case.constants
        return {"ssim": metrics.ssim_mean_device(
            _up(a, dev), _up(b, dev), K.window(case.window), source=_lib.SSIM_LUMA if case.source == "luma" else _lib.SSIM_CHANNELS,
            border=_lib.SSIM_REFLECT if case.border == "reflect" else _lib.SSIM_VALID, C1=C1, C2=C2, cov_norm=1.0,
            pad=_lib.SSIM_PAD_AUTO if case.pad is None else case.pad, scale=case.scale, masks=_up(m, dev), rects=rects)}

    def compare(got, want):
        g = got["ssim"]
        assert g.shape == want.shape and g.dtype == np.float64
        assert (np.abs(g - want) <= K.BAR).all(), (cid, g, want)
        assert (g[want == 1.0] == 1.0).all()

    _add(Case(f"ssim_{cid}", "ssim", clip, "_qualitycases.CASES", run, lambda: K.expected(K.BY_ID[cid]), compare))


for _cid in ("batch_luma_reflect", "batch_channels_reflect", "batch_luma_valid", "batch_channels_valid"):
    _ssim(_cid, (3, 37, 53))


# ----------------------------------------------------------------------------------------------------------- VMAF
def _vmaf(cid, clip):
    """A clip of VMAF_PASS_FRAMES + 1 frames: the second pass reuses the first one's pyramids and tile partials."""
    K = importlib.import_module("_vmafcases")
    R = importlib.import_module("_vmaf_ref")

    def run(dev):
        from elvis_amd import vmaf
        ref, dis, prev, nxt = (_up(a, dev) for a in K.inputs(cid))
        feats = vmaf.vmaf_features_device(ref, dis, prev=prev, following=nxt)
        return {"features": feats, "scores": vmaf.vmaf_predict_device(feats, vmaf.make_vmaf_model(0))}

    def expected():
        from elvis_amd import vmaf
        want = K.expected(cid)
        return {"features": want, "scores": R.score(want, vmaf.make_vmaf_model(0))}

    def compare(got, want):
        for name in ("features", "scores"):
            assert _rel(got[name], want[name]) <= R.BAR, (cid, name, got[name], want[name])

    assert K.BY_ID[cid].n == R.PASS_FRAMES + 1
    _add(Case(f"vmaf_{cid}", "vmaf", clip, "_vmafcases.CASES", run, expected, compare))


_vmaf("pass_64x64_n5", (5, 64, 64))


def _vmaf_luma():
    """The luma plane of tests/_vmafcases.py's tall shape (1 x 260 x 20 is over the frame budget's height, so the
    rectangle is cut from the LPIPS clip instead): masked, inverted, odd rectangle."""
    L = importlib.import_module("_lpips_ref")
    R = importlib.import_module("_vmaf_ref")
    case = L.BY_ID["rect_odd_masked"]

    def run(dev):
        from elvis_amd import vmaf
        a, _, m = L.inputs(case)
        return {"luma": vmaf.luma_device(_up(a, dev), "bgr", masks=_up(m, dev), invert=True, rect=case.rect)}

    def expected():
        a, _, m = L.inputs(case)
        return {"luma": R.luma(a, "bgr", m, True, case.rect)}

    _add(Case("vmaf_luma_rect_odd_masked", "vmaf", (2, 70, 90), "_lpips_ref.CASES + _vmaf_ref.luma", run, expected, _exact))


_vmaf_luma()


# ----------------------------------------------------------------------------------------------------------- FVMD
def _fvmd_frechet():
    """The smallest case of tests/_fvmdcases.py that reaches gram, singular_values and finish."""
    K = importlib.import_module("_fvmdcases")
    R = importlib.import_module("_fvmd_ref")
    n, m, d = K.FRECHET[0]

    def run(dev):
        from elvis_amd import fvmd
        a, b = K.frechet_rows(n, m, d)
        a_d, b_d = _up(a, dev), _up(b, dev)
        gram, scalars = fvmd.gram_device(a_d, b_d)
        return {"gram": gram, "scalars": scalars, "distance": fvmd._frechet_tensor(a_d, b_d)}

    def expected():
        a, b = K.frechet_rows(n, m, d)
        gram, scalars = R.gram_parts(a, b)
        return gram, scalars, R.frechet(a, b), R.fd_scale(a, b)

    def compare(got, want):
        gram, scalars, fd, scale = want
        assert _rel(got["gram"], gram) <= R.BAR and _rel(got["scalars"], scalars) <= R.BAR
        err = abs(float(got["distance"][0]) - fd) / max(1.0, scale)
        assert err <= R.BAR, (got["distance"], fd, err)                          # NaN compares false: it fails here

    _add(Case(f"fvmd_frechet_{n}x{m}x{d}", "fvmd", (0, 0, 0), "_fvmdcases.FRECHET", run, expected, compare))


def _fvmd_hist():
    K = importlib.import_module("_fvmdcases")
    R = importlib.import_module("_fvmd_ref")
    name = next(iter(K.HIST))

    def run(dev):
        from elvis_amd import fvmd
        return {"rows": fvmd.motion_features_device(_up(K.hist_tracks(name), dev))}

    def compare(got, want):
        assert _rel(got["rows"], want) <= R.BAR

    _add(Case(f"fvmd_hist_{name}", "fvmd", (0, 0, 0), "_fvmdcases.HIST", run, lambda: K.hist_expected(name), compare))


def _fvmd_tracker():
    """The shortest clip the tracker takes: FVMD_MIN_SEQ frames of 64 x 65, one segment.  The surface refuses anything
    shorter, so this is the one case above MAX_FRAMES (min_frames says so; the ledger allows exactly that minimum)."""
    K = importlib.import_module("_fvmdcases")
    R = importlib.import_module("_fvmd_ref")
    kind, h, w, s = K.TRACKER

    def run(dev):
        from elvis_amd import fvmd
        tracks = fvmd.track_keypoints_device(_up(K.tracker_expected()["clip"], dev), s)
        return {"tracks": tracks}

    def compare(got, want):
        assert _rel(got["tracks"], want["tracks"]) <= R.BAR

    _add(Case(f"fvmd_tracker_{h}x{w}_s{s}", "fvmd", (s, h, w), "_fvmdcases.TRACKER", run, K.tracker_expected, compare, min_frames=s))


_fvmd_frechet()
_fvmd_hist()
_fvmd_tracker()


# ----------------------------------------------------------------------------------------------------------- inpaint, tfill
def _inpaint_pixels(name, clip):
    R = importlib.import_module("_inpaint_ref")
    cases = _once(R.cases)

    def run(dev):
        from elvis_amd import inpaint
        frames, masks = cases()[name]
        return {"out": inpaint.inpaint_device(_up(frames, dev), _up(masks, dev))}

    _add(Case(f"inpaint_{name}", "inpaint", clip, "_inpaint_ref.cases", run, lambda: {"out": R.inpaint(*cases()[name])}, _exact))


def _inpaint_blocks():
    R = importlib.import_module("_inpaint_ref")
    given = _once(lambda: importlib.import_module("test_gpu_inpaint")._block_case())

    def run(dev):
        from elvis_amd import inpaint
        frames, bm, b = given()
        return {"out": inpaint.inpaint_blocks_device(_up(frames, dev), _up(bm, dev), b)}

    def expected():
        frames, bm, b = given()
        return {"out": R.inpaint(frames, R.expand_block_mask(bm, b, frames.shape[1], frames.shape[2]))}

    _add(Case("inpaint_blocks_44x61_b8", "inpaint", (3, 44, 61), "test_gpu_inpaint.py::_block_case", run, expected, _exact))


_inpaint_pixels("odd_random60", (1, 37, 53))
_inpaint_pixels("mixed_clip", (4, 40, 50))
_inpaint_blocks()


def _tfill(name, clip):
    R = importlib.import_module("_tfill_ref")
    cases = _once(R.cases)

    def run(dev):
        tf = importlib.import_module("elvis_amd.inpaint_temporal")
        frames, masks, p = cases()[name]
        out, left = tf.temporal_fill_device(_up(frames, dev), _up(masks, dev), **p)
        return {"out": out, "left": left}

    def expected():
        frames, masks, p = cases()[name]
        out, left = R.temporal_fill(frames, masks, **p)
        return {"out": out, "left": left}

    _add(Case(f"tfill_{name}", "tfill", clip, "_tfill_ref.cases", run, expected, _exact))


_tfill("ragged_33x49_c3", (5, 33, 49))


# ----------------------------------------------------------------------------------------------------------- complexity
def _complexity(cid, clip):
    R = importlib.import_module("_complexity_ref")

    def run(dev):
        from elvis_amd import complexity
        case = R.BY_ID[cid]
        frames, prev = R.inputs(case)
        sc, tc = complexity.block_complexity_device(_up(frames, dev), case.block, case.order, prev=_up(prev, dev))
        return {"sc": sc, "tc": tc}

    def compare(got, want):
        assert R.within_bar(got["sc"], want[0]) and R.within_bar(got["tc"], want[1]), (cid, R.worst(got["sc"], want[0]),
                                                                                        R.worst(got["tc"], want[1]))

    _add(Case(f"complexity_{cid}", "complexity", clip, "_complexity_ref.NAMED", run, lambda: R.expected(cid), compare))


_complexity("named_b16_rgb_prev", (3, 37, 53))


# ----------------------------------------------------------------------------------------------------------- shrink, stretch
def _shrink_inputs():
    """The clip of tests/test_gpu_block_matrix.py's gather case 40 x 104 x 3, block 8 (5 x 13 blocks: more than one
    workgroup row, 24-byte segments), with scores that tie."""
    rng = np.random.default_rng(40 + 104 + 8)
    frames = rng.integers(0, 256, size=(2, 40, 104, 3), dtype=np.uint8)
    scores = rng.integers(0, 50, size=(2, 5, 13)).astype(np.float64) / 50
    return frames, scores, 8, 0.333


def shrink_topk_statement(frames, scores, b, amount):
    """The statement's shrink by top-k and the flat stretch back, of any clip and scores."""
    R = importlib.import_module("_shrink_ref")
    k = R.topk_count(amount, scores.shape[2])
    sel = [R.topk_select(s, k) for s in scores]
    out = np.stack([R.gather_blocks(f, so, b) for f, (m, so) in zip(frames, sel)])
    mask = np.stack([m for m, so in sel])
    return {"out": out, "mask": mask, "src_of": np.stack([so for m, so in sel]),
            "back": np.stack([R.stretch_frame(o, m, b) for o, m in zip(out, mask)]),
            "full": np.stack([np.repeat(np.repeat(m.astype(np.uint8) * 255, b, 0), b, 1) for m in mask])}


def _shrink_topk():
    def run(dev):
        from elvis_amd import shrink
        frames, scores, b, amount = _shrink_inputs()
        out, mask, src_of = shrink.shrink_topk_device(_up(frames, dev), _up(scores, dev), b, amount)
        back, full = shrink.stretch_device(out, mask, b, "flat", fullres_mask=True)
        return {"out": out, "mask": mask, "src_of": src_of, "back": back, "full": full}

    _add(Case("shrink_topk_stretch_40x104_b8", "shrink", (2, 40, 104), "test_gpu_shrink.py::test_full_size_clips_equal_restatement",
              run, lambda: shrink_topk_statement(*_shrink_inputs()), _exact))


def _shrink_passes(mode):
    R = importlib.import_module("_shrink_ref")

    def run(dev):
        from elvis_amd import shrink
        frames, scores, b, amount = _shrink_inputs()
        out, mask, src_of, ridx, counts = shrink.shrink_passes_device(_up(frames, dev), _up(scores, dev), b, amount, mode)
        got = {"out": out, "mask": mask, "src_of": src_of, "ridx": ridx, "counts": np.asarray(counts, np.int64)}
        if mode == "rows":
            got["back"] = shrink.stretch_device(out, mask, b, "rows")
        return got

    def expected():
        frames, scores, b, amount = _shrink_inputs()
        by, bx = scores.shape[1:]
        sel = [R.passes_select(s, int(by * bx * amount), mode == "rows") for s in scores]
        want = {"out": np.stack([R.gather_blocks(f, origin, b, (by, bx)) for f, (m, origin, passes) in zip(frames, sel)]),
                "mask": np.stack([m for m, o, p in sel]), "src_of": np.stack([o for m, o, p in sel]),
                "ridx": np.stack([np.concatenate(p) if p else np.zeros(0, np.int32) for m, o, p in sel]),
                "counts": np.asarray([len(p) for p in sel[0][2]], np.int64)}
        if mode == "rows":
            want["back"] = np.stack([R.stretch_frame_row_only(o, m, b) for o, m in zip(want["out"], want["mask"])])
        return want

    _add(Case(f"shrink_passes_{mode}_40x104_b8", "shrink", (2, 40, 104), "test_gpu_shrink.py::test_full_size_clips_equal_restatement",
              run, expected, _exact))


_shrink_topk()
_shrink_passes("rows")
_shrink_passes("rows_cols")



# ----------------------------------------------------------------------------------------------------------- PNG writer
def _png_write():
    """tests/test_gpu_png.py::test_types_statistics_and_guard_bytes: adaptive filter, 33 x 65 in segments of 2 rows (17
    segments a frame), guard = 64 so that `types`, `stats_d` and `out` are all fresh allocations."""
    R = importlib.import_module("_png_ref")
    guard = 64
    index = _once(lambda: R.CASE_IDS.index("content-diag-fadaptive"))

    def run(dev):
        from elvis_amd import png
        case = R.CASES[index()]
        out, plan, types = png._encode_clip(_up(case.frames(), dev), case.order, case.filt, case.segment_rows, "test", guard=guard)
        host = out.cpu().numpy()
        total = int(plan.file_offsets[-1])
        files = png._finish_files(host[guard:guard + total].copy(), plan, case.h, case.w, case.c)
        got = {f"file{i}": v.tobytes() for i, v in enumerate(files)}
        got.update(types=types, guard_lo=host[:guard], guard_hi=host[guard + total:])
        return got

    def expected():
        encs = R.expected(index())
        want = {f"file{i}": e.file for i, e in enumerate(encs)}
        want.update(types=np.stack([e.types for e in encs]), guard_lo=np.full(guard, 0xA5, np.uint8), guard_hi=np.full(guard, 0xA5, np.uint8))
        return want

    _add(Case("png_write_diag_adaptive_33x65", "png_write", (3, 33, 65), "_png_ref.CASES", run, expected, _exact))


_png_write()


# ----------------------------------------------------------------------------------------------------------- PNG reader
PNG_READ_FILES = ("stream-stored-c3", "stream-fixed-c1", "stream-huffman-c4")     # a stored, a fixed and a dynamic stream


def _png_read():
    R = importlib.import_module("_png_read_ref")
    guard = 64

    def picked():
        by_name = {fc.name: fc for fc in R.files()}
        streams = {sc.name: sc for sc in R.good_streams()}
        return [by_name[n] for n in PNG_READ_FILES], [streams[n] for n in PNG_READ_FILES]

    def run(dev):
        import tempfile
        from elvis_amd import png
        files, streams = picked()
        frames, buf, filt_buf, codes = png._decode_clip([fc.data for fc in files], dev, "bgr", 3, guard=guard)
        ibuf, out_off, status = png._inflate_clip([sc.stream for sc in streams], [sc.cap for sc in streams], dev, guard=guard)
        host = ibuf.cpu().numpy()[guard:]
        got = {"pixels": frames, "codes": np.asarray(codes, np.int64), "status": status,
               "guards": np.concatenate([buf.cpu().numpy()[:guard], buf.cpu().numpy()[-guard:], filt_buf.cpu().numpy()[:guard],
                                         filt_buf.cpu().numpy()[-guard:], ibuf.cpu().numpy()[:guard], ibuf.cpu().numpy()[-guard:]])}
        for i, sc in enumerate(streams):
            got[f"inflated{i}"] = host[int(out_off[i]):int(out_off[i]) + int(status[i][1])].tobytes()
        with tempfile.TemporaryDirectory() as d:
            paths = []
            for i, fc in enumerate(files):
                paths.append(f"{d}/{i}.png")
                with open(paths[-1], "wb") as fh:
                    fh.write(fc.data)
            got["loaded"] = png.load_frames_device(paths, dev, "bgr", 3, chunk_frames=2)
        return got

    def expected():
        files, streams = picked()
        pixels = np.stack([R.decode_with_pil(fc.data, "bgr") for fc in files])
        inf = [R.inflated(sc.name) for sc in streams]
        want = {"pixels": pixels, "loaded": pixels, "codes": np.zeros(len(files), np.int64),
                "status": np.array([[w.status, len(w.out), w.consumed, w.adler] for w in inf], np.int64),
                "guards": np.full(6 * guard, 0xA5, np.uint8)}
        want.update({f"inflated{i}": w.out for i, w in enumerate(inf)})
        return want

    _add(Case("png_read_stored_fixed_dynamic_33x65", "png_read", (3, 33, 65), "_png_read_ref.files + good_streams", run, expected, _exact))


_png_read()


# ----------------------------------------------------------------------------------------------------------- JPEG reader
def _jpeg_group(size, clip, limit):
    """One size group of tests/_jpeg_ref.py's corpus through `_decode_clip` with guards (for 37 x 53 every ninth file:
    the group has 69, the budget is MAX_FRAMES a clip)."""
    R = importlib.import_module("_jpeg_ref")
    guard = 64

    def group():
        g = [fc for fc in R.files() if (fc.h, fc.w) == size]
        return g if len(g) <= limit else g[::(len(g) + limit - 1) // limit]

    def run(dev):
        from elvis_amd import jpeg
        got = jpeg._decode_clip([fc.data for fc in group()], dev, "rgb", 3, guard=guard)
        plan = got["plan"]
        out = {"pixels": got["frames"], "codes": np.asarray(got["codes"], np.int64), "status": got["status"]}
        coef = got["coef_buf"].cpu().numpy()[guard:-guard].view(np.int16).reshape(len(group()), plan.stride_blocks, 64)
        for i, fc in enumerate(group()):
            out[f"coef{i}"] = coef[i, :R.decoded(fc.name, "rgb", 3).coef.shape[0]]
        out["guards"] = np.concatenate([got[k].cpu().numpy()[e] for k in ("frames_buf", "coef_buf", "plane_buf")
                                        for e in (slice(0, guard), slice(-guard, None))])
        return out

    def expected():
        want = [R.decoded(fc.name, "rgb", 3) for fc in group()]
        assert all(w.status == R.OK for w in want)
        out = {"pixels": np.stack([w.pixels for w in want]), "codes": np.zeros(len(want), np.int64),
               "status": np.array([row for w in want for row in w.seg_status], np.int64), "guards": np.full(6 * guard, 0xA5, np.uint8)}
        out.update({f"coef{i}": w.coef for i, w in enumerate(want)})
        return out

    _add(Case(f"jpeg_group_{size[0]}x{size[1]}", "jpeg", clip, "_jpeg_ref.files", run, expected, _exact))


def _jpeg_bad_between_good():
    """tests/test_gpu_jpeg.py::test_malformed_streams_in_a_batch_with_good_frames, its 17 x 33 entry `bits-run-out`: the
    bad frame's planes are never written (its pixels are not compared: they are whatever the planes held), the good
    frames on either side must still be exact; then the two good files through the path loaders."""
    R = importlib.import_module("_jpeg_ref")

    def given():
        k, bf = next((k, b) for k, b in enumerate(R.device_bad_files()) if b.name == "bits-run-out")
        comp = importlib.import_module("test_gpu_jpeg")._companion
        return bf, comp(bf.h, bf.w, 2 * k), comp(bf.h, bf.w, 2 * k + 1)

    def run(dev):
        import tempfile
        from elvis_amd import jpeg
        bf, first, last = given()
        got = jpeg._decode_clip([first, bf.data, last], dev, "bgr", 3, guard=64)
        out = {"first": got["frames"][0], "last": got["frames"][2], "codes": np.asarray(got["codes"], np.int64),
               "bad_status": got["status"][got["plan"].seg_frame == 1]}
        with tempfile.TemporaryDirectory() as d:
            paths = [f"{d}/0.jpg", f"{d}/1.jpeg"]
            for path, data in zip(paths, (first, last)):
                with open(path, "wb") as fh:
                    fh.write(data)
            out["loaded"] = jpeg.load_jpeg_frames_device(paths, dev, chunk_frames=1)
            png_path = f"{d}/2.png"
            from elvis_amd import frameio
            frameio.save_frame(R.decode(first, "bgr").pixels, png_path)
            out["mixed"] = jpeg.load_images_device([paths[0], png_path, paths[1]], dev)
        return out

    def expected():
        bf, first, last = given()
        a, b = R.decode(first, "bgr").pixels, R.decode(last, "bgr").pixels
        return {"first": a, "last": b, "codes": np.array([0, bf.status, 0], np.int64),
                "bad_status": np.array(R.decoded(bf.name).seg_status, np.int64), "loaded": np.stack([a, b]), "mixed": np.stack([a, a, b])}

    _add(Case("jpeg_bad_between_good_17x33", "jpeg", (3, 17, 33), "_jpeg_ref.device_bad_files", run, expected, _exact))


_jpeg_group((37, 53), (8, 37, 53), MAX_FRAMES)
_jpeg_group((17, 33), (5, 17, 33), MAX_FRAMES)
_jpeg_bad_between_good()


# ----------------------------------------------------------------------------------------------------------- I420, Y4M
I420_SHAPES = ((3, 6, 18), (2, 18, 66), (3, 4, 12), (2, 6, 36))      # w % 16, w % 8 and w % 4 nonzero; w % 16 and w % 8 only; w % 16 only


def _i420():
    F = importlib.import_module("_handoff_ref")
    R = importlib.import_module("_i420_in_ref")

    def frames(shape):
        n, h, w = shape
        return np.random.default_rng(1000 * h + w + n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)

    def run(dev):
        from elvis_amd import handoff
        got = {}
        for shape in I420_SHAPES:
            for order in ("rgb", "bgr"):
                planes = handoff.rgb_to_i420_device(_up(frames(shape), dev), order)
                got[f"planes_{shape}_{order}"] = planes
                got[f"back_{shape}_{order}"] = handoff.i420_to_rgb_device(planes, order)
        return got

    def expected():
        want = {}
        for shape in I420_SHAPES:
            for order in ("rgb", "bgr"):
                planes = F.rgb_to_i420(frames(shape), order)
                want[f"planes_{shape}_{order}"] = planes
                want[f"back_{shape}_{order}"] = R.i420_to_rgb(planes, order)
        return want

    _add(Case("i420_both_ways", "i420", (2, 18, 66), "test_gpu_handoff.py / test_gpu_i420_in.py WIDTHS, HEIGHTS", run, expected, _exact))


def _y4m():
    """The clip fixture of tests/test_gpu_i420_in.py: five 18 x 6 frames; chunks of 2, so both staging slots and the
    copy stream are used."""
    F = importlib.import_module("_handoff_ref")
    R = importlib.import_module("_i420_in_ref")
    frames = _once(lambda: list(np.random.default_rng(31).integers(0, 256, (5, 6, 18, 3), dtype=np.uint8)))

    def run(dev):
        import tempfile
        from elvis_amd import handoff
        with tempfile.TemporaryDirectory() as d:
            handoff.write_y4m(frames(), f"{d}/clip.y4m", 29.97)
            return {"rgb": handoff.load_y4m_device(f"{d}/clip.y4m", dev, "rgb", chunk_frames=2),
                    "bgr_tail": handoff.load_y4m_device(f"{d}/clip.y4m", dev, "bgr", start=1, count=3)}

    def expected():
        planes = F.rgb_to_i420(np.stack(frames()))
        return {"rgb": R.i420_to_rgb(planes, "rgb"), "bgr_tail": R.i420_to_rgb(planes, "bgr")[1:4]}

    _add(Case("i420_load_y4m_6x18_n5", "i420", (5, 6, 18), "test_gpu_i420_in.py::clip", run, expected, _exact))


_i420()
_y4m()


# ----------------------------------------------------------------------------------------------------------- per-block families
def _blocks(cid, clip):
    """A case of tests/_blockref.py whose frame is whole blocks, run without `out=`: `_block_out` picks `empty_like`."""
    R = importlib.import_module("_blockref")
    case = _once(lambda: next(c for c in R.CASES if c.id == cid))

    def run(dev):
        from elvis_amd import classical, degrade
        c = case()
        assert c.shape[1] % c.block == 0 and c.shape[2] % c.block == 0
        if c.op == "blend":
            frames, = R.inputs(c)
            return {"out": classical.temporal_blend_device(_up(frames, dev), c.tb)}
        frames, m = R.inputs(c)
        fd, md = _up(frames, dev), _up(m, dev)
        call = {"lanczos": lambda: classical.lanczos_restore_device(fd, md, c.block),
                "unsharp": lambda: classical.unsharp_restore_device(fd, md, c.block, c.halo),
                "downsample": lambda: degrade.degrade_downsample_device(fd, md, c.block),
                "gaussian": lambda: degrade.degrade_gaussian_device(fd, md, c.block),
                "dct": lambda: degrade.degrade_dct_device(fd, md)}[c.op]
        return {"out": call()}

    _add(Case(f"blocks_{cid}", "blocks", clip, "_blockref.CASES", run, lambda: {"out": R.expected(case())[0]}, _exact))


BLOCK_CASES = {"lanczos_c3_b8": (2, 24, 32), "unsharp_c3_b8_halo0": (1, 32, 40), "downsample_b8_c1_n3": (3, 24, 24),
               "gaussian_b5_total64_n1_c1": (1, 40, 40), "dct_noise_c3": (1, 24, 24), "blend_five_frames_tb1": (5, 7, 9)}
for _cid, _clip in BLOCK_CASES.items():
    _blocks(_cid, _clip)


def presley_given(kind, b=8):
    """(frames, maps) of the presley cases: tests/test_gpu_presley_degrade.py's maps on its frames cut to whole blocks."""
    T = importlib.import_module("test_gpu_presley_degrade")
    if kind == "scale":
        values = np.arange(-1, b + 2, dtype=np.int32)
        bx = (len(values) + 1) // 2
        grid = np.full(2 * bx, 3, np.int32)
        grid[:len(values)] = values
        maps = np.stack([grid.reshape(2, bx), grid[::-1].reshape(2, bx)])
        return T._frames(100 * b + 3, 2, 2 * b, bx * b, 3), maps
    maps = np.array([[[-1, 0, 1], [2, 10, 64]], [[64, 10, 2], [1, 0, -1]]], np.int32)
    return T._frames(200 * b + 3, 2, 2 * b, 3 * b, 3), maps


def _presley(kind):
    """tests/test_gpu_presley_degrade.py's maps and block size 8 on its frames cut to whole blocks (the cases there are
    all ragged, and a ragged frame takes the `clone` branch of `_block_out`)."""
    R = importlib.import_module("_presley_degrade_ref")
    b = 8
    given = lambda: presley_given(kind, b)

    def run(dev):
        from elvis_amd import degrade
        frames, maps = given()
        fn = degrade.degrade_scale_device if kind == "scale" else degrade.degrade_gaussian_fx_device
        return {"out": fn(_up(frames, dev), _up(maps, dev), b)}

    def expected():
        frames, maps = given()
        return {"out": (R.scale_clip if kind == "scale" else R.blur_clip)(frames, maps, b)}

    _add(Case(f"presley_{kind}_b8_whole_blocks", "presley", (2, 16, 48) if kind == "scale" else (2, 16, 24),
              "test_gpu_presley_degrade.py", run, expected, _exact))


_presley("scale")
_presley("gaussian")


# ----------------------------------------------------------------------------------------------------------- enhance
def _resize():
    E = importlib.import_module("_enhance_ref")
    name = "tile16x64_plus1"

    def run(dev):
        from elvis_amd import enhance
        hs, ws, hd, wd = E.RESIZE_CASES[name]
        return {"out": enhance.resize_lanczos4_device(_up(E.resize_inputs(name, 3, "random"), dev), hd, wd)}

    def expected():
        hs, ws, hd, wd = E.RESIZE_CASES[name]
        return {"out": E.resize(E.resize_inputs(name, 3, "random"), hd, wd)}

    hs, ws, hd, wd = E.RESIZE_CASES[name]
    _add(Case(f"enhance_resize_{name}", "enhance", (2, max(hs, hd), max(ws, wd)), "_enhance_ref.RESIZE_CASES", run, expected, _exact))


def _enhance(model_name):
    """tests/test_gpu_enhance.py::test_pre_pad_is_forward_on_the_padded_frame: 9 x 13, tile 8, tile_pad 3, pre_pad 4,
    through a model BUILT under poison (its weights, its activation buffers and the enhancer's tiles are all fresh),
    against the statement's composition (tests/_enhance_ref.py `compose`) around the forward of a model built before."""
    box = {}

    def frames():
        return np.random.default_rng(33).integers(0, 256, size=(2, 9, 13, 3), dtype=np.uint8)

    def prepare(dev):
        if not box:
            T = importlib.import_module("test_gpu_enhance")
            box["sd"] = T._state_dict(dev, model_name)
            box["want"] = T._composition(T._model(dev, model_name), frames(), 8, 3, 4)

    def run(dev):
        from elvis_amd import enhance, restore, weights
        cfg = restore._check_realesrgan_args(1.0, 0, False, model_name)
        if isinstance(cfg, weights.SRVGGConfig):
            from elvis_amd.srvgg import SRVGGModel as Model
        else:
            from elvis_amd.realesrgan import RRDBNetModel as Model
        model = Model(cfg, box["sd"], dev)
        return {"out": enhance.RealESRGANer(model, tile=8, tile_pad=3, pre_pad=4).enhance_device(_up(frames(), dev))}

    _add(Case(f"enhance_tiles_pre_pad_{model_name}", "enhance", (2, 9, 13), "test_gpu_enhance.py", run, lambda: {"out": box["want"]},
              _exact, prepare=prepare))


_resize()
_enhance("realesr-animevideov3")
_enhance("RealESRGAN_x4plus_anime_6B")


# ----------------------------------------------------------------------------------------------------------- packed weights
# One conv of tests/_convref.py's matrix per pack format, each with pad rows or pad K-slots in its packed image.
CONV_CASES = {
    "igemm_f16_s2_t1": "f16 igemm, cout 70 of 72",
    "igemm_f32_1x1_t3": "f32 igemm, cin 24, cout 3 of 4",
    "f16_16_ks3_a0": "halo f16, cin 40, cout 3",
    "f16_64_ks3_pro_a0": "halo f16, cin2 = 24 > 0, prologue, fused statistics",
    "f16_up_ragged_cout": "sub-pixel up-conv (four 2x2 packs), cout 70, fused statistics",
    "x3p_64_ks3_a0": "the planar x3 format, cin 40 padded to K = 64",
    "x3_64_cat_a0": "the interleaved x3 format, cin2 = 8 > 0",
    "ws_1_16": "weight-stationary, cin 24",
    "s2d_f16_pad1": "space-to-depth down-conv, fused statistics",
}


def _conv(cid):
    R = importlib.import_module("_convref")
    box = {}

    def run(dev):
        T = importlib.import_module("test_gpu_conv_matrix")
        case = next(c for c in R.CASES if c.id == cid)
        y, pads, st, r, names, last = T._run(case, dev)         # packs under poison; activations from torch.zeros, as there
        assert last == case.expect, (cid, last)
        box.update(case=case, ref=r)          # the float64 reference of the seeded operands: the same in every run
        return {"y": y, "pads": pads} if st is None else {"y": y, "pads": pads, "stats": st}

    def compare(got, want):
        case, r = want
        y = torch.from_numpy(got["y"])
        ok, worst, at = R.tier1(y, r)
        assert ok, f"{cid}: tier 1 fails at {at} (worst {worst:.3f})"
        assert got["pads"].size == 0 or (got["pads"] == 0).all(), f"{cid}: pad channels not zeroed"
        if case.stats:
            ty = R.kernel_ty(case.expect)
            if case.kind == "up":
                parts = [R.tile_stats_ref(y, ty, parity=k) for k in range(4)]
                tpi = parts[0].shape[0] // case.n
                ref = torch.cat([p[i * tpi:(i + 1) * tpi] for i in range(case.n) for p in parts], 0)
            else:
                ref = R.tile_stats_ref(y, ty)
            ok, sw = R.stats_check(torch.from_numpy(got["stats"]), ref)
            assert ok, f"{cid}: per-tile statistics off (worst ratio {sw:.3f})"

    _add(Case(f"conv_{cid}", "conv", (0, 0, 0), "_convref.CASES", run, lambda: (box["case"], box["ref"]), compare))


for _cid in CONV_CASES:
    _conv(_cid)


def _swin():
    R = importlib.import_module("_modelref")
    box = {}
    pick = _once(lambda: next(c for c in R.CASES if c.op == "swin" and c.mode == 2))      # PROJ + MLP: the SwinBlock pack

    def run(dev):
        T = importlib.import_module("test_gpu_model_kernels_matrix")
        name, y, b = T._run_swin(pick(), dev)
        assert name == pick().expect
        box.update(ref=b)                     # the float64 reference of the seeded operands: the same in every run
        return {"y": y}

    def compare(got, want):
        y, b = torch.from_numpy(got["y"]), want
        ok, worst, at = R.tier1(y, b)
        assert ok, f"swin: tier 1 fails at {tuple(int(i) for i in at)} (worst {worst:.3f})"

    _add(Case("swin_block_pack", "swin", (0, 0, 0), "_modelref.CASES", run, lambda: box["ref"], compare))


_swin()



# ----------------------------------------------------------------------------------------------------------- masks, block SSIM
def _quality(cid, clip):
    K = importlib.import_module("_qualitycases")

    def run(dev):
        from elvis_amd import metrics
        case = K.BY_ID[cid]
        if case.op == "bbox":
            m, = K.inputs(case)
            return {"out": metrics.mask_bbox_device(_up(m, dev))}
        frames, m = K.inputs(case)
        return {"out": metrics.apply_mask_device(_up(frames, dev), _up(m, dev), case.invert)}

    _add(Case(f"quality_{cid}", "quality", clip, "_qualitycases.CASES", run, lambda: {"out": K.expected(K.BY_ID[cid])}, _exact))


def _block_ssim():
    """tests/test_gpu_metrics.py::test_block_ssim at block 12 (50 x 70 is no multiple of it), against the oracle's
    float64 restatement with that test's bound."""
    bar = 2e-5                                                     # the bound of test_block_ssim

    def given():
        b = 12
        rng = np.random.default_rng(b)
        f1 = [rng.integers(0, 256, size=(50, 70, 3), dtype=np.uint8) for _ in range(2)]
        f2 = [np.clip(f.astype(int) + rng.integers(-12, 13, f.shape), 0, 255).astype(np.uint8) for f in f1]
        f2[1][:b, :b] = f1[1][:b, :b]
        return np.stack(f1), np.stack(f2), b

    def run(dev):
        from elvis_amd import metrics
        f1, f2, b = given()
        return {"ssim": metrics.block_ssim_device(_up(f1, dev), _up(f2, dev), b)}

    def expected():
        from oracle import glue_ref
        f1, f2, b = given()
        return np.stack([glue_ref.block_ssim(x, y, b) for x, y in zip(f1, f2)])

    def compare(got, want):
        g = got["ssim"]
        assert g.shape == want.shape and g.dtype == np.float32 and not np.isnan(g).any()
        assert np.abs(g - want).max() < bar

    _add(Case("quality_block_ssim_50x70_b12", "quality", (2, 50, 70), "test_gpu_metrics.py::test_block_ssim", run, expected, compare))


_quality("bbox_n3_5x7_empty_middle", (3, 5, 7))        # a frame whose box stays at its initial value
_quality("apply_c3_p17_off0_inv", (1, 1, 17))           # 17 pixels: one past the 16-pixel group
_block_ssim()


# ----------------------------------------------------------------------------------------------------------- the model pipelines
# The restore drivers have no float64 statement of their own; their kernels do, and those run above.  What is asked of
# the drivers here is the property itself: the bytes of a run whose fresh allocations were poisoned are the bytes of a
# run before the poison (`prepare`), and the same under both poisons.  Three different starting states cannot agree on a
# byte that depends on the state.
def _surface_frames(n, h, w, seed):
    return importlib.import_module("test_gpu_surfaces")._frames(n, h, w, seed)


def _pipeline(cid, clip, source, call):
    box = {}

    def prepare(dev):
        if not box:
            box["want"] = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in call(dev).items()}

    _add(Case(cid, "pipeline", clip, source, call, lambda: box["want"], _exact, prepare=prepare))


def _sinsr_frames(dev):
    from elvis_amd import restore
    from elvis_amd.weights import tiny_config
    frames = _surface_frames(4, 64, 96, 7)
    maps = np.random.default_rng(8).integers(0, 3, size=(4, 8, 12)).astype(np.int32)
    return {"out": np.stack(restore.restore_frames_sinsr(frames, maps, 8, dev, cfg=tiny_config()))}


def _single4x(dev):
    from elvis_amd import restore
    from elvis_amd.weights import tiny_config
    model = restore.get_sinsr_model(dev, cfg=tiny_config())
    frames = np.stack(_surface_frames(5, 64, 96, 21))
    lv = np.random.default_rng(22).integers(0, 3, size=(5, 8, 12)).astype(np.int32)
    lv[3] = 0
    fh, lh = torch.from_numpy(frames).pin_memory(), torch.from_numpy(lv).pin_memory()
    gidx = [40 + i for i in range(5)]
    resident = restore.restore_clip_single4x_device(model, fh.to(dev), lh.to(dev), 8, gidx, batch=2)
    model.__dict__.pop("_host_pipelines", None)          # the staging is kept on the model: this call allocates its own
    out, dev_buf = restore.restore_clip_single4x_host(model, fh, lh, 8, gidx, None, batch=2, want_device=True)
    torch.cuda.synchronize(dev)
    return {"resident": resident, "host": out, "device_copy": dev_buf}


def _slot_host(kind):
    def call(dev):
        import elvis_amd as E
        from elvis_amd import restore
        frames = _surface_frames(7, 64, 96, 31)
        bm = np.random.default_rng(32).integers(0, 4, size=(7, 8, 12)).astype(np.int32)
        bm[2] = 0
        bm[5] = np.minimum(bm[5], 1)
        fn, kw = (E.restore_frames_blur, dict(batch_size=2)) if kind == "blur" else (E.restore_frames_dct, {})
        level = np.stack(fn(frames, bm, 8, dev, **kw))
        fh, mh = torch.from_numpy(np.stack(frames)).pin_memory(), torch.from_numpy(bm).pin_memory()
        model = restore._get_restorer(kind, dev, False)
        model.__dict__.pop("_host_pipelines", None)      # the staging is kept on the model: this call allocates its own
        out = restore.restore_clip_slot_host(kind, model, fh, mh, 8, None, batch_size=2, upload_chunk=3)
        torch.cuda.synchronize(dev)
        return {"frames_level": level, "host": out}
    return call


def _realesrgan_frames(dev):
    from elvis_amd import restore
    T = importlib.import_module("test_gpu_enhance")
    frames, maps = T._composition_inputs()
    name = "realesr-animevideov3"
    return {"out": np.stack(restore.restore_frames_realesrgan(frames, maps, 16, dev, model_name=name, state_dict=T._state_dict(dev, name)))}


_pipeline("pipeline_sinsr_frames_64x96", (4, 64, 96), "test_gpu_surfaces.py::test_pool_threads_on_one_device", _sinsr_frames)
_pipeline("pipeline_single4x_host_64x96", (5, 64, 96), "test_gpu_surfaces.py::test_host_to_host_pipeline_equals_device_path", _single4x)
_pipeline("pipeline_slot_host_blur_64x96", (7, 64, 96), "test_gpu_surfaces.py::test_slot_host_pipelines_equal_the_frames_level_drivers",
          _slot_host("blur"))
_pipeline("pipeline_slot_host_dct_64x96", (7, 64, 96), "test_gpu_surfaces.py::test_slot_host_pipelines_equal_the_frames_level_drivers",
          _slot_host("dct"))
_pipeline("pipeline_realesrgan_frames_32x48", (4, 32, 48), "test_gpu_enhance.py::_composition_inputs", _realesrgan_frames)


def _tiler():
    """tests/test_gpu_surfaces.py::test_p3_naive_restore_under_the_tiler's tiling (32-pixel tiles, halo 8, chunks of 2 with
    an overlap of 1) around a restorer that inverts, then the blend of test_blended_restoration: against the oracle's
    numpy tiler and blend, bit for bit."""
    kw = dict(tile_size=32, halo=8, chunk_size=2, chunk_overlap=1)
    invert = lambda frames, device=None, **_: [255 - f for f in frames]

    def given():
        rng = np.random.default_rng(6)
        frames = [rng.integers(0, 256, size=(64, 96, 3), dtype=np.uint8) for _ in range(3)]
        return frames, rng.integers(0, 3, size=(3, 4, 6)).astype(np.int32)

    def run(dev):
        from elvis_amd import tiler
        frames, maps = given()
        return {"tiled": np.stack(tiler.resource_aware_restore(invert, frames, device=str(dev), **kw)),
                "blended": np.stack(tiler.blended_restoration(frames, maps, 16, alpha=0.35, restore_fn=invert, device=str(dev), **kw))}

    def expected():
        from oracle import glue_ref
        frames, maps = given()
        rest = glue_ref.resource_aware_restore(invert, frames, device="cpu", **kw)
        return {"tiled": np.stack(rest), "blended": np.stack([glue_ref.blend_by_map(f, r, m, 16, 0.35) for f, r, m in zip(frames, rest, maps)])}

    _add(Case("pipeline_tiler_blend_64x96", "pipeline", (3, 64, 96), "test_gpu_surfaces.py (tiler, blended_restoration)", run, expected, _exact))


_tiler()



def _plane_merge():
    """ops.plane_merge without `out=` (the DCN restorer passes its own): the 9 x 13 frames of the enhance cases, three of
    them, merged from frame 1 on.  The statement is the kernel's written contract (csrc/dcn.hip), in float32 as there:
    out = rint(clip(frame / 255 + residual, 0, 1) * 255), the residual being channel 0 of plane (frame * 3 + colour)."""
    f0, nsel, h, w = PLANE_MERGE[:4]

    def run(dev):
        from elvis_amd import ops
        frames, res = plane_merge_given()
        return {"out": ops.plane_merge(_up(frames, dev), ops.Act(_up(res, dev), 1), f0, nsel)}

    _add(Case("pipeline_plane_merge_9x13", "pipeline", (3, h, w), "csrc/dcn.hip plane_merge_kernel's contract", run,
              lambda: plane_merge_statement(*plane_merge_given()), _exact))


PLANE_MERGE = (1, 2, 9, 13, 8)          # f0, nsel, h, w, pitch


def plane_merge_given(seed=33):
    f0, nsel, h, w, pitch = PLANE_MERGE
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, size=(3, h, w, 3), dtype=np.uint8)
    res = (rng.random((nsel * 3, h, w, pitch), dtype=np.float32) - np.float32(0.5)) * np.float32(0.8)
    return frames, res


def plane_merge_statement(frames, res):
    f0, nsel, h, w, pitch = PLANE_MERGE
    centre = frames[f0:f0 + nsel].astype(np.float32) / np.float32(255.0)
    r = res[..., 0].reshape(nsel, 3, h, w).transpose(0, 2, 3, 1)
    v = np.clip(centre + r, np.float32(0.0), np.float32(1.0)).astype(np.float32)
    return {"out": np.rint(v * np.float32(255.0)).astype(np.uint8)}


_plane_merge()


# ----------------------------------------------------------------------------------------------------------- the ledger
def _case(cid):
    return ("case", cid)


GLUE = "test_gpu_glue_matrix.py::test_glue_matrix"

SITES = {
    # segment
    ("elvis_amd.segment", "foreground_masks_device", "torch.empty"): _case("segment_48x64_n5"),
    ("elvis_amd.segment", "_details.<locals>.view", "torch.empty"):
        ("host", "a 0-dim CPU tensor asked only for its element_size(); nothing reads its contents"),
    # quality, LPIPS, VMAF, FVMD
    ("elvis_amd.metrics", "ssim_mean_device", "torch.empty"): _case("ssim_batch_luma_reflect"),
    ("elvis_amd.metrics", "mask_bbox_device", "torch.empty"): _case("quality_bbox_n3_5x7_empty_middle"),
    ("elvis_amd.metrics", "apply_mask_device", "torch.empty_like"): _case("quality_apply_c3_p17_off0_inv"),
    ("elvis_amd.metrics", "block_ssim_device", "torch.empty"): _case("quality_block_ssim_50x70_b12"),
    ("elvis_amd.lpips", "lpips_device", "torch.empty"): _case("lpips_rect_odd_masked"),
    ("elvis_amd.lpips", "distance_device", "torch.empty"): _case("lpips_distance_tap0"),
    ("elvis_amd.vmaf", "vmaf_features_device", "torch.empty"): _case("vmaf_pass_64x64_n5"),
    ("elvis_amd.vmaf", "vmaf_predict_device", "torch.empty"): _case("vmaf_pass_64x64_n5"),
    ("elvis_amd.vmaf", "luma_device", "torch.empty"): _case("vmaf_luma_rect_odd_masked"),
    ("elvis_amd.vmaf", "calculate_vmaf.<locals>.chunks", "torch.empty"):
        ("host", "the device side of an upload: `plane.copy_(host[:len(part)])` fills all of it before any kernel sees it"),
    ("elvis_amd.vmaf", "calculate_vmaf.<locals>.<listcomp>", "torch.empty"):
        ("host", "pinned staging that `readinto` fills; only the rows just read are uploaded (`host[:len(part)]`)"),
    ("elvis_amd.fvmd", "pyramid_device", "torch.empty"): _case("fvmd_tracker_64x65_s10"),
    ("elvis_amd.fvmd", "pyramid_device", "new_empty"): ("host", "the two 0-element levels returned for a clip of no frames"),
    ("elvis_amd.fvmd", "track_keypoints_device", "torch.empty"): _case("fvmd_tracker_64x65_s10"),
    ("elvis_amd.fvmd", "motion_features_device", "torch.empty"): _case("fvmd_hist_axes_S10_B1"),
    ("elvis_amd.fvmd", "gram_device", "torch.empty"): _case("fvmd_frechet_128x128x384"),
    ("elvis_amd.fvmd", "singular_values_device", "torch.empty"): _case("fvmd_frechet_128x128x384"),
    ("elvis_amd.fvmd", "_frechet_tensor", "torch.empty"): _case("fvmd_frechet_128x128x384"),
    # inpaint, tfill, complexity, shrink / stretch
    ("elvis_amd.inpaint", "_inpaint", "torch.empty"): _case("inpaint_mixed_clip"),
    ("elvis_amd.inpaint_temporal", "_fill", "torch.empty"): _case("tfill_ragged_33x49_c3"),
    ("elvis_amd.inpaint_temporal", "_fill", "torch.empty_like"): _case("tfill_ragged_33x49_c3"),
    ("elvis_amd.complexity", "block_complexity_device", "torch.empty"): _case("complexity_named_b16_rgb_prev"),
    ("elvis_amd.shrink", "shrink_topk_device", "torch.empty"): _case("shrink_topk_stretch_40x104_b8"),
    ("elvis_amd.shrink", "shrink_passes_device", "torch.empty"): _case("shrink_passes_rows_cols_40x104_b8"),
    ("elvis_amd.shrink", "stretch_index_device", "torch.empty"): _case("shrink_topk_stretch_40x104_b8"),
    ("elvis_amd.shrink", "block_gather_device", "torch.empty"): _case("shrink_topk_stretch_40x104_b8"),
    # the per-block families
    ("elvis_amd.ops", "_block_out", "torch.empty_like"): _case("blocks_lanczos_c3_b8"),
    ("elvis_amd.classical", "temporal_blend_device", "torch.empty_like"): _case("blocks_blend_five_frames_tb1"),
    # enhance and the Real-ESRGAN models
    ("elvis_amd.enhance", "resize_lanczos4_device", "torch.empty"): _case("enhance_resize_tile16x64_plus1"),
    ("elvis_amd.enhance", "gather_tiles_device", "torch.empty"): _case("enhance_tiles_pre_pad_realesr-animevideov3"),
    ("elvis_amd.enhance", "RealESRGANer.network_device", "torch.empty"): _case("enhance_tiles_pre_pad_realesr-animevideov3"),
    ("elvis_amd.srvgg", "SRVGGModel._alloc_buffers", "torch.empty"): _case("enhance_tiles_pre_pad_realesr-animevideov3"),
    ("elvis_amd.srvgg", "SRVGGModel._forward_batch", "torch.empty"): _case("enhance_tiles_pre_pad_realesr-animevideov3"),
    ("elvis_amd.realesrgan", "RRDBNetModel._alloc_buffers", "torch.empty"): _case("enhance_tiles_pre_pad_RealESRGAN_x4plus_anime_6B"),
    ("elvis_amd.realesrgan", "RRDBNetModel._alloc_buffers.<locals>.<listcomp>", "torch.empty"):
        _case("enhance_tiles_pre_pad_RealESRGAN_x4plus_anime_6B"),
    ("elvis_amd.realesrgan", "RRDBNetModel._forward_batch", "torch.empty"): _case("enhance_tiles_pre_pad_RealESRGAN_x4plus_anime_6B"),
    ("elvis_amd._srnet", "SRModel.forward", "torch.empty"): ("host", "the 0-element result returned for a clip without a frame or a pixel"),
    # codecs and the hand-off
    ("elvis_amd.png", "_encode_clip", "torch.empty"): _case("png_write_diag_adaptive_33x65"),
    ("elvis_amd.png", "_decode_clip", "torch.empty"): _case("png_read_stored_fixed_dynamic_33x65"),
    ("elvis_amd.png", "_launch_decode", "torch.empty"): _case("png_read_stored_fixed_dynamic_33x65"),
    ("elvis_amd.png", "_inflate_clip", "torch.empty"): _case("png_read_stored_fixed_dynamic_33x65"),
    ("elvis_amd.png", "load_frames_device", "torch.empty"): _case("png_read_stored_fixed_dynamic_33x65"),
    ("elvis_amd.jpeg", "_guarded", "torch.empty"): _case("jpeg_group_37x53"),
    ("elvis_amd.jpeg", "_launch_decode", "torch.empty"): _case("jpeg_group_37x53"),
    ("elvis_amd.jpeg", "load_jpeg_frames_device", "torch.empty"): _case("jpeg_bad_between_good_17x33"),
    ("elvis_amd.jpeg", "load_images_device", "torch.empty"): _case("jpeg_bad_between_good_17x33"),
    ("elvis_amd.handoff", "rgb_to_i420_device", "torch.empty"): _case("i420_both_ways"),
    ("elvis_amd.handoff", "i420_to_rgb_device", "torch.empty"): _case("i420_both_ways"),
    ("elvis_amd.handoff", "_planes_to_clip", "torch.empty"): _case("i420_load_y4m_6x18_n5"),
    ("elvis_amd.handoff", "_planes_to_clip.<locals>.<listcomp>", "torch.empty"): _case("i420_load_y4m_6x18_n5"),
    ("elvis_amd.drivers", "ClipFileSink.save", "torch.empty"):
        ("host", "pinned receive buffer of one download: `host.copy_(planes)` fills all of it before the file is written"),
    # packed weights and the conv wrappers
    ("elvis_amd.ops", "PackedConv.__init__", "torch.empty"): _case("conv_x3p_64_ks3_a0"),
    ("elvis_amd.ops", "PackedConv.__call__", "torch.empty"): _case("conv_f16_64_ks3_pro_a0"),
    ("elvis_amd.ops", "PackedUpConv.__call__", "torch.empty"): _case("conv_f16_up_ragged_cout"),
    ("elvis_amd.ops", "PackedDownConv.__init__", "torch.empty"): _case("conv_s2d_f16_pad1"),
    ("elvis_amd.ops", "PackedDownConv.__call__", "torch.empty"): _case("conv_s2d_f16_pad1"),
    ("elvis_amd.ops", "SwinFused.__init__", "torch.empty"): _case("swin_block_pack"),
    ("elvis_amd.ops", "new_act", "torch.empty"):
        ("prefilled", "test_gpu_conv_matrix.py::test_conv_matrix", "_nan_new_act fills every activation new_act hands out with NaN, pads included"),
}

SITES.update({
    # the u8 glue and the norm / misc kernels, through the model pipelines (and pre-filled by their own matrices besides)
    ("elvis_amd.ops", "area_downscale_u8", "torch.empty"): _case("pipeline_realesrgan_frames_32x48"),
    ("elvis_amd.ops", "recompose_u8", "torch.empty_like"): _case("pipeline_realesrgan_frames_32x48"),
    ("elvis_amd.ops", "blend_u8", "torch.empty_like"): _case("pipeline_tiler_blend_64x96"),
    ("elvis_amd.ops", "temporal_stack", "torch.empty"): _case("pipeline_slot_host_dct_64x96"),
    ("elvis_amd.ops", "u8_to_float", "torch.empty"): _case("pipeline_slot_host_blur_64x96"),
    ("elvis_amd.ops", "float_to_u8", "torch.empty"): _case("pipeline_slot_host_blur_64x96"),
    ("elvis_amd.ops", "vq_nearest", "torch.empty"): _case("pipeline_sinsr_frames_64x96"),
    ("elvis_amd.ops", "groupnorm_affine", "torch.empty"): _case("pipeline_sinsr_frames_64x96"),
    ("elvis_amd.ops", "select_levels_u8", "torch.empty_like"): ("prefilled", GLUE, "_run_select's output is an Out filled with each of FILLS"),
    ("elvis_amd.ops", "tile_normalize", "torch.empty"): ("prefilled", GLUE, "_run_normalize's output is an Out filled with each of FILLS"),
    ("elvis_amd.ops", "convert_act", "torch.empty"):
        ("prefilled", "test_gpu_norm_misc_matrix.py::test_convert_act_exact", "the output is _guarded: torch.full of the sentinel"),
    ("elvis_amd.ops", "plane_merge", "torch.empty"): _case("pipeline_plane_merge_9x13"),
    # the model pipelines
    ("elvis_amd.recompose", "upscale_adaptive_device", "torch.empty_like"): _case("pipeline_sinsr_frames_64x96"),
    ("elvis_amd.restore", "restore_frames_sinsr_device", "torch.empty_like"): _case("pipeline_sinsr_frames_64x96"),
    ("elvis_amd.restore", "restore_frames_realesrgan_device", "torch.empty_like"): _case("pipeline_realesrgan_frames_32x48"),
    ("elvis_amd.restore", "restore_clip_single4x_device", "torch.empty_like"): _case("pipeline_single4x_host_64x96"),
    ("elvis_amd.restore", "restore_clip_single4x_host", "torch.empty"): _case("pipeline_single4x_host_64x96"),
    ("elvis_amd.restore", "_HostClipPipeline.__init__", "torch.empty"): _case("pipeline_single4x_host_64x96"),
    ("elvis_amd.restore", "_HostClipPipeline.__init__", "torch.empty_like"): _case("pipeline_single4x_host_64x96"),
    ("elvis_amd.restore", "_HostClipPipeline.__init__.<locals>.<listcomp>", "torch.empty"): _case("pipeline_single4x_host_64x96"),
    ("elvis_amd.restore", "restore_clip_slot_host", "torch.empty"): _case("pipeline_slot_host_blur_64x96"),
    ("elvis_amd.restore", "_HostSlotPipeline.__init__", "torch.empty"): _case("pipeline_slot_host_blur_64x96"),
    ("elvis_amd.restore", "_HostSlotPipeline.__init__", "torch.empty_like"): _case("pipeline_slot_host_blur_64x96"),
    ("elvis_amd.restorers", "DCNRestorer.restore", "torch.empty"): _case("pipeline_slot_host_dct_64x96"),
    ("elvis_amd.tiler", "resource_aware_restore", "torch.empty"): _case("pipeline_tiler_blend_64x96"),
    # collectives
    ("elvis_amd.distributed", "all_gather_frames", "torch.empty"):
        ("host", "the receive buffer of all_gather_into_tensor: every rank's nmax frames are written by the collective"),
    ("elvis_amd.distributed", "all_gather_frames.<locals>.<listcomp>", "torch.empty_like"):
        ("host", "the receive list of all_gather, one whole tensor per rank, concatenated only after the collective"),
    ("elvis_amd.distributed", "restore_clip_sharded", "torch.empty"): ("host", "the 0-frame shard of a rank that was given no frame"),
})

# The ledger keys a site without line numbers, so a function that spells the same allocator more than once is one site;
# how often it does is kept here, and a second `torch.empty` added to such a function fails the ledger like any other.
SPELLINGS = {
    ('elvis_amd.complexity', 'block_complexity_device', 'torch.empty'): 2,
    ('elvis_amd.distributed', 'all_gather_frames.<locals>.<listcomp>', 'torch.empty_like'): 2,
    ('elvis_amd.fvmd', 'gram_device', 'torch.empty'): 3,
    ('elvis_amd.fvmd', 'pyramid_device', 'new_empty'): 2,
    ('elvis_amd.handoff', '_planes_to_clip.<locals>.<listcomp>', 'torch.empty'): 2,
    ('elvis_amd.metrics', 'ssim_mean_device', 'torch.empty'): 2,
    ('elvis_amd.ops', 'PackedConv.__init__', 'torch.empty'): 2,
    ('elvis_amd.ops', 'float_to_u8', 'torch.empty'): 2,
    ('elvis_amd.ops', 'groupnorm_affine', 'torch.empty'): 4,
    ('elvis_amd.png', '_encode_clip', 'torch.empty'): 3,
    ('elvis_amd.png', '_launch_decode', 'torch.empty'): 2,
    ('elvis_amd.realesrgan', 'RRDBNetModel._alloc_buffers', 'torch.empty'): 5,
    ('elvis_amd.realesrgan', 'RRDBNetModel._forward_batch', 'torch.empty'): 2,
    ('elvis_amd.restore', '_HostClipPipeline.__init__', 'torch.empty'): 3,
    ('elvis_amd.restore', '_HostSlotPipeline.__init__', 'torch.empty'): 2,
    ('elvis_amd.segment', 'foreground_masks_device', 'torch.empty'): 2,
    ('elvis_amd.shrink', 'block_gather_device', 'torch.empty'): 2,
    ('elvis_amd.shrink', 'shrink_passes_device', 'torch.empty'): 5,
    ('elvis_amd.shrink', 'shrink_topk_device', 'torch.empty'): 2,
    ('elvis_amd.srvgg', 'SRVGGModel._alloc_buffers', 'torch.empty'): 3,
    ('elvis_amd.vmaf', 'vmaf_features_device', 'torch.empty'): 2,
}

# Integer-typed sites: where every element is written before anything reads it (read from the kernels and wrappers; no
# case was run to find out).
INTEGER_SITES = {
    ("elvis_amd.segment", "foreground_masks_device", "torch.empty"):
        "ws: csrc/segment.hip clears sad, maxima, hist, count and shift with one hipMemsetAsync before the first launch (shift is "
        "added to pixel coordinates by the terms kernel); every other section is written whole by the kernel before the one that reads it",
    ("elvis_amd.inpaint", "_inpaint", "torch.empty"):
        "ws: workgroup 0 of inpaint_rows_kernel clears hist before inpaint_columns_kernel adds to it; inpaint_scan_kernel writes offs "
        "and cursor from hist before the scatter advances cursor; the fill reads list[offs[k] ...] for the count the host took from hist",
    ("elvis_amd.shrink", "shrink_topk_device", "torch.empty"):
        "src_of: shrink_select_topk_kernel writes exactly bx - k entries a row (a column is kept iff at least k beat it); the gather "
        "treats an index outside the source grid as a hole and never reads through it",
    ("elvis_amd.shrink", "shrink_passes_device", "torch.empty"):
        "ws_scores / ws_pos: shrink_select_passes_kernel copies the scores and writes pos[e] = e for every cell before the first pass; "
        "src_of is written for every shrunk cell from pos; ridx only up to the removals made, and the wrapper returns ridx[:, :sum(counts)]",
    ("elvis_amd.shrink", "stretch_index_device", "torch.empty"):
        "src_of: stretch_index_kernel writes every cell (a rank or -1); block_gather_u8_kernel bounds-checks what it reads from it",
    ("elvis_amd.metrics", "mask_bbox_device", "torch.empty"):
        "out: an output only; one workgroup a frame writes its four words, zeros for an empty mask; the host reads it after the launch",
    ("elvis_amd.png", "_encode_clip", "torch.empty"):
        "stats_d: png_stats_kernel, one workgroup a segment, stores all 260 words of its row (256 histogram bins from LDS, two Adler "
        "partials, the length, 0) before the host downloads them and sizes `out` from them; types: one byte a row, written by the same kernel",
    ("elvis_amd.jpeg", "_launch_decode", "torch.empty"):
        "tables_d: jpeg_tables_kernel builds all n * 8 tables (jpeg_build_table writes every fast[], count[] and values[] entry) before "
        "jpeg_entropy_kernel indexes them; the status words and the coefficients come from torch.zeros",
    ("elvis_amd.png", "_launch_decode", "torch.empty"):
        "streams_d and filt_buf hold bytes, not indices: the gather writes every stream byte, the inflater bounds every copy by the "
        "stream's capacity; the status and chunk words come from torch.zeros",
    ("elvis_amd.recompose", "upscale_adaptive_device", "torch.empty_like"):
        "new_lev: the map_out of recompose_u8, which writes every block's clamped level in the launch before the next stage reads it as "
        "its map (tests/test_gpu_glue_matrix.py pre-fills map_out with both FILLS)",
    ("elvis_amd.ops", "vq_nearest", "torch.empty"):
        "idx: an output only; one thread a pixel writes its index (tests/test_gpu_norm_misc_matrix.py pre-fills it with -7)",
    ("elvis_amd.restore", "_HostClipPipeline.__init__", "torch.empty"):
        "levels_d: the device side of an upload; every launch that reads frames [a, b) waits for the copy of levels [a, b)",
    ("elvis_amd.restore", "_HostSlotPipeline.__init__", "torch.empty"):
        "maps_d: the device side of an upload, copied chunk by chunk before the chunk's launches",
}

# Would the chosen case notice?  tests/test_dirty_ledger.py restates the cleared sections from the poison for the families
# that have one; the others say here why there is nothing to restate.
DISCRIMINATION = {
    "segment": "sad .. shift are cleared per call: hist -> Otsu's threshold and count -> the fallback are restated from the poison word "
               "through details=True (48x64_n5); flat_40x52_n3 and 21x23_n1 rest on the cleared values themselves",
    "inpaint": "the per-wave histogram is cleared by the rows kernel; the statement's `inpaint` takes no histogram (no hook is added), "
               "so `wave_counts` is restated from the poison: the host would read another deepest wave",
    "jpeg": "the coefficient buffer is cleared per call (torch.zeros): the statement's idct_blocks on a block whose uncoded "
            "coefficients hold the poison gives other samples",
    "tfill": "out and left are outputs written whole by tfill_kernel, nothing is accumulated in a fresh allocation; the statement's "
             "hooks (mutant=, stats=) take no buffer, and an unwritten output byte cannot equal both poisons",
    "shrink": "mask, src_of and the working copies are written whole before they are read and nothing is accumulated; "
              "`passes_select` has no hook for a working copy, and an unwritten output word cannot equal both poisons",
    "png": "the writer's bit buffer is LDS cleared by the kernel and `out` is written byte by byte (the host adds head and tail); the "
           "reader's status words come from torch.zeros; `encode(mutant=)` takes no buffer; an unwritten byte cannot equal both poisons",
}
