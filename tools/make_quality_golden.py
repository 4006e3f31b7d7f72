"""Regenerate tests/golden/quality.npz from the reference's own quality-report code.

    python tools/make_quality_golden.py   # needs the reference (ELVIS_REFERENCE, see oracle/make_golden.py)

What is pinned is the reference's control flow, run from its own code through `oracle.make_golden.import_reference()`:
`_masked_ssim` (crop to the mask's box, zeroing, win_size choice, early returns), `_compute_mask_union_bbox` (padding
arithmetic and clipping), `_apply_binary_mask`, `_masked_psnr` / `_masked_mse`, `utils.compute_fg_bg_ssim` (FG / BG
defaulting), and from `_evaluate_single_video_metrics` and the function that prepares its context the statements
that build the ROI, choose the frame indices, loop over them and aggregate - taken by parsing elvis.py and
compiling exactly those statements into a function.

PARITY UNPINNED against cv2, skimage and pytorch_msssim themselves: the packages are absent.  `cv2.cvtColor` is
replaced by `tests/_quality_ref.luma_bgr`, `ssim` (skimage's structural_similarity) by
`_quality_ref.skimage_ssim_gaussian`, and `cv2.resize(..., INTER_NEAREST)` by `_quality_ref.nearest_resize`.

Only inputs and outputs are stored; the largest frame is 48 x 64.
"""
import ast
import os
import sys
from typing import Dict, List  # noqa: F401  (names the compiled statements' annotations use)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import make_golden  # noqa: E402
import _quality_ref as Q  # noqa: E402

H, W = 37, 53          # masked-SSIM frame
EH, EW, EN = 48, 64, 7   # evaluator clip
STRIDES = (1, 3)


def ssim_masks() -> Dict[str, np.ndarray]:
    """The mask list of the GPU tests (tests/test_gpu_quality.py builds its larger frames' masks the same way)."""
    m = {k: np.zeros((H, W), bool) for k in ("full", "blob", "box3x4", "box5x9", "box6x6", "strip2x40", "empty", "edges", "ring")}
    m["full"][:] = True
    yy, xx = np.mgrid[:H, :W]
    m["blob"] = ((yy - 17) ** 2 * 2 + (xx - 25) ** 2) < 150          # box starts at odd coordinates
    m["blob"][:9] = False
    m["box3x4"][5:8, 7:11] = True
    m["box5x9"][11:16, 3:12] = True
    m["box5x9"][13, 5] = False
    m["box6x6"][20:26, 30:36] = True
    m["strip2x40"][30:32, 5:45] = True
    m["edges"][0, 10] = m["edges"][H - 1, 20] = m["edges"][15, 0] = m["edges"][18, W - 1] = True
    m["edges"][10:20, 10:30] = True
    m["ring"][:] = True
    m["ring"][3:H - 3, 3:W - 3] = False
    return m


def _names(stmt) -> set:
    targets = stmt.targets if isinstance(stmt, ast.Assign) else [stmt.target] if isinstance(stmt, ast.AnnAssign) else []
    return {n.id for t in targets for n in ast.walk(t) if isinstance(n, ast.Name)}


def compile_evaluator(ref_elvis):
    """The reference's ROI, frame-index, per-frame loop and aggregation statements as one function."""
    tree = ast.parse(open(os.path.join(make_golden.REF, "elvis.py")).read())
    fns = {n.name: n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}
    worker = fns["_evaluate_single_video_metrics"]
    context = next(f for f in fns.values() if f is not worker and any("roi_slice" in _names(s) for s in f.body))
    roi = [s for s in context.body if _names(s) & {"fg_bbox", "bbox_x", "y_start", "y_stop", "x_start", "x_stop", "roi_slice"}]
    assert len(roi) == 7
    lists = {f"{r}_{k}" for r in ("fg", "bg") for k in ("psnr_vals", "ssim_vals", "mse_vals", "ref_lpips_frames", "dec_lpips_frames")}
    body = []
    for s in worker.body:
        if _names(s) & ({"total_reference_frames", "frame_count", "frame_indices", "result"} | lists):
            body.append(s)
        elif isinstance(s, ast.If) and any(isinstance(n, ast.Name) and n.id == "frame_indices" for n in ast.walk(s.test)):
            body.append(s)
        elif isinstance(s, ast.For) and isinstance(s.iter, ast.Name) and s.iter.id == "frame_indices":
            body.append(s)
    last = next(i for i, s in enumerate(body) if isinstance(s, ast.AnnAssign) and s.target.id == "result")
    body = body[:last + 1]                                   # what follows fills in the FVMD / LPIPS / VMAF keys
    kinds = [type(s).__name__ for s in body]
    assert kinds.count("For") == 1 and kinds.count("If") == 2 and kinds[-1] == "AnnAssign", kinds
    args = ["reference_frames", "decoded_frames", "fg_masks", "bg_masks", "width", "height", "metric_stride", "bitrate_bps",
            "masked_reference_fg_frames", "masked_decoded_fg_frames", "masked_reference_bg_frames", "masked_decoded_bg_frames"]
    ret = ast.Return(ast.Tuple([ast.Name(n, ast.Load()) for n in ("result", "frame_indices", "fg_bbox", "roi_slice")], ast.Load()))
    fn = ast.FunctionDef(name="core", args=ast.arguments(posonlyargs=[], args=[ast.arg(a) for a in args], kwonlyargs=[],
                                                         kw_defaults=[], defaults=[]), body=roi + body + [ret], decorator_list=[])
    mod = ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[]))
    ns = dict(vars(ref_elvis))
    exec(compile(mod, "elvis.py", "exec"), ns)
    return ns["core"]


def main() -> None:
    ref_elvis, ref_utils = make_golden.import_reference()
    cv2_stub = sys.modules["cv2"]
    assert not hasattr(cv2_stub, "GaussianBlur") and ref_elvis.ssim is None, "real cv2 / skimage installed: pin the packages instead"
    cv2_stub.COLOR_BGR2YCrCb, cv2_stub.INTER_NEAREST = 36, 0

    def cvt(img, code):
        assert code == cv2_stub.COLOR_BGR2YCrCb
        return np.repeat(Q.luma_bgr(img)[..., None], 3, axis=2)          # only channel 0 is read

    def resize(src, dsize, interpolation):
        assert interpolation == cv2_stub.INTER_NEAREST
        return Q.nearest_resize(src, dsize[1], dsize[0])

    win_sizes = []

    def ssim(a, b, data_range, gaussian_weights, win_size):
        assert data_range == 255 and gaussian_weights is True and a.dtype == np.uint8
        win_sizes.append(win_size)
        return Q.skimage_ssim_gaussian(a, b, win_size)

    cv2_stub.cvtColor, cv2_stub.resize, ref_elvis.ssim = cvt, resize, ssim
    rng = np.random.default_rng(20261018)
    out = {}

    # ---- _masked_ssim / _apply_binary_mask on one 37 x 53 pair
    yy, xx = np.mgrid[:H, :W]
    smooth = np.stack([96 + 80 * np.sin(yy / 5.0 + c) * np.cos(xx / 7.0 - c) for c in range(3)], axis=-1)
    ref = np.clip(smooth + rng.normal(0, 6, smooth.shape), 0, 255).astype(np.uint8)
    dec = np.clip(ref.astype(np.float64) + rng.normal(0, 9, ref.shape), 0, 255).astype(np.uint8)
    masks = ssim_masks()
    names = list(masks)
    keep = ref.copy(), dec.copy()
    values, wins, applied, applied_inv = [], [], [], []
    for k in names:
        before = len(win_sizes)
        values.append(ref_elvis._masked_ssim(ref, dec, masks[k]))
        wins.append(win_sizes[-1] if len(win_sizes) > before else 0)      # 0: an early return, ssim was never called
        applied.append(ref_elvis._apply_binary_mask(ref, masks[k]))
        applied_inv.append(ref_elvis._apply_binary_mask(ref, masks[k], invert=True))
    assert np.array_equal(ref, keep[0]) and np.array_equal(dec, keep[1])
    assert dict(zip(names, wins)) == dict(full=7, blob=7, box3x4=3, box5x9=5, box6x6=5, strip2x40=0, empty=0, edges=7, ring=7)
    out.update(ssim_ref=ref, ssim_dec=dec, ssim_mask_names=np.asarray(names), ssim_masks=np.stack([masks[k] for k in names]).astype(np.uint8),
               ssim_values=np.asarray(values + [ref_elvis._masked_ssim(ref, dec, None), ref_elvis._masked_ssim(ref, ref, masks["blob"])]),
               ssim_wins=np.asarray(wins, np.int32), applied=np.stack(applied), applied_inv=np.stack(applied_inv))

    # ---- _compute_mask_union_bbox: mask lists by index into ssim_masks (-1 = None), frame H x W
    lists = [[], [names.index("empty")], [names.index("empty"), -1], [names.index("box3x4")], [names.index("box3x4"), names.index("box6x6"), -1],
             [names.index("blob"), names.index("strip2x40")], [names.index("edges")], [names.index("ring")], [names.index("box5x9")]]
    ratios = [0.05, 0.05, 0.05, 0.05, 0.05, 0.3, 0.05, 0.05, 0.5]       # 0.5 on a box at the left edge: clipped padding
    boxes = [ref_elvis._compute_mask_union_bbox([None if i < 0 else masks[names[i]] for i in ids], W, H, r) for ids, r in zip(lists, ratios)]
    out.update(union_lists=np.asarray([ids + [-2] * (3 - len(ids)) for ids in lists], np.int32), union_ratios=np.asarray(ratios),
               union_boxes=np.asarray(boxes, np.int32))

    # ---- utils.compute_fg_bg_ssim: maps 3 x (4 x 6); masks same shape / to be resized / fewer than maps / all FG / all BG
    maps = [rng.random((4, 6)).astype(np.float32) for _ in range(3)]
    fg_cases = {"same": rng.random((3, 4, 6)), "resize": rng.random((3, 2, 3)), "fewer": rng.random((1, 4, 6)),
                "all_fg": np.ones((3, 4, 6)), "all_bg": np.zeros((3, 4, 6))}
    out["fgbg_maps"] = np.stack(maps)
    for k, m in fg_cases.items():
        out[f"fgbg_mask_{k}"] = m
        out[f"fgbg_out_{k}"] = np.asarray(ref_utils.compute_fg_bg_ssim(maps, m, 0.5))
    out["fgbg_out_thr"] = np.asarray(ref_utils.compute_fg_bg_ssim(maps, fg_cases["same"], 0.8))
    out["fgbg_out_nomaps"] = np.asarray(ref_utils.compute_fg_bg_ssim([], fg_cases["same"]))

    # ---- the evaluator: 7 frames of 48 x 64, a moving foreground, frame 2 without any
    core = compile_evaluator(ref_elvis)
    yy, xx = np.mgrid[:EH, :EW]
    refs, decs, fgs = [], [], []
    for i in range(EN):
        base = np.stack([110 + 70 * np.sin((yy + 2 * i) / 6.0 + c) * np.cos((xx - i) / 9.0) for c in range(3)], axis=-1)
        r = np.clip(base + rng.normal(0, 5, base.shape), 0, 255).astype(np.uint8)
        fg = ((yy - 20 - i) ** 2 + (xx - 25 - 2 * i) ** 2) < 90
        if i == 2:
            fg[:] = False
        noise = np.where(fg[..., None], 3.0, 12.0)                       # the background is degraded harder
        refs.append(r)
        decs.append(np.clip(r.astype(np.float64) + rng.normal(0, 1, r.shape) * noise, 0, 255).astype(np.uint8))
        fgs.append(fg)
    decs[5][fgs[5]] = refs[5][fgs[5]]                                      # an untouched foreground: PSNR 100, MSE 0
    bgs = [~m for m in fgs]
    apply = ref_elvis._apply_binary_mask
    results, indices = [], []
    for stride in STRIDES:
        result, idx, bbox, roi = core(refs, decs, fgs, bgs, EW, EH, stride, 0.0,
                                      [apply(f, m) for f, m in zip(refs, fgs)], [apply(f, m) for f, m in zip(decs, fgs)],
                                      [apply(f, m) for f, m in zip(refs, bgs)], [apply(f, m) for f, m in zip(decs, bgs)])
        results.append(Q.flatten_result(result))
        indices.append(idx)
    assert indices[1] == [0, 3, 6] and indices[0] == list(range(EN))
    out.update(eval_refs=np.stack(refs), eval_decs=np.stack(decs), eval_fg=np.stack(fgs).astype(np.uint8), eval_strides=np.asarray(STRIDES),
               eval_results=np.stack(results), eval_bbox=np.asarray(bbox, np.int32),
               eval_roi=np.asarray([roi[0].start, roi[0].stop, roi[1].start, roi[1].stop], np.int32))
    # the index rule alone, through the same compiled statements: (frames, stride) -> indices, -1 padded
    pairs = [(1, 1), (1, 4), (2, 5), (7, 1), (7, 2), (7, 3), (7, 6), (7, 7), (7, 100), (10, 3), (10, 9)]
    rows = []
    for count, stride in pairs:
        idx = core(refs[:1] * count, decs[:1] * count, fgs[:1] * count, bgs[:1] * count, EW, EH, stride, 0.0, *([[refs[0]] * count] * 4))[1]
        rows.append(idx + [-1] * (10 - len(idx)))
    out.update(index_pairs=np.asarray(pairs, np.int32), index_rows=np.asarray(rows, np.int32))

    path = os.path.join(make_golden.OUT, "quality.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
