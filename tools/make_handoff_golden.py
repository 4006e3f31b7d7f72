"""Regenerate tests/golden/handoff.npz from the reference's own hand-off functions.

    python tools/make_handoff_golden.py   # needs the reference (ELVIS_REFERENCE, see oracle/make_golden.py)

`utils.py` is imported through `oracle.make_golden.import_reference()` and its `calculate_importance_scores`,
`create_kvazaar_roi_file`, `create_svtav1_roi_file` and `write_y4m` are run as they are.  cv2 is absent, so the two cv2
calls they make are answered by `tests/_handoff_ref.CvStub`: `cv2.resize` by the restated float INTER_AREA and
`cv2.cvtColor` by the restated planes (the codes it is asked for are recorded).  What is pinned is therefore the
importance arithmetic, the delta-QP rules, both file formats and the Y4M framing - not OpenCV's pixels.  Only the inputs
and the produced arrays / file bytes are stored (flat, case after case; `*_params` holds each case's shape and settings).

Inputs, float32 and float64.  Importance rule: F = 1, 2 and 3; masks of 0, 0.49999, 0.5 and 1; one frame of constant
complexity (the + 1e-8 decides).  Kvazaar: importances that put the delta exactly on +-14 for qp_range 15 and 20, one ulp
either side, on the .5 steps, 0 and 1, noise; base_qp 5, 30 and 48 (the HEVC clip bites at both ends).  SVT-AV1: a whole
ratio (32 x 64 blocks of 16 -> 8 x 16) and the ragged 1080p grid (67 x 120 -> 17 x 30); every grid keeps 8 * resized at
least 1e-4 from a whole number (asserted), so the unpinned resize cannot move a level.
"""
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import make_golden  # noqa: E402
import _handoff_ref as R  # noqa: E402

MARGIN = 1e-4
FRAMERATES = (30, 29.97, 23.976)
# (F, By, Bx, alpha, beta, dtype, frame 0 flat)
IMPORTANCE_CASES = [(1, 3, 4, 0.5, 0.5, "f4", 0), (1, 3, 4, 0.5, 0.5, "f4", 1), (2, 3, 4, 0.5, 0.5, "f4", 1), (2, 4, 5, 0.7, 0.3, "f8", 0),
                    (3, 4, 5, 0.25, 0.9, "f4", 0), (1, 2, 6, 1.0, 0.0, "f8", 1), (3, 3, 3, 0.0, 1.0, "f8", 1)]
# (base_qp, qp_range, dtype)
KVAZAAR_CASES = [(5, 15, "f4"), (30, 15, "f4"), (48, 15, "f4"), (5, 15, "f8"), (30, 15, "f8"), (48, 15, "f8"), (30, 20, "f8"),
                 (30, 10, "f4")]
# (By, Bx, width, height, base_crf, qp_range, F, dtype)
SVTAV1_CASES = [(32, 64, 1024, 512, 35, 15, 2, "f4"), (32, 64, 1024, 512, 60, 20, 1, "f8"), (67, 120, 1920, 1080, 35, 15, 2, "f4"),
                (67, 120, 1920, 1080, 5, 15, 1, "f8")]


def kvazaar_values(rng, qp_range: int, dtype) -> np.ndarray:
    on_limit = [0.5 - 14 / (2 * qp_range), 0.5 + 14 / (2 * qp_range)]
    steps = [1.0 - (k + 0.5 + qp_range) / (2 * qp_range) for k in range(-qp_range, qp_range)]      # delta = k + .5
    whole = [1.0 - (k + qp_range) / (2 * qp_range) for k in range(-qp_range, qp_range + 1)]        # delta = k
    vals = np.asarray(on_limit + steps + whole + [0.0, 1.0], np.float64).astype(dtype)
    near = np.concatenate([np.nextafter(vals, dtype(2)), np.nextafter(vals, dtype(-1))])
    return np.concatenate([vals, near, rng.random(8).astype(dtype)]).astype(dtype)


def svtav1_grid(seed: int, by: int, bx: int, width: int, height: int, dtype) -> np.ndarray:
    """A diagonal ramp plus seeded steps, on the nine values (k + 0.37) / 9 (few distinct values keep the fixture
    small); the first of 64 seeds whose levels all keep the margin."""
    yy, xx = np.mgrid[:by, :bx]
    for s in range(seed, seed + 64):
        k = np.clip(np.rint(4 * (yy / by + xx / bx)) + np.random.default_rng(s).integers(-1, 2, (by, bx)), 0, 8)
        grid = ((k + 0.37) / 9).astype(dtype)
        if R.svtav1_levels_margin(grid, width, height) >= MARGIN:
            return grid
    raise AssertionError("no grid keeps 8 * resized clear of a whole number")


def main() -> None:
    _, ref_utils = make_golden.import_reference()
    cv2_stub = sys.modules["cv2"]
    assert not hasattr(cv2_stub, "cvtColor"), "a real cv2 is installed: record its pixels instead"
    stub = R.CvStub()
    cv2_stub.resize, cv2_stub.cvtColor, cv2_stub.INTER_AREA = stub.resize, stub.cvtColor, R.INTER_AREA
    cv2_stub.COLOR_RGB2YUV_I420, cv2_stub.COLOR_BGR2YUV_I420 = R.COLOR_RGB2YUV_I420, R.COLOR_BGR2YUV_I420
    rng = np.random.default_rng(20261018)
    out = {}
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "artefact")

    # ---- calculate_importance_scores
    params, flat = [], {k: {"f4": [], "f8": []} for k in ("sc", "tc", "mask", "score")}
    for count, by, bx, alpha, beta, dt, flat0 in IMPORTANCE_CASES:
        sc, tc = rng.random((count, by, bx)).astype(dt), rng.random((count, by, bx)).astype(dt)
        masks = rng.choice(np.asarray([0.0, 0.49999, 0.5, 1.0]), size=(count, by, bx)).astype(dt)
        masks[-1].reshape(-1)[:4] = [0.0, 0.49999, 0.5, 1.0]
        if flat0:                                                   # frame 0 is one value everywhere: the + 1e-8 decides
            sc[0], tc[min(1, count - 1)], masks[0] = 0.25, 0.75, 1.0
        keep = [a.copy() for a in (sc, tc, masks)]
        scores = ref_utils.calculate_importance_scores(None, 16, alpha, beta, SimpleNamespace(SC=sc, TC=tc), masks)
        assert all(np.array_equal(a, b) for a, b in zip(keep, (sc, tc, masks)))
        scores = np.stack(scores)
        assert scores.dtype == np.dtype(dt) and scores.shape == sc.shape
        assert not flat0 or (np.ptp(scores[0]) == 0 and scores[0].flat[0] == 0)
        params.append((count, by, bx, np.dtype(dt).itemsize))
        out.setdefault("importance_alpha_beta", []).append((alpha, beta))
        for k, a in (("sc", sc), ("tc", tc), ("mask", masks), ("score", scores)):
            flat[k][dt].append(a.reshape(-1))
    out["importance_params"] = np.asarray(params, np.int32)
    out["importance_alpha_beta"] = np.asarray(out["importance_alpha_beta"], np.float64)
    for k, by_dtype in flat.items():
        for dt, parts in by_dtype.items():
            out[f"importance_{k}_{dt}"] = np.concatenate(parts)

    # ---- create_kvazaar_roi_file
    params, inputs, files = [], {"f4": [], "f8": []}, []
    for base_qp, qp_range, dt in KVAZAAR_CASES:
        vals = kvazaar_values(rng, qp_range, np.dtype(dt).type)
        bx = 7
        by = -(-len(vals) // bx)
        frame0 = np.concatenate([vals, rng.random(by * bx - len(vals)).astype(dt)]).reshape(by, bx)
        frame1 = rng.random((2, 3)).astype(dt)                      # a file's frames need not share a grid
        ref_utils.create_kvazaar_roi_file([frame0, frame1], path, base_qp, qp_range)
        data = np.frombuffer(open(path, "rb").read(), np.uint8)
        assert data.size == 8 + by * bx + 8 + 6
        params.append((base_qp, qp_range, by, bx, np.dtype(dt).itemsize, data.size))
        inputs[dt] += [frame0.reshape(-1), frame1.reshape(-1)]
        files.append(data)
    out["kvazaar_params"] = np.asarray(params, np.int32)
    out["kvazaar_importance_f4"], out["kvazaar_importance_f8"] = np.concatenate(inputs["f4"]), np.concatenate(inputs["f8"])
    out["kvazaar_files"] = np.concatenate(files)

    # ---- create_svtav1_roi_file
    params, inputs, files = [], {"f4": [], "f8": []}, []
    for k, (by, bx, width, height, base_crf, qp_range, count, dt) in enumerate(SVTAV1_CASES):
        grids = [svtav1_grid(1000 * k + 100 * f, by, bx, width, height, np.dtype(dt).type) for f in range(count)]
        for g in grids:
            assert R.svtav1_levels_margin(g, width, height) >= MARGIN
        ref_utils.create_svtav1_roi_file(grids, path, base_crf, qp_range, width, height)
        data = np.frombuffer(open(path, "rb").read(), np.uint8)
        params.append((by, bx, width, height, base_crf, qp_range, count, np.dtype(dt).itemsize, data.size))
        inputs[dt] += [g.reshape(-1) for g in grids]
        files.append(data)
    out["svtav1_params"] = np.asarray(params, np.int32)
    out["svtav1_importance_f4"], out["svtav1_importance_f8"] = np.concatenate(inputs["f4"]), np.concatenate(inputs["f8"])
    out["svtav1_files"] = np.concatenate(files)

    # ---- write_y4m
    frames = [rng.integers(0, 256, (6, 10, 3), dtype=np.uint8) for _ in range(3)]
    sizes, files = [], []
    for rate in FRAMERATES:
        stub.codes.clear()
        ref_utils.write_y4m(frames, path, rate)
        assert stub.codes == [R.COLOR_RGB2YUV_I420] * len(frames)
        data = np.frombuffer(open(path, "rb").read(), np.uint8)
        sizes.append(data.size)
        files.append(data)
    out["y4m_frames"], out["y4m_framerates"] = np.stack(frames), np.asarray(FRAMERATES, np.float64)
    out["y4m_sizes"], out["y4m_files"] = np.asarray(sizes, np.int32), np.concatenate(files)

    os.remove(path)
    os.rmdir(tmp)
    target = os.path.join(make_golden.OUT, "handoff.npz")
    np.savez_compressed(target, **out)
    print(f"{target}: {os.path.getsize(target)} bytes")


if __name__ == "__main__":
    main()
