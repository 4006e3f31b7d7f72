"""Regenerate tests/golden/shrink.npz from the reference's own shrink / stretch functions.

    python tools/make_shrink_golden.py            # needs the reference (ELVIS_REFERENCE, see oracle/make_golden.py)

Only inputs and outputs are stored.  `elvis.py` and `utils.py` are imported at run time through
`oracle.make_golden.import_reference()`; `presley.py` runs an experiment on import, so its `stretch_video_frames`
is taken by parsing the file and compiling that one function.  Frames come from `tests/_shrink_ref.make_frame`
(blocks that can be told apart, yet compressible), scores from a seeded generator.  Cases per family: no removal,
whole passes only, a partial row pass, a partial column pass, a deep sequence (0.95), everything (k = Bx / 1.0);
block sizes 4, 8, 16; grids from 1x1 to 12x20; rows and columns beyond the block grid for the utils.py forms; tied
scores for the argmin forms, tie-free (asserted) for the top-k form; float32 and float64 scores.
"""
import ast
import os
import sys
from typing import Any, Callable, List, Tuple  # noqa: F401  (names the compiled Presley function's annotations use)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import make_golden  # noqa: E402
import _shrink_ref as R  # noqa: E402

# (blocks_y, blocks_x, block, amount, extra rows, extra columns, score dtype, tied scores)
ELVIS_CASES = [
    (1, 1, 8, 0.0, "f8"), (1, 1, 8, 1.0, "f8"), (3, 5, 4, 0.25, "f4"), (6, 10, 8, 0.33, "f8"), (6, 10, 8, 0.0, "f8"),
    (4, 7, 16, 3.0, "f4"), (5, 6, 4, 1.0, "f8"), (5, 6, 4, 9.0, "f8"), (12, 20, 4, 0.5, "f8"), (2, 16, 8, 0.95, "f4"),
]
PASS_CASES = [
    (1, 1, 8, 0.0, 0, 0, "f8", False), (1, 1, 8, 1.0, 3, 2, "f8", False), (1, 4, 4, 1.0, 0, 0, "f8", False),
    (4, 1, 4, 0.5, 0, 0, "f8", True), (6, 10, 8, 0.0, 0, 0, "f8", False), (6, 10, 8, 0.1, 0, 0, "f8", False),
    (6, 10, 8, 0.25, 5, 3, "f4", False), (6, 10, 8, 0.33, 0, 0, "f8", True), (6, 10, 8, 0.95, 1, 7, "f8", False),
    (5, 4, 16, 0.45, 0, 0, "f4", True), (5, 4, 16, 0.95, 0, 0, "f8", True), (3, 9, 4, 0.34, 2, 0, "f8", False),
    (12, 20, 4, 0.25, 0, 3, "f8", False), (12, 20, 4, 0.31, 0, 0, "f4", True), (7, 7, 4, 1.0, 0, 0, "f8", False),
    (9, 3, 8, 0.6, 0, 0, "f8", True),
]


def presley_stretch_video_frames():
    src = open(os.path.join(make_golden.REF, "presley.py")).read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "stretch_video_frames")
    ns = {"np": np, "List": List, "Tuple": Tuple, "Any": Any, "Callable": Callable}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "presley.py", "exec"), ns)
    return ns["stretch_video_frames"]


def scores_for(rng, by, bx, dtype, tied):
    if tied:
        s = rng.integers(0, 4, size=(by, bx)).astype(dtype) / 4
    else:
        s = rng.permutation(by * bx).reshape(by, bx).astype(dtype) / (by * bx) + dtype(0.001)
        assert all(len(np.unique(r)) == bx for r in s), "the top-k goldens need tie-free rows"
    return s


def flat(arrays, dtype):
    counts = np.array([len(a) for a in arrays], np.int32)
    return (np.concatenate([np.asarray(a, dtype) for a in arrays]) if len(arrays) else np.zeros(0, dtype)), counts


def main() -> None:
    ref_elvis, ref_utils = make_golden.import_reference()
    presley_stretch = presley_stretch_video_frames()
    rng = np.random.default_rng(20261016)
    out = {}
    n = 0

    def put(**kw):
        nonlocal n
        for k, v in kw.items():
            out[f"c{n}_{k}"] = np.asarray(v)
        n += 1

    for by, bx, b, amount, dt in ELVIS_CASES:
        dtype = np.dtype(dt).type
        frame = R.make_frame(by * b, bx * b, b, salt=n)
        scores = scores_for(rng, by, bx, dtype, False)
        keep_f, keep_s = frame.copy(), scores.copy()
        shrunk, mask, coords = ref_elvis.apply_selective_removal(frame, scores, b, amount)
        stretched = ref_elvis.stretch_frame(shrunk, mask, b)
        presley = presley_stretch([np.ascontiguousarray(shrunk)], [mask.astype(bool)], b)[0]
        assert np.array_equal(frame, keep_f) and np.array_equal(scores, keep_s)
        cf, cc = flat(coords, np.int64)
        put(family="elvis", block=b, amount=amount, frame=frame, scores=scores, shrunk=shrunk, mask=mask, coords_flat=cf,
            coords_counts=cc, stretched=stretched, stretched_presley=presley)

    for by, bx, b, amount, eh, ew, dt, tied in PASS_CASES:
        dtype = np.dtype(dt).type
        frame = R.make_frame(by * b + eh, bx * b + ew, b, salt=n)
        scores = scores_for(rng, by, bx, dtype, tied)
        keep_f, keep_s = frame.copy(), scores.copy()
        shrunk, mask = ref_utils.shrink_frame_row_only(frame, scores, b, amount)
        shrunk = np.ascontiguousarray(shrunk)
        put(family="row_only", block=b, amount=amount, frame=frame, scores=scores, shrunk=shrunk, mask=mask,
            stretched=ref_utils.stretch_frame_row_only(shrunk, mask, b),
            stretched_presley=presley_stretch([shrunk], [mask], b)[0])
        shrunk, mask, pmap = ref_utils.shrink_frame_position_map(frame, scores, b, amount)
        shrunk = np.ascontiguousarray(shrunk)
        shrunk2, mask2, ridx = ref_utils.shrink_frame_removal_indices(frame, scores, b, amount)
        assert np.array_equal(shrunk, shrunk2) and np.array_equal(mask, mask2)
        assert np.array_equal(frame, keep_f) and np.array_equal(scores, keep_s)
        rf, rc = flat(ridx, np.int32)
        assert all(a.dtype == np.int32 for a in ridx)
        put(family="position_map", block=b, amount=amount, frame=frame, scores=scores, shrunk=shrunk, mask=mask, posmap=pmap,
            ridx_flat=rf, ridx_counts=rc, stretched=ref_utils.stretch_frame_position_map(shrunk, mask, pmap, b),
            stretched_ridx=ref_utils.stretch_frame_removal_indices(shrunk, ridx, by, bx, b),
            stretched_presley=presley_stretch([shrunk], [mask], b)[0])

    out["n_cases"] = np.int64(n)
    path = os.path.join(make_golden.OUT, "shrink.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {n} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
