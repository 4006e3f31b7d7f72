"""Regenerate tests/golden/presley_degrade.npz from the reference's own adaptive degraders.

    python tools/make_presley_degrade_golden.py   # needs the reference (ELVIS_REFERENCE, see oracle/make_golden.py)

What is pinned is the map rule and the control flow, not pixels: `utils.degrade_adaptive_downsample` /
`degrade_adaptive_blur` are imported through `oracle.make_golden.import_reference()`; `presley.py` runs an experiment
on import, so its `generate_degradation_map`, `downscale_block`, `blur_block` and `degrade_frame` are taken by parsing
the file and compiling those functions.  cv2 is absent, so `cv2.resize` and `cv2.GaussianBlur` are replaced by
`tests/_presley_degrade_ref.Recorder`, which notes its arguments per block (target size, interpolation flag, kernel
size, sigma) and returns zeros of the right shape; frames are `id_frame`s, whose blocks name themselves.  Only the
importance inputs, the returned maps and the recorded numbers are stored (flat, case after case: `params` holds each
case's family, block, maximum, extra rows and columns, grid and importance item size).

Importance inputs, float32 and float64: values exactly on bin edges (k / max), exactly .5 after scaling (round-half-
even decides), 0 and 1, values one ulp either side of an edge, values outside [0, 1] (the clips), and seeded noise.
"""
import ast
import os
import sys
from typing import Any, Callable, List, Tuple  # noqa: F401  (names the compiled Presley functions' annotations use)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import make_golden  # noqa: E402
import _presley_degrade_ref as R  # noqa: E402

FAMILIES = ("utils_downsample", "utils_blur", "presley_downsample", "presley_blur")
PRESLEY_NAMES = ("generate_degradation_map", "downscale_block", "blur_block", "degrade_frame")
# (family, block, max value, extra rows, extra columns, importance dtype)
CASES = [
    ("utils_downsample", 16, 4, 0, 0, "f8"), ("utils_downsample", 16, 4, 8, 3, "f4"), ("utils_downsample", 12, 3, 7, 0, "f4"),
    ("utils_downsample", 4, 8, 1, 1, "f8"),
    ("utils_blur", 16, 10, 0, 0, "f8"), ("utils_blur", 8, 4, 0, 5, "f4"), ("utils_blur", 5, 7, 2, 0, "f4"),
    ("presley_downsample", 16, 4, 8, 3, "f8"), ("presley_downsample", 8, 10, 0, 5, "f4"), ("presley_downsample", 16, 20, 0, 0, "f4"),
    ("presley_blur", 16, 4, 0, 0, "f4"), ("presley_blur", 16, 10, 8, 3, "f8"), ("presley_blur", 3, 6, 1, 2, "f4"),
]


def presley_functions(cv2_stub):
    src = open(os.path.join(make_golden.REF, "presley.py")).read()
    fns = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in PRESLEY_NAMES]
    assert len(fns) == len(PRESLEY_NAMES)
    ns = {"np": np, "cv2": cv2_stub, "List": List, "Tuple": Tuple, "Any": Any, "Callable": Callable}
    exec(compile(ast.Module(body=fns, type_ignores=[]), "presley.py", "exec"), ns)
    return ns


def importance_values(rng, max_value: int, dtype) -> np.ndarray:
    k = np.arange(max_value + 1, dtype=np.float64)
    edges = 1.0 - k / max_value                                  # (1 - v) * max is a whole number
    halves = 1.0 - (k[:-1] + 0.5) / max_value                    # ... is exactly .5 past one
    vals = np.concatenate([edges, halves, [0.0, 1.0, -0.25, 1.25], rng.random(4)]).astype(dtype)
    near = np.concatenate([np.nextafter(vals[:len(edges) + len(halves)], dtype(2)),
                           np.nextafter(vals[:len(edges) + len(halves)], dtype(-1))])
    return np.concatenate([vals, near]).astype(dtype)


def main() -> None:
    _, ref_utils = make_golden.import_reference()
    cv2_stub = sys.modules["cv2"]
    assert not hasattr(cv2_stub, "GaussianBlur"), "a real cv2 is installed: record pixels, not control flow"
    cv2_stub.INTER_LINEAR, cv2_stub.INTER_AREA = R.INTER_LINEAR, R.INTER_AREA
    presley = presley_functions(cv2_stub)
    rng = np.random.default_rng(20261017)
    params, records, scores, kernels = [], [], {"f4": [], "f8": []}, set()
    for family, b, max_value, eh, ew, dt in CASES:
        dtype = np.dtype(dt).type
        vals = importance_values(rng, max_value, dtype)
        bx = 6
        by = -(-len(vals) // bx)
        importance = np.concatenate([vals, rng.random(by * bx - len(vals)).astype(dtype)]).reshape(by, bx)
        assert importance.dtype == dtype
        frame = R.id_frame(by * b + eh, bx * b + ew, b)
        rec = R.Recorder(by, bx)
        cv2_stub.resize, cv2_stub.GaussianBlur = rec.resize, rec.GaussianBlur
        keep_f, keep_i = frame.copy(), importance.copy()
        if family == "utils_downsample":
            degraded, dmap = ref_utils.degrade_adaptive_downsample(frame, importance, b, max_value)
        elif family == "utils_blur":
            degraded, dmap = ref_utils.degrade_adaptive_blur(frame, importance, b, max_value)
        else:
            dmap = presley["generate_degradation_map"](importance, max_value)
            method = presley["downscale_block" if family == "presley_downsample" else "blur_block"]
            degraded = presley["degrade_frame"](frame, dmap, b, method)
        assert np.array_equal(frame, keep_f) and np.array_equal(importance, keep_i)
        assert degraded.shape == frame.shape and dmap.dtype == np.int32 and dmap.shape == (by, bx)
        # the stand-ins return zeros: a block is black exactly where a call replaced it, all else is the input
        touched = (rec.resizes + rec.blurs) > 0
        expect = frame.copy()
        for i, j in zip(*np.nonzero(touched)):
            expect[i * b:(i + 1) * b, j * b:(j + 1) * b] = 0
        assert np.array_equal(degraded, expect)
        kernels |= rec.kernels
        # per block: map value, touched, first and second resize (size, flag), resize calls, blur calls
        record = np.concatenate([dmap[..., None], touched[..., None], rec.sizes[..., :1], rec.flags[..., :1], rec.sizes[..., 1:],
                                 rec.flags[..., 1:], rec.resizes[..., None], rec.blurs[..., None]], axis=-1).astype(np.int32)
        params.append((FAMILIES.index(family), b, max_value, eh, ew, by, bx, dtype().itemsize))
        records.append(record.reshape(-1, 8))
        scores[dt].append(importance.reshape(-1))
    out = dict(families=np.asarray(FAMILIES), params=np.asarray(params, np.int32), records=np.concatenate(records),
               importance_f4=np.concatenate(scores["f4"]), importance_f8=np.concatenate(scores["f8"]),
               kernels=np.asarray(sorted(kernels), np.float64).reshape(-1, 3))
    path = os.path.join(make_golden.OUT, "presley_degrade.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(CASES)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
