"""Regenerate tests/golden/removability.npz from the reference's own `calculate_removability_scores` (elvis.py:968-1224).

    python tools/make_removability_golden.py   # needs the reference (ELVIS_REFERENCE, see oracle/make_golden.py)

`elvis.py` is imported through `oracle.make_golden.import_reference()` and the function is run as it is.  The outside
world it reaches for is absent here (EVCA, UFO, cv2) and is stubbed for the run:
  - a fake `evca` module in `sys.modules` whose `__file__` lies in a temporary directory;
  - `subprocess.run` replaced by a function that, for the EVCA command, writes `evca_SC_blocks.csv` and
    `evca_TC_blocks.csv` there - a header line, then one row per block and one column per frame, `%.17g` (float64 reads
    back exactly) - and, for the UFO command, creates the empty mask files `00001.png ...` of the case; both return 0;
  - `cv2.imread` answered from the case's mask arrays by file name, `cv2.resize` by the nearest rule
    (source index floor(dst * src_n / dst_n)).
What is pinned is therefore everything the function does with the two maps and the masks - both `normalize_array`
calls and their `max > min` guard, the alpha mix, the x10 on background blocks, the smoothing from the unsmoothed
previous frame - not EVCA's or UFO's pixels and not cv2's resize.  Only inputs and the produced arrays are stored (flat,
case after case; `params` holds each case's shape and settings).

Cases: F = 2 and 3 (np.loadtxt needs two columns); alpha 0, 0.5 and 1; smoothing_beta 1 and 0.5; masks all foreground,
all background and mixed (values 0, 1, 128, 255), at a size that is no multiple of the grid; one frame without a mask
file; flat clips, where the `max > min` guards decide.
"""
import contextlib
import io
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden  # noqa: E402

BLOCK = 16
# (F, By, Bx, alpha, smoothing_beta, masks, frame without a mask file or -1, flat clip)
CASES = [
    (2, 2, 3, 0.5, 1, "mixed", -1, 0),
    (3, 3, 4, 0.5, 0.5, "mixed", -1, 0),
    (3, 2, 3, 0.0, 1, "foreground", -1, 0),
    (3, 2, 3, 1.0, 0.5, "background", -1, 0),
    (2, 3, 2, 0.0, 0.5, "mixed", 1, 0),
    (3, 2, 2, 0.5, 1, "mixed", 0, 0),
    (3, 4, 3, 0.25, 0.75, "mixed", 2, 0),
    (2, 2, 3, 0.5, 1, "foreground", -1, 1),
    (3, 2, 3, 1.0, 0.5, "mixed", -1, 1),
    (2, 2, 2, 0.5, 0.5, "background", -1, 1),
]


def nearest(mask: np.ndarray, size, interpolation=None) -> np.ndarray:
    cols, rows = size
    ys = (np.arange(rows, dtype=np.int64) * mask.shape[0]) // rows
    xs = (np.arange(cols, dtype=np.int64) * mask.shape[1]) // cols
    return mask[ys][:, xs]


def make_masks(rng, kind: str, count: int, rows: int, cols: int) -> np.ndarray:
    if kind == "foreground":
        return rng.choice(np.asarray([1, 128, 255], np.uint8), size=(count, rows, cols))
    if kind == "background":
        return np.zeros((count, rows, cols), np.uint8)
    return rng.choice(np.asarray([0, 0, 1, 128, 255], np.uint8), size=(count, rows, cols))


def run_case(ref_elvis, rng, case):
    count, by, bx, alpha, beta, kind, missing, flat = case
    spatial, temporal = rng.random((count, by, bx)), rng.random((count, by, bx))
    if flat:
        spatial[:], temporal[:] = 0.25, 0.25                  # the first two guards return the maps as they are
    rows, cols = 3 * by + 1, 2 * bx + 1                         # no multiple of the grid in either axis
    masks = make_masks(rng, kind, count, rows, cols)
    keep = [a.copy() for a in (spatial, temporal, masks)]
    width, height = bx * BLOCK + 5, by * BLOCK + 3              # the remainder is floored away (elvis.py:1163-1164)
    cv2_stub = sys.modules["cv2"]
    with tempfile.TemporaryDirectory() as tmp:
        package, work, frames_dir = (os.path.join(tmp, d) for d in ("evca_package", "work", "frames"))
        for d in (package, work, frames_dir):
            os.makedirs(d)
        for i in range(count):
            open(os.path.join(frames_dir, f"{i + 1:05d}.png"), "wb").close()
        evca = types.ModuleType("evca")
        evca.__file__ = os.path.join(package, "__init__.py")
        masks_dir = os.path.join(work, "maps", "ufo_masks")
        calls = []

        def fake_run(cmd, *args, **kwargs):
            if isinstance(cmd, (list, tuple)) and "evca.main" in cmd:
                assert cmd[cmd.index("-b") + 1] == str(BLOCK) and cmd[cmd.index("-f") + 1] == str(count)
                assert cmd[cmd.index("-r") + 1] == f"{width}x{height}"
                header = ",".join(f"frame{i}" for i in range(count))
                for name, maps in (("evca_SC_blocks.csv", spatial), ("evca_TC_blocks.csv", temporal)):
                    np.savetxt(os.path.join(package, name), maps.reshape(count, by * bx).T, fmt="%.17g", delimiter=",",
                               header=header, comments="")
                calls.append("evca")
            else:
                assert "ufo.test" in cmd and masks_dir in cmd
                for i in range(count):
                    if i != missing:
                        open(os.path.join(masks_dir, f"{i + 1:05d}.png"), "wb").close()
                calls.append("ufo")
            return types.SimpleNamespace(returncode=0, stdout="", stderr="")

        def fake_imread(path, flags=None):
            assert os.path.dirname(path) == masks_dir and flags == cv2_stub.IMREAD_GRAYSCALE
            index = int(os.path.splitext(os.path.basename(path))[0]) - 1
            assert index != missing
            return masks[index]

        real_run, had_evca = subprocess.run, sys.modules.get("evca")
        cv2_stub.imread, cv2_stub.resize = fake_imread, nearest
        cv2_stub.IMREAD_GRAYSCALE, cv2_stub.INTER_NEAREST = 0, 0
        subprocess.run, sys.modules["evca"] = fake_run, evca
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                scores = ref_elvis.calculate_removability_scores(os.path.join(tmp, "raw.yuv"), frames_dir, width, height, BLOCK,
                                                                 alpha=alpha, working_dir=work, smoothing_beta=beta)
        finally:
            subprocess.run = real_run
            if had_evca is None:
                del sys.modules["evca"]
            else:
                sys.modules["evca"] = had_evca
    assert calls == ["evca", "ufo"], calls
    assert all(np.array_equal(a, b) for a, b in zip(keep, (spatial, temporal, masks)))
    assert scores.dtype == np.float64 and scores.shape == (count, by, bx)
    return spatial, temporal, masks, scores


def main() -> None:
    ref_elvis, _ = make_golden.import_reference()
    assert not hasattr(sys.modules["cv2"], "cvtColor"), "a real cv2 is installed: let it resize the masks instead"
    rng = np.random.default_rng(20261019)
    params, settings = [], []
    flat = {k: [] for k in ("spatial", "temporal", "masks", "scores")}
    for case in CASES:
        count, by, bx, alpha, beta, kind, missing, is_flat = case
        spatial, temporal, masks, scores = run_case(ref_elvis, rng, case)
        if is_flat and kind != "mixed":                          # nothing gives the clip a spread: the last guard returns it as it is
            assert np.ptp(scores) == 0 and scores.flat[0] != 0
        else:
            assert scores.min() == 0 and scores.max() == 1
        params.append((count, by, bx, masks.shape[1], masks.shape[2], missing))
        settings.append((alpha, beta))
        for k, a in (("spatial", spatial), ("temporal", temporal), ("masks", masks), ("scores", scores)):
            flat[k].append(a.reshape(-1))
    out = {"params": np.asarray(params, np.int32), "alpha_beta": np.asarray(settings, np.float64)}
    out.update({k: np.concatenate(v) for k, v in flat.items()})
    target = os.path.join(make_golden.OUT, "removability.npz")
    np.savez_compressed(target, **out)
    print(f"{target}: {os.path.getsize(target)} bytes")


if __name__ == "__main__":
    main()
