"""Regenerate tests/golden/fvmd.npz from the reference's own `calculate_fvmd`.

    python tools/make_fvmd_golden.py   # needs the reference (ELVIS_REFERENCE, see oracle/make_golden.py)

What is pinned is the reference's control flow (elvis.py:3358-3597), run from its own code through
`oracle.make_golden.import_reference()`: `_build_indices`, the 10-frame minimum, the growing prefix in steps of
`early_stop_window`, the relative-delta early stop, the stride-halving fallback on `_FvmdNoTrajectories`, `_compute_std`
over windows of 10, and which exception ends a call that cannot be scored.

PARITY UNPINNED against the `fvmd` package itself: it is absent.  Its four imports (`VideoDataset`, `track_keypoints`,
`calc_hist`, `calculate_fd_given_vectors`), `cv2.imwrite` and the `torch.cuda` probes are replaced by recording stubs:
frames are 1 x 1 arrays holding their index, `cv2.imwrite` notes which index went to which clip directory, and the score
is `tests/_fvmd_ref.scripted_score(kind, indices)` of the rendered index list.

Only arguments, the index lists scored and the results are stored: per case `case<i>_args` = (frames, stride,
max_frames or 0, early_stop_delta, early_stop_window), `case<i>_script`, `case<i>_calls` int [calls, longest] padded with
-1, `case<i>_result` = (value, std) or NaNs, `case<i>_error` = the exception's class name or "".
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import make_golden  # noqa: E402
import _fvmd_ref as R  # noqa: E402

# (frames, stride, max_frames, early_stop_delta, early_stop_window, script)
CASES = (
    (120, 1, None, 0.002, 50, "converge"),       # early stop at the second prefix... or the third: whatever the reference does
    (120, 1, None, 0.05, 20, "converge"),        # early stop hit, then the std windows over the frames used
    (64, 1, None, 0.002, 25, "grow"),            # never hit: every prefix, the last one short
    (90, 3, None, 0.002, 50, "spread"),          # one prefix holds everything; the std windows differ
    (200, 2, 37, 0.002, 10, "grow"),             # max_frames cuts the index list
    (40, 8, None, 0.002, 50, "converge"),        # stride 8 yields 5 frames: sampling falls back 8 -> 4 -> 2
    (100, 4, None, 0.002, 50, "wide_fails"),     # the scorer gives up at stride 4 and 2, succeeds at 1
    (100, 4, 20, 0.002, 50, "wide_fails"),       # the same under max_frames
    (9, 1, None, 0.002, 50, "converge"),         # fewer than 10 frames: ValueError
    (9, 4, None, 0.002, 50, "converge"),         # the same, reached through the fallback
    (30, 1, None, 0.002, 5, "converge"),         # a first prefix of 5 frames cannot be scored, and stride 1 has no fallback
    (30, 2, None, 0.002, 5, "converge"),         # the same, after one fallback
    (12, 1, None, 0.002, 50, "spread"),          # three std windows
    (10, 1, None, 0.002, 50, "spread"),          # one std window: std 0
)


def run_reference(ref_elvis, case):
    frames, stride, max_frames, delta, window, script = case
    written = {}                                                            # clip directory -> indices rendered into it
    calls = []

    def imwrite(path, frame):
        written.setdefault(os.path.dirname(path), []).append(int(np.asarray(frame).reshape(-1)[0]))
        return True

    class VideoDataset:
        def __init__(self, root, seq_len, stride):
            assert stride == 1
            self.root, self.seq_len = root, seq_len

        def __len__(self):
            return 1

    def track_keypoints(log_dir, gen_dataset, gt_dataset, v_stride, S, device_ids):
        gt = written[os.path.join(gt_dataset.root, "clip_0001")]
        gen = written[os.path.join(gen_dataset.root, "clip_0001")]
        assert gt == gen and v_stride == 1 and S == gt_dataset.seq_len == max(10, min(16, len(gt))) and device_ids == [0]
        calls.append(list(gt))
        try:
            R.scripted_score(script, gt)                                    # the script's failures surface where the package's would
        except R.NoTrajectories as exc:
            raise RuntimeError(str(exc))
        row = np.asarray([gt], np.float64)
        return row, row, row, row

    ref_elvis.cv2.imwrite = imwrite
    ref_elvis.VideoDataset, ref_elvis.track_keypoints = VideoDataset, track_keypoints
    ref_elvis.calc_hist = lambda x: x
    ref_elvis.calculate_fd_given_vectors = lambda gt_hist, gen_hist: R.scripted_score(script, gt_hist[0, :gt_hist.shape[1] // 2].astype(int))
    cuda = ref_elvis.torch.cuda
    keep = cuda.is_available, cuda.device_count, cuda.set_device
    cuda.is_available, cuda.device_count, cuda.set_device = (lambda: True), (lambda: 1), (lambda d: None)
    clip = [np.full((1, 1), i, np.uint8) for i in range(frames)]
    try:
        result, error = ref_elvis.calculate_fvmd(clip, clip, None, stride, max_frames, delta, window, None, False), ""
    except (ValueError, RuntimeError) as exc:
        result, error = (float("nan"), float("nan")), type(exc).__name__
    finally:
        cuda.is_available, cuda.device_count, cuda.set_device = keep
    return calls, result, error


def main() -> None:
    ref_elvis, _ = make_golden.import_reference()
    out = {"cases": np.asarray(len(CASES))}
    for i, case in enumerate(CASES):
        calls, result, error = run_reference(ref_elvis, case)
        longest = max([len(c) for c in calls] + [1])
        out[f"case{i}_args"] = np.asarray([case[0], case[1], case[2] or 0, case[3], case[4]], np.float64)
        out[f"case{i}_script"] = np.asarray(case[5])
        out[f"case{i}_calls"] = np.asarray([c + [-1] * (longest - len(c)) for c in calls], np.int16).reshape(len(calls), longest)
        out[f"case{i}_result"] = np.asarray(result, np.float64)
        out[f"case{i}_error"] = np.asarray(error)
        print(case, "->", len(calls), "windows scored,", result, error)
    path = os.path.join(make_golden.OUT, "fvmd.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
