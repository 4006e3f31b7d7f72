"""FVMD of the evaluation report on the device.

The reference computes FVMD by writing both clips to disk as PNG files and handing them to the `fvmd` package:
`calculate_fvmd` (elvis.py:3358-3597, called twice per evaluated video at elvis.py:4009-4030) builds a `VideoDataset`,
calls `track_keypoints`, `calc_hist` and `calculate_fd_given_vectors` (elvis.py:3476-3505).

BUILD-DEFINED: the `fvmd` package is available neither to the reference tree nor to this build.  Its tracker (PIPs++, a
network), its `calc_hist` and its `VideoDataset` semantics cannot be read.  This is a restatement of the *published
form* - tracks -> velocity / acceleration -> cell orientation histograms -> Frechet distance - on the device
(csrc/fvmd.hip), with a classical pyramidal Lucas-Kanade (KLT) tracker in the network's place.
It does NOT claim parity with the `fvmd` package; its values are not comparable with published FVMD numbers.
The contract is the one of include/elvis_amd.h and DESIGN.md 7.
PINNED against: its own numpy float64 statement, tests/_fvmd_ref.py (1e-9 * max(1, |value|) per stage), and - for the
control flow of `calculate_fvmd` only - the reference's own code, run with recording stubs (tools/make_fvmd_golden.py,
tests/golden/fvmd.npz): `_build_indices`, the 10-frame minimum, the growing prefix in steps of `early_stop_window`, the
relative-delta early stop, the stride-halving fallback on `FvmdNoTrajectories`, `_compute_std` over windows of 10.
DEPARTURES: nothing is written to disk and `log_root` is ignored.  A window that yields fewer than two segments raises
`FvmdNoTrajectories` (the reference's behaviour there depends on the absent package); `_compute_std`'s windows hold 10
frames, which is one segment of S = 10 whatever `segment_step` is, so they contribute nothing and the std is 0.0.  A
prefix's segments are a prefix of the whole clip's segments while S is the same, so a clip is tracked ONCE per sampling
stride and each prefix's score is a Frechet distance over the first rows: the result equals tracking each prefix afresh.
`segment_step` is this build's reading of `VideoDataset(..., stride=1)`.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib, ptr
from .ops import _s

MIN_SIDE = 64
MIN_REQUIRED_FRAMES = 10           # elvis.py:3423
MAX_SEQ_LEN = 16                   # elvis.py:3452
POINTS = 400
FIELD_VALUES = 128                 # 16 cells x 8 bins
MAX_ROWS = 1024                    # the most segments of one clip a Frechet distance takes (FVMD_MAX_ROWS)


class FvmdNoTrajectories(RuntimeError):
    """The build's `_FvmdNoTrajectories` (elvis.py:3396): a window that cannot be scored; `calculate_fvmd` answers it by
    halving the sampling stride."""


@dataclass(frozen=True)
class FvmdConfig:
    """The constants of the contract (fixed in csrc/fvmd.hip; here for the record and for `segment_step`) and the
    evaluation settings of the reference's `ElvisConfig` (elvis.py:95-99).  BUILD-DEFINED (module docstring).
    `segment_step`: a clip's sliding segments start every `segment_step` frames - this build's reading of
    `VideoDataset(..., stride=1)`; raise it to keep a long clip under `MAX_ROWS` segments."""
    segment_step: int = 1
    grid: int = 20
    pyramid_levels: int = 3
    window_radius: int = 7
    iterations: int = 8
    min_eigenvalue: float = 1e-3
    cells: int = 4
    bins: int = 8
    stride: int = 1                           # fvmd_stride
    max_frames: Optional[int] = None          # fvmd_max_frames
    early_stop_delta: float = 0.002           # fvmd_early_stop_delta
    early_stop_window: int = 50               # fvmd_early_stop_window

    def __post_init__(self):
        if int(self.segment_step) < 1:
            raise ValueError("fvmd: segment_step must be at least 1")
        fixed = FvmdConfig.__dataclass_fields__
        for name in ("grid", "pyramid_levels", "window_radius", "iterations", "min_eigenvalue", "cells", "bins"):
            if getattr(self, name) != fixed[name].default:
                raise ValueError(f"fvmd: {name} is a constant of the contract ({fixed[name].default}); the kernels are built for it")


def clip_seq_len(frames: int) -> int:
    """elvis.py:3452: the segment length for a window of `frames` sampled frames."""
    return max(MIN_REQUIRED_FRAMES, min(MAX_SEQ_LEN, int(frames)))


def segment_count(frames: int, seq_len: int, segment_step: int = 1) -> int:
    return 0 if frames < seq_len else (frames - seq_len) // segment_step + 1


def feature_length(seq_len: int) -> int:
    return (2 * seq_len - 3) * FIELD_VALUES


# ----------------------------------------------------------------------------- the device form
def _chk_luma(t, who):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3:
        raise ValueError(f"fvmd: {who} must be a uint8 tensor [F, H, W]")
    if t.shape[1] < MIN_SIDE or t.shape[2] < MIN_SIDE:
        raise ValueError(f"fvmd: a {t.shape[1]} x {t.shape[2]} plane is smaller than {MIN_SIDE} x {MIN_SIDE}")
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"fvmd: {who} must be a contiguous CUDA uint8 tensor [F, H, W]")


def _chk_f64(t, who, dims):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != dims:
        raise ValueError(f"fvmd: {who} must be a float64 tensor of {dims} dimensions")
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"fvmd: {who} must be a contiguous CUDA float64 tensor")


def pyramid_device(luma_d: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """u8 [F,H,W] -> the float64 pyramid levels 1 and 2, [F,(H+1)//2,(W+1)//2] and the same again (views of one
    allocation; level 0 is the luma itself).  BUILD-DEFINED."""
    _chk_luma(luma_d, "luma")
    f, h, w = luma_d.shape
    h1, w1 = (h + 1) // 2, (w + 1) // 2
    h2, w2 = (h1 + 1) // 2, (w1 + 1) // 2
    if f == 0:
        return luma_d.new_empty((0, h1, w1), dtype=torch.float64), luma_d.new_empty((0, h2, w2), dtype=torch.float64)
    nbytes = lib().elvis_fvmd_pyramid_bytes(f, h, w)
    if nbytes == 0:
        raise ValueError(f"fvmd: {f} frames of {h} x {w} are more than one call holds")
    with torch.cuda.device(luma_d.device):
        pyr = torch.empty(nbytes // 8, dtype=torch.float64, device=luma_d.device)
        check(lib().elvis_fvmd_pyramid_f64(ptr(luma_d), ptr(pyr), f, h, w, _s(luma_d)), luma_d.device)
    return pyr[:f * h1 * w1].view(f, h1, w1), pyr[f * h1 * w1:].view(f, h2, w2)


def track_keypoints_device(luma_d: torch.Tensor, seq_len: int, cfg: Optional[FvmdConfig] = None) -> torch.Tensor:
    """elvis.py:3476-3483 (`track_keypoints`) in this build's form: u8 [F,H,W] luma on the device, H, W >= 64 ->
    float64 [B, seq_len, 400, 2] = (x, y) of the 20 x 20 keypoints of every sliding segment, B = (F - seq_len) //
    segment_step + 1, each segment tracked from a fresh grid by the pyramidal Lucas-Kanade step of the contract.  A clip
    shorter than one segment gives B = 0.  BUILD-DEFINED (module docstring): it does NOT claim parity with the package's
    PIPs++ tracker."""
    cfg = cfg or FvmdConfig()
    _chk_luma(luma_d, "luma")
    seq_len = int(seq_len)
    if not MIN_REQUIRED_FRAMES <= seq_len <= MAX_SEQ_LEN:
        raise ValueError(f"fvmd: seq_len {seq_len} outside [{MIN_REQUIRED_FRAMES}, {MAX_SEQ_LEN}]")
    f, h, w = luma_d.shape
    b = segment_count(f, seq_len, cfg.segment_step)
    tracks = torch.empty((b, seq_len, POINTS, 2), dtype=torch.float64, device=luma_d.device)
    if b == 0:
        return tracks
    if b > 65535:
        raise ValueError(f"fvmd: {b} segments are more than one call holds; raise segment_step")
    lvl1, _ = pyramid_device(luma_d)                                   # level 2 follows level 1 in the same allocation
    with torch.cuda.device(luma_d.device):
        check(lib().elvis_fvmd_track_f64(ptr(luma_d), lvl1.data_ptr(), ptr(tracks), f, h, w, seq_len, int(cfg.segment_step), _s(luma_d)),
              luma_d.device)
    return tracks


def motion_features_device(tracks: torch.Tensor) -> torch.Tensor:
    """elvis.py:3494-3503 (`calc_hist` of velocities and accelerations, concatenated) in this build's form: float64
    [B,S,400,2] -> [B, (2 S - 3) 128], the soft orientation histograms of the S - 1 velocity fields, then of the S - 2
    acceleration fields, unnormalised.  BUILD-DEFINED."""
    _chk_f64(tracks, "tracks", 4)
    b, s = tracks.shape[:2]
    if tuple(tracks.shape[2:]) != (POINTS, 2) or not MIN_REQUIRED_FRAMES <= s <= MAX_SEQ_LEN:
        raise ValueError(f"fvmd: tracks must be [B, S, {POINTS}, 2] with {MIN_REQUIRED_FRAMES} <= S <= {MAX_SEQ_LEN}")
    rows = torch.empty((b, feature_length(s)), dtype=torch.float64, device=tracks.device)
    if b:
        with torch.cuda.device(tracks.device):
            check(lib().elvis_fvmd_features_f64(ptr(tracks), ptr(rows), b, s, _s(tracks)), tracks.device)
    return rows


def _chk_rows(rows_a, rows_b):
    _chk_f64(rows_a, "rows_a", 2)
    _chk_f64(rows_b, "rows_b", 2)
    if rows_a.shape[1] != rows_b.shape[1] or rows_a.shape[1] < 1 or rows_a.device != rows_b.device:
        raise ValueError("fvmd: the two sets of rows must be [n, d] and [m, d] on one device")
    n, m = rows_a.shape[0], rows_b.shape[0]
    if n < 2 or m < 2:
        raise FvmdNoTrajectories(f"fvmd: {n} and {m} feature rows; a Frechet distance needs at least two of each")
    if n > MAX_ROWS or m > MAX_ROWS:
        raise ValueError(f"fvmd: {max(n, m)} segments are more than the {MAX_ROWS} a Frechet distance takes; raise segment_step")
    return n, m, rows_a.shape[1]


def gram_device(rows_a: torch.Tensor, rows_b: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """float64 [n,d], [m,d] -> (the centred A Bm^T [n,m], [|mu_A - mu_B|^2, |A|_F^2, |Bm|_F^2])."""
    n, m, d = _chk_rows(rows_a, rows_b)
    dev = rows_a.device
    with torch.cuda.device(dev):
        ws = torch.empty(lib().elvis_fvmd_gram_workspace_bytes(n, m, d) // 8, dtype=torch.float64, device=dev)
        gram = torch.empty((n, m), dtype=torch.float64, device=dev)
        scalars = torch.empty(3, dtype=torch.float64, device=dev)
        check(lib().elvis_fvmd_gram_f64(ptr(rows_a), ptr(rows_b), ptr(ws), ptr(gram), ptr(scalars), n, m, d, _s(rows_a)), dev)
    return gram, scalars


def singular_values_device(matrix: torch.Tensor) -> torch.Tensor:
    """float64 [k,len] -> its k singular values (those past min(k, len) are 0 to rounding), unsorted, by one-sided
    Jacobi on the device; the matrix is left as it is (a copy is rotated).  k, len <= MAX_ROWS."""
    _chk_f64(matrix, "matrix", 2)
    k, ln = matrix.shape
    if k < 1 or ln < 1 or k > MAX_ROWS or ln > MAX_ROWS:
        raise ValueError(f"fvmd: a {k} x {ln} matrix is outside 1 .. {MAX_ROWS}; raise segment_step")
    with torch.cuda.device(matrix.device):
        work = matrix.clone()
        sv = torch.empty(k, dtype=torch.float64, device=matrix.device)
        check(lib().elvis_fvmd_singular_values_f64(ptr(work), ptr(sv), k, ln, _s(matrix)), matrix.device)
    return sv


def _frechet_tensor(rows_a: torch.Tensor, rows_b: torch.Tensor) -> torch.Tensor:
    n, m, _ = _chk_rows(rows_a, rows_b)
    if n > m:                                                            # |A Bm^T|_* = |Bm A^T|_*: rotate the fewer vectors
        rows_a, rows_b, n, m = rows_b, rows_a, m, n
    gram, scalars = gram_device(rows_a, rows_b)
    sv = singular_values_device(gram)
    out = torch.empty(1, dtype=torch.float64, device=rows_a.device)
    with torch.cuda.device(rows_a.device):
        check(lib().elvis_fvmd_finish_f64(ptr(sv), ptr(scalars), ptr(out), n, n, m, _s(rows_a)), rows_a.device)
    return out


def frechet_distance_device(rows_a: torch.Tensor, rows_b: torch.Tensor) -> float:
    """elvis.py:3505 (`calculate_fd_given_vectors`) in this build's form, between the rows A [n,d] of the reference and
    Bm [m,d] of the decoded clip, each centred by its own mean:
    FD = |mu_A - mu_B|^2 + |A|_F^2 / (n-1) + |Bm|_F^2 / (m-1) - 2 |A Bm^T|_* / sqrt((n-1)(m-1)), |.|_* the sum of
    singular values.  In exact arithmetic this is the textbook tr S1 + tr S2 - 2 tr (S1 S2)^(1/2) with np.cov
    covariances - the non-zero eigenvalues of S1 S2 are those of (A Bm^T)(A Bm^T)^T / ((n-1)(m-1)) - and it needs no
    d x d matrix and no square root of a singular product.  Fewer than two rows: FvmdNoTrajectories; more than 1024:
    ValueError (raise segment_step).  BUILD-DEFINED."""
    return float(_frechet_tensor(rows_a, rows_b).item())


def _rows_of(luma_d: torch.Tensor, seq_len: int, cfg: FvmdConfig) -> torch.Tensor:
    return motion_features_device(track_keypoints_device(luma_d, seq_len, cfg))


def _chk_pair(ref_luma_d, dec_luma_d):
    _chk_luma(ref_luma_d, "the reference clip")
    _chk_luma(dec_luma_d, "the decoded clip")
    if ref_luma_d.shape != dec_luma_d.shape or ref_luma_d.device != dec_luma_d.device:
        raise ValueError("fvmd: the two clips must be [F, H, W], of one shape and on one device")


def fvmd_device(ref_luma_d: torch.Tensor, dec_luma_d: torch.Tensor, cfg: Optional[FvmdConfig] = None) -> float:
    """The score of one window (elvis.py:3452-3509): two resident luma clips u8 [F,H,W] -> the Frechet distance between
    their segments' motion features, S = max(10, min(16, F)).  Fewer than two segments: FvmdNoTrajectories.
    BUILD-DEFINED (module docstring); it does NOT claim parity with the `fvmd` package."""
    cfg = cfg or FvmdConfig()
    _chk_pair(ref_luma_d, dec_luma_d)
    frames = ref_luma_d.shape[0]
    s = clip_seq_len(frames)
    b = segment_count(frames, s, cfg.segment_step)
    if b < 2:
        raise FvmdNoTrajectories(f"fvmd: {frames} frame(s) give {b} segment(s) of {s}; a Frechet distance needs two")
    if b > MAX_ROWS:
        raise ValueError(f"fvmd: {b} segments are more than the {MAX_ROWS} a Frechet distance takes; raise segment_step")
    return frechet_distance_device(_rows_of(ref_luma_d, s, cfg), _rows_of(dec_luma_d, s, cfg))


# ----------------------------------------------------------------------------- the reference's control flow
def fvmd_control_flow(total_frames: int, score: Callable[[Sequence[int]], float], stride: int = 1, max_frames: Optional[int] = None,
                      early_stop_delta: float = 0.002, early_stop_window: int = 50, printer: Callable = print) -> Tuple[float, float]:
    """elvis.py:3376-3597 without the frames: the sampling, early-stop, fallback and std loop of `calculate_fvmd` around
    `score(indices) -> float`, which stands where `_run_fvmd_once` renders and scores a list of sampled frame indices and
    may raise FvmdNoTrajectories.  A scorer with a `prepare(indices)` method is told each attempt's whole index list
    before its prefixes are scored.  HOST."""
    if total_frames < 2:
        raise ValueError("FVMD requires at least two frames in both reference and decoded sequences.")
    base_stride = max(1, stride)

    def _build_indices(stride_value: int) -> List[int]:
        idxs = list(range(0, total_frames, stride_value))
        if len(idxs) < 2 and total_frames >= 2:
            idxs = [0, total_frames - 1]
        if max_frames is not None and max_frames > 0:
            idxs = idxs[:max_frames]
        return list(dict.fromkeys(idxs))

    def _run_fvmd_once(frame_indices: Sequence[int]) -> float:
        if len(frame_indices) < MIN_REQUIRED_FRAMES:
            raise FvmdNoTrajectories(f"Only {len(frame_indices)} frame(s) sampled; FVMD requires at least {MIN_REQUIRED_FRAMES}.")
        value = score(frame_indices)
        if not np.isfinite(value):
            raise RuntimeError("FVMD produced a non-finite score.")
        return float(value)

    def _compute_std(selected_indices: Sequence[int]) -> float:
        if len(selected_indices) < 2:
            return 0.0
        scores: List[float] = []
        warned = False
        window_span = min(len(selected_indices), max(MIN_REQUIRED_FRAMES, 8))
        for start in range(0, len(selected_indices) - window_span + 1):
            window_indices = selected_indices[start:start + window_span]
            try:
                scores.append(_run_fvmd_once(window_indices))
            except FvmdNoTrajectories as exc:
                if not warned:
                    printer("  Warning: FVMD could not compute variability for one or more windows; "
                            f"first failure involving frames {window_indices}: {exc}")
                    warned = True
        if len(scores) <= 1:
            return 0.0
        return float(np.std(scores, ddof=1))

    window = max(1, early_stop_window)
    attempt_stride = base_stride
    while True:
        indices = _build_indices(attempt_stride)
        if len(indices) < MIN_REQUIRED_FRAMES:
            if attempt_stride == 1:
                raise ValueError(f"FVMD requires at least {MIN_REQUIRED_FRAMES} sampled frames; provide more frames or disable stride.")
            next_stride = max(1, attempt_stride // 2)
            if next_stride == attempt_stride:
                next_stride = attempt_stride - 1
            printer(f"  Warning: FVMD sampling with stride {attempt_stride} yielded only {len(indices)} frame(s); retrying with stride {next_stride}.")
            attempt_stride = next_stride
            continue
        processed = 0
        last_score: Optional[float] = None
        used_indices: Sequence[int] = []
        try:
            if hasattr(score, "prepare"):
                score.prepare(indices)
            while processed < len(indices):
                next_count = min(len(indices), processed + window)
                current_indices = indices[:next_count]
                current_score = _run_fvmd_once(current_indices)
                used_indices = list(current_indices)
                if last_score is not None:
                    baseline = max(abs(last_score), 1e-6)
                    delta = abs(current_score - last_score) / baseline
                    if delta < early_stop_delta:
                        std_value = _compute_std(used_indices)
                        if attempt_stride != base_stride:
                            printer(f"  Info: FVMD used effective stride {attempt_stride} instead of requested {base_stride}.")
                        return current_score, std_value
                last_score = current_score
                processed = next_count
            assert last_score is not None
            std_value = _compute_std(used_indices if used_indices else indices)
            if attempt_stride != base_stride:
                printer(f"  Info: FVMD used effective stride {attempt_stride} instead of requested {base_stride}.")
            return last_score, std_value
        except FvmdNoTrajectories as exc:
            if attempt_stride == 1:
                raise RuntimeError("FVMD failed to track keypoints even with stride=1. Consider reviewing the input frames or masks.") from exc
            next_stride = max(1, attempt_stride // 2)
            if next_stride == attempt_stride:
                next_stride = attempt_stride - 1
            printer(f"  Warning: FVMD tracking failed with stride {attempt_stride}; retrying with stride {next_stride}.")
            attempt_stride = next_stride


class _ClipScorer:
    """`_run_fvmd_once` on two resident luma clips.  `prepare(indices)` tracks the sampled clip once with S = 16 and keeps
    its feature rows; a prefix of those indices is then scored over the first rows.  Any other window is tracked afresh."""

    def __init__(self, ref_luma_d: torch.Tensor, dec_luma_d: torch.Tensor, cfg: FvmdConfig):
        self.ref, self.dec, self.cfg = ref_luma_d, dec_luma_d, cfg
        self.base: Tuple[int, ...] = ()
        self.rows: Optional[Tuple[torch.Tensor, torch.Tensor]] = None

    def _take(self, indices: Sequence[int]):
        if list(indices) == list(range(self.ref.shape[0])):
            return self.ref, self.dec
        at = torch.as_tensor(list(indices), dtype=torch.long, device=self.ref.device)
        return self.ref.index_select(0, at), self.dec.index_select(0, at)

    def prepare(self, indices: Sequence[int]) -> None:
        self.base, self.rows = tuple(indices), None
        s = clip_seq_len(len(indices))
        if s == MAX_SEQ_LEN and segment_count(len(indices), s, self.cfg.segment_step) >= 2:
            a, b = self._take(indices)
            self.rows = (_rows_of(a, s, self.cfg), _rows_of(b, s, self.cfg))

    def __call__(self, indices: Sequence[int]) -> float:
        count = len(indices)
        s = clip_seq_len(count)
        b = segment_count(count, s, self.cfg.segment_step)
        if b < 2:
            raise FvmdNoTrajectories(f"fvmd: {count} frame(s) give {b} segment(s) of {s}; a Frechet distance needs two")
        if b > MAX_ROWS:
            raise ValueError(f"fvmd: {b} segments are more than the {MAX_ROWS} a Frechet distance takes; raise segment_step")
        if self.rows is not None and s == MAX_SEQ_LEN and tuple(indices) == self.base[:count]:
            return frechet_distance_device(self.rows[0][:b], self.rows[1][:b])
        a, d = self._take(indices)
        return frechet_distance_device(_rows_of(a, s, self.cfg), _rows_of(d, s, self.cfg))


def _make_scorer(ref_luma_d: torch.Tensor, dec_luma_d: torch.Tensor, cfg: FvmdConfig):
    return _ClipScorer(ref_luma_d, dec_luma_d, cfg)


def calculate_fvmd_device(ref_luma_d: torch.Tensor, dec_luma_d: torch.Tensor, cfg: Optional[FvmdConfig] = None, stride: int = 1,
                          max_frames: Optional[int] = None, early_stop_delta: float = 0.002, early_stop_window: int = 50,
                          verbose: bool = False) -> Tuple[float, float]:
    """`calculate_fvmd` (elvis.py:3358-3597) on two resident luma clips u8 [F,H,W]: (value, std).  BUILD-DEFINED
    (module docstring); the departures are listed there."""
    cfg = cfg or FvmdConfig()
    _chk_pair(ref_luma_d, dec_luma_d)
    printer = print if verbose else (lambda *args, **kwargs: None)
    with torch.cuda.device(ref_luma_d.device):
        return fvmd_control_flow(ref_luma_d.shape[0], _make_scorer(ref_luma_d, dec_luma_d, cfg), stride, max_frames, early_stop_delta,
                                 early_stop_window, printer)


def _host_planes(frames: Sequence[np.ndarray], count: int) -> np.ndarray:
    """The first `count` frames as one uint8 array [count, H, W(, 3)], checked on the host."""
    planes = []
    for f in frames[:count]:
        if f is None:
            raise ValueError("Frames must not be None when computing FVMD.")
        f = np.ascontiguousarray(f)
        if f.dtype != np.uint8:
            f = np.clip(f, 0, 255).astype(np.uint8)
        planes.append(f)
    shape = planes[0].shape
    if any(p.shape != shape for p in planes) or len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 3):
        raise ValueError("fvmd: frames must be H x W x 3 (BGR) or H x W (luma) arrays of one shape")
    if shape[0] < MIN_SIDE or shape[1] < MIN_SIDE:
        raise ValueError(f"fvmd: a {shape[0]} x {shape[1]} plane is smaller than {MIN_SIDE} x {MIN_SIDE}")
    return np.stack(planes)


def calculate_fvmd(reference_frames: Sequence[np.ndarray], decoded_frames: Sequence[np.ndarray], log_root: Optional[str] = None,
                   stride: int = 1, max_frames: Optional[int] = None, early_stop_delta: float = 0.002, early_stop_window: int = 50,
                   device=None, verbose: bool = True, *, cfg: Optional[FvmdConfig] = None) -> Tuple[float, float]:
    """elvis.py:3358-3597 on the device, with the reference's signature: (fvmd_value, std_dev) of two lists of frames -
    H x W x 3 BGR (reduced to luma by `vmaf.luma_device`) or H x W luma; other dtypes are clipped to uint8 as the
    reference does before it writes them.  `device`: None (cuda:0), an index as in the reference, or a torch device.
    The control flow is the reference's own (`fvmd_control_flow`).  DEPARTURES: nothing is written to disk and
    `log_root` is ignored; frames under 64 x 64 and clips of differing shape raise ValueError; a window of fewer than
    two segments raises FvmdNoTrajectories, so the std is 0.0; the clip is tracked once per sampling stride.
    BUILD-DEFINED (module docstring): it does NOT claim parity with the `fvmd` package."""
    cfg = cfg or FvmdConfig()
    printer = print if verbose else (lambda *args, **kwargs: None)
    if not len(reference_frames) or not len(decoded_frames):
        raise ValueError("Both reference_frames and decoded_frames must contain at least one frame.")
    total_frames = min(len(reference_frames), len(decoded_frames))
    if total_frames < 2:
        raise ValueError("FVMD requires at least two frames in both reference and decoded sequences.")
    if total_frames < MIN_REQUIRED_FRAMES:                                    # what the loop would find at stride 1, before any upload
        raise ValueError(f"FVMD requires at least {MIN_REQUIRED_FRAMES} sampled frames; provide more frames or disable stride.")
    scorer = _make_scorer_host(reference_frames, decoded_frames, total_frames, device, cfg)
    return fvmd_control_flow(total_frames, scorer, stride, max_frames, early_stop_delta, early_stop_window, printer)


def _make_scorer_host(reference_frames, decoded_frames, total_frames: int, device, cfg: FvmdConfig):
    from .vmaf import luma_device
    ref, dec = _host_planes(reference_frames, total_frames), _host_planes(decoded_frames, total_frames)
    if ref.shape != dec.shape:
        raise ValueError("fvmd: the two clips must be of one shape")
    dev = L.resolve_device("cuda:0" if device is None else f"cuda:{device}" if isinstance(device, int) else device)
    with torch.cuda.device(dev):
        ref_d, dec_d = (torch.from_numpy(t).to(dev) for t in (ref, dec))
        if ref.ndim == 4:
            ref_d, dec_d = luma_device(ref_d, "bgr"), luma_device(dec_d, "bgr")
    return _make_scorer(ref_d, dec_d, cfg)
