"""VMAF of the evaluation report on the device.

The reference computes VMAF by writing both clips to disk as I420 and starting `/opt/local/bin/vmaf` in a subprocess:
`calculate_vmaf` (elvis.py:3197-3356, called twice per evaluated video at elvis.py:3932-3952) and `calculate_vmaf`
(presley.py:262-326, inside `measure_performance`).  libvmaf and its model file are available neither to the reference
tree nor to this build.

BUILD-DEFINED: a restatement of the published float feature extractors - VIF on four scales, ADM2 on four scales,
motion2 - and of the nu-SVR over them, behind the reference's call surfaces, on the device (csrc/vmaf.hip).  The
constants are recalled from libvmaf and UNVERIFIED against it.  The contract is the one of include/elvis_amd.h and
DESIGN.md 7; tests/_vmaf_ref.py states it in numpy float64 and the device agrees with it to 1e-9 * max(1, |value|).
It does NOT claim parity with libvmaf.  The model is a seeded synthetic one (`make_vmaf_model`) unless a real
`vmaf_v0.6.1.json` is given (`load_vmaf_model`); nothing is downloaded.
PINNED against the reference's own code: the statistics block of elvis.py:3316-3331 (`vmaf_stats`).
DEPARTURES: a container other than `.yuv` / `.y4m` raises ValueError (there is no ffmpeg to convert it), and so do a
`.y4m` whose header disagrees with `width` / `height`, clips of different length, and planes under 64 x 64.
"""
from __future__ import annotations

import json
import math
import os
import threading
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib, ptr
from .ops import _s

MIN_SIDE = 64
VMAF_CHUNK_BYTES = 64 << 20        # host clips are uploaded in chunks of about this size
FEATURE_KEYS = ("adm2", "motion2", "vif_scale0", "vif_scale1", "vif_scale2", "vif_scale3")
SYNTHETIC_SUPPORT_VECTORS = 32

_CSF_A = ((0.62171, 0.67234, 0.72709, 0.67234), (0.34537, 0.41317, 0.49428, 0.41317), (0.18004, 0.22727, 0.28688, 0.22727),
          (0.091401, 0.11792, 0.15214, 0.11792))
_CSF_G = (1.501, 1.0, 0.534, 1.0)

_tables_lock = threading.Lock()
_tables: Dict[str, torch.Tensor] = {}


# ----------------------------------------------------------------------------- the tables
def _gaussian(n: int, sigma: float) -> np.ndarray:
    k = np.arange(n, dtype=np.float64) - n // 2
    g = np.exp(-(k * k) / (2.0 * sigma ** 2))
    return g / g.sum()


def _csf_q(lam: int, theta: int) -> float:
    r = 3.0 * 1080.0 * math.pi / 180.0
    return 2.0 * 0.495 * 10.0 ** (0.466 * math.log10(2.0 ** lam * 0.401 * _CSF_G[theta] / r) ** 2) / _CSF_A[lam - 1][theta]


def vmaf_tables() -> np.ndarray:
    """The 56 float64 constants the kernels are handed, built on the host so that no device exp / cos takes part:
    the normalised Gaussians exp(-k^2 / (2 (N / 5)^2)) of N = 17, 9, 5, 3 taps (VIF scales 0..3), the 5-tap motion
    blur exp(-k^2 / 2), the db2 analysis pair, cos^2(1 degree), and per ADM scale 1 / Q(scale + 1, 1) (h and v bands)
    and 1 / Q(scale + 1, 2) (d band)."""
    r3, d = math.sqrt(3.0), 4.0 * math.sqrt(2.0)
    lo = np.asarray([(1 + r3) / d, (3 + r3) / d, (3 - r3) / d, (1 - r3) / d], np.float64)
    hi = np.asarray([lo[3], -lo[2], lo[1], -lo[0]], np.float64)
    csf = [1.0 / _csf_q(s + 1, th) for s in range(4) for th in (1, 2)]
    return np.ascontiguousarray(np.concatenate([_gaussian(17, 17 / 5.0), _gaussian(9, 9 / 5.0), _gaussian(5, 5 / 5.0),
                                                _gaussian(3, 3 / 5.0), _gaussian(5, 1.0), lo, hi,
                                                [math.cos(math.pi / 180.0) ** 2], csf]).astype(np.float64))


def _device_tables(device: torch.device) -> torch.Tensor:
    with _tables_lock:
        if str(device) not in _tables:
            _tables[str(device)] = torch.from_numpy(vmaf_tables()).to(device)
        return _tables[str(device)]


# ----------------------------------------------------------------------------- the model
@dataclass
class VmafModel:
    """A nu-SVR with an RBF kernel over the six features, in this build's feature order (`feature_names`).
    f'_i = slopes[i + 1] f_i + intercepts[i + 1]; p = sum_j coef_j exp(-gamma |sv_j - f'|^2) - rho;
    score = (p - intercepts[0]) / slopes[0]; with `enable_transform`, t = p0 + p1 s + p2 s^2 (and max(t, s) where
    out_gte_in); then the clip.  BUILD-DEFINED (module docstring)."""
    slopes: np.ndarray                                   # [7]
    intercepts: np.ndarray                               # [7]
    sv: np.ndarray                                       # [n, 6]
    coef: np.ndarray                                     # [n]
    rho: float
    gamma: float
    score_clip: Optional[Tuple[float, float]] = (0.0, 100.0)
    transform: Tuple[float, float, float, bool] = (0.0, 1.0, 0.0, False)
    enable_transform: bool = False
    feature_names: Tuple[str, ...] = FEATURE_KEYS
    _resident: Dict[str, torch.Tensor] = field(default_factory=dict, repr=False, compare=False)
    _lock: threading.Lock = field(default_factory=threading.Lock, repr=False, compare=False)

    def __post_init__(self):
        self.slopes = np.ascontiguousarray(self.slopes, np.float64)
        self.intercepts = np.ascontiguousarray(self.intercepts, np.float64)
        self.sv = np.ascontiguousarray(self.sv, np.float64)
        self.coef = np.ascontiguousarray(self.coef, np.float64)
        if self.slopes.shape != (7,) or self.intercepts.shape != (7,):
            raise ValueError("vmaf model: slopes and intercepts hold 7 values, the score's and the six features'")
        if self.sv.ndim != 2 or self.sv.shape[1] != 6 or self.sv.shape[0] < 1 or self.coef.shape != (self.sv.shape[0],):
            raise ValueError("vmaf model: support vectors must be [n, 6] with n >= 1 and coef [n]")
        if self.slopes[0] == 0.0:
            raise ValueError("vmaf model: slopes[0] is 0")

    @property
    def flags(self) -> int:
        return int(bool(self.enable_transform)) | int(bool(self.transform[3])) << 1 | int(self.score_clip is not None) << 2

    def packed(self) -> np.ndarray:
        """The float64 array elvis_vmaf_predict_f64 takes."""
        clip = (0.0, 0.0) if self.score_clip is None else tuple(float(v) for v in self.score_clip)
        head = np.concatenate([self.slopes, self.intercepts, [self.rho, self.gamma], clip, [float(v) for v in self.transform[:3]]])
        return np.ascontiguousarray(np.concatenate([head, self.sv.reshape(-1), self.coef]), np.float64)

    def on(self, device) -> torch.Tensor:
        with self._lock:
            key = str(device)
            if key not in self._resident:
                self._resident[key] = torch.from_numpy(self.packed()).to(device)
            return self._resident[key]


def make_vmaf_model(seed: int = 0) -> VmafModel:
    """The seeded synthetic default: 32 support vectors in the unit cube, positive coefficients, scores spread over
    the clip's range for features in theirs.  It stands in for a trained model's arithmetic, not for its judgement."""
    rng = np.random.default_rng(seed)
    n = SYNTHETIC_SUPPORT_VECTORS
    sv = rng.uniform(0.0, 1.0, (n, 6))
    coef = rng.uniform(0.5, 1.5, n) / n
    slopes = np.concatenate([[0.01], rng.uniform(0.8, 1.2, 6)])
    slopes[2] = 0.05                                                  # motion2 runs to tens, the others to 1
    intercepts = np.concatenate([[0.0], rng.uniform(-0.1, 0.1, 6)])
    return VmafModel(slopes, intercepts, sv, coef, rho=0.05, gamma=0.5, score_clip=(0.0, 100.0), transform=(1.7, 1.04, -0.0004, True))


def _feature_slot(name: str) -> int:
    for slot, key in enumerate(FEATURE_KEYS):
        if key in name:
            return slot
    raise ValueError(f"vmaf model: feature_names: unknown feature {name!r} (known: {', '.join(FEATURE_KEYS)})")


def load_vmaf_model(path: str) -> VmafModel:
    """A model in libvmaf's JSON layout, as `vmaf_v0.6.1.json` has it: `model_dict` with `model_type` "LIBSVMNUSVR",
    `norm_type` "linear_rescale", `feature_names`, `slopes`, `intercepts` (the score's first, then one per feature in
    `feature_names`' order), `score_clip`, optionally `score_transform` {p0, p1, p2, out_gte_in}, and `model`: the
    libsvm text - `svm_type`, `kernel_type rbf`, `gamma`, `total_sv`, `rho`, then after `SV` one line
    `coef 1:v 2:v ...` per support vector.  This layout is recalled from libvmaf 2.x and is UNVERIFIED here: neither
    the library nor its model file is available to this build.  Feature names are mapped by the substrings `adm2`,
    `motion2`, `vif_scale0..3`, in any order.  The transform is read and left off (`enable_transform = False`), as
    libvmaf leaves it.  ValueError naming the field: another `model_type`, `norm_type` or `kernel_type`, an unknown
    feature, a count mismatch, a missing key."""
    with open(path, "r") as f:
        doc = json.load(f)

    def need(d, key, where):
        if not isinstance(d, dict) or key not in d:
            raise ValueError(f"{path}: vmaf model: {where}{key} is missing")
        return d[key]

    md = need(doc, "model_dict", "")
    if need(md, "model_type", "model_dict.") != "LIBSVMNUSVR":
        raise ValueError(f"{path}: vmaf model: model_type {md['model_type']!r} is not LIBSVMNUSVR")
    if need(md, "norm_type", "model_dict.") != "linear_rescale":
        raise ValueError(f"{path}: vmaf model: norm_type {md['norm_type']!r} is not linear_rescale")
    names = list(need(md, "feature_names", "model_dict."))
    slots = [_feature_slot(str(nm)) for nm in names]
    if sorted(slots) != list(range(6)):
        raise ValueError(f"{path}: vmaf model: feature_names must name each of {', '.join(FEATURE_KEYS)} once, got {names}")
    slopes, intercepts = list(need(md, "slopes", "model_dict.")), list(need(md, "intercepts", "model_dict."))
    if len(slopes) != 7 or len(intercepts) != 7:
        raise ValueError(f"{path}: vmaf model: slopes / intercepts hold {len(slopes)} / {len(intercepts)} values, expected 7 (count mismatch)")
    clip = need(md, "score_clip", "model_dict.")
    if clip is not None and len(clip) != 2:
        raise ValueError(f"{path}: vmaf model: score_clip must hold two values")
    tr = md.get("score_transform") or {}
    truth = tr.get("out_gte_in", False)
    transform = (float(tr.get("p0", 0.0)), float(tr.get("p1", 1.0)), float(tr.get("p2", 0.0)),
                 truth.strip().lower() == "true" if isinstance(truth, str) else bool(truth))
    text = need(md, "model", "model_dict.")
    head: Dict[str, str] = {}
    rows: List[str] = []
    in_sv = False
    for line in str(text).splitlines():
        line = line.strip()
        if not line:
            continue
        if in_sv:
            rows.append(line)
        elif line == "SV":
            in_sv = True
        else:
            key, _, value = line.partition(" ")
            head[key] = value.strip()
    for key in ("svm_type", "kernel_type", "gamma", "total_sv", "rho"):
        if key not in head:
            raise ValueError(f"{path}: vmaf model: model: {key} is missing")
    if head["kernel_type"] != "rbf":
        raise ValueError(f"{path}: vmaf model: kernel_type {head['kernel_type']!r} is not rbf")
    if head["svm_type"] != "nu_svr":
        raise ValueError(f"{path}: vmaf model: svm_type {head['svm_type']!r} is not nu_svr")
    if int(head["total_sv"]) != len(rows) or not rows:
        raise ValueError(f"{path}: vmaf model: total_sv says {head['total_sv']}, the text holds {len(rows)} (count mismatch)")
    sv = np.zeros((len(rows), 6), np.float64)
    coef = np.zeros(len(rows), np.float64)
    for j, row in enumerate(rows):
        parts = row.split()
        coef[j] = float(parts[0])
        for item in parts[1:]:
            idx, _, value = item.partition(":")
            if not 1 <= int(idx) <= 6:
                raise ValueError(f"{path}: vmaf model: support vector {j} has index {idx}; six features (count mismatch)")
            sv[j, slots[int(idx) - 1]] = float(value)
    order = [0] + [1 + slots.index(slot) for slot in range(6)]             # ours <- the file's
    return VmafModel(np.asarray(slopes, np.float64)[order], np.asarray(intercepts, np.float64)[order], sv, coef,
                     rho=float(head["rho"]), gamma=float(head["gamma"]),
                     score_clip=None if clip is None else (float(clip[0]), float(clip[1])), transform=transform, enable_transform=False)


_VMAF_MODEL_CACHE: Dict[Tuple[Optional[str], str], VmafModel] = {}
_cache_lock = threading.Lock()


def get_vmaf_model(model_path: Optional[str] = None, device="cuda:0") -> VmafModel:
    """One model per (file, device), loaded and made resident on first use, under a lock.  Without a path: the
    synthetic `make_vmaf_model(0)`."""
    dev = L.resolve_device(device)
    key = (None if model_path is None else os.path.abspath(os.fspath(model_path)), str(dev))
    with _cache_lock:
        model = _VMAF_MODEL_CACHE.get(key)
        if model is None:
            model = _VMAF_MODEL_CACHE[key] = make_vmaf_model(0) if model_path is None else load_vmaf_model(os.fspath(model_path))
            model.on(dev)
        return model


# ----------------------------------------------------------------------------- the device form
def luma_device(frames_d: torch.Tensor, order: str = "bgr", masks: Optional[torch.Tensor] = None, invert: bool = False,
                rect: Optional[Tuple[int, int, int, int]] = None) -> torch.Tensor:
    """The luma plane the metric reads, of a resident clip: frames [n,H,W,3] u8 -> [n, y1 - y0, x1 - x0] u8, the Y of
    `rgb_to_i420_device` (any H and W).  `masks` u8 [n,H,W]: where it is 0 (where it is set, with `invert`) the pixel's
    three bytes count as 0 (`apply_binary_mask`), which is luma 16; `rect` (y0, y1, x0, x1) crops."""
    if order not in ("rgb", "bgr"):
        raise ValueError('vmaf luma: order must be "rgb" or "bgr"')
    if not isinstance(frames_d, torch.Tensor) or frames_d.dtype != torch.uint8 or not frames_d.is_cuda or not frames_d.is_contiguous() \
            or frames_d.dim() != 4 or frames_d.shape[3] != 3:
        raise ValueError("vmaf luma: frames must be a contiguous CUDA uint8 tensor [n, H, W, 3]")
    n, h, w, _ = frames_d.shape
    if masks is not None and (not isinstance(masks, torch.Tensor) or masks.dtype != torch.uint8 or not masks.is_contiguous()
                              or masks.device != frames_d.device or tuple(masks.shape) != (n, h, w)):
        raise ValueError(f"vmaf luma: masks must be a contiguous uint8 tensor {(n, h, w)} on the frames' device")
    rect = (0, h, 0, w) if rect is None else tuple(int(v) for v in rect)
    if len(rect) != 4 or rect[0] < 0 or rect[2] < 0 or rect[1] > h or rect[3] > w or rect[0] >= rect[1] or rect[2] >= rect[3]:
        raise ValueError(f"vmaf luma: rect {rect} does not lie inside the {h} x {w} frame")
    y0, y1, x0, x1 = rect
    out = torch.empty((n, y1 - y0, x1 - x0), dtype=torch.uint8, device=frames_d.device)
    if n:
        check(lib().elvis_vmaf_luma_u8(ptr(frames_d), ptr(masks), ptr(out), n, h, w, int(order == "bgr"), int(bool(invert)), y0, y1, x0, x1,
                                       _s(frames_d)), frames_d.device)
    return out


def _chk_planes(t, who, shape=None, device=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"vmaf: {who} must be a contiguous CUDA uint8 tensor")
    if shape is not None and (tuple(t.shape) != tuple(shape) or t.device != device):
        raise ValueError(f"vmaf: {who} must have shape {tuple(shape)} on the clips' device")


def vmaf_features_device(ref_y: torch.Tensor, dis_y: torch.Tensor, prev: Optional[torch.Tensor] = None,
                         following: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ref_y, dis_y u8 [F,H,W] luma on the device, H, W >= 64 -> float64 [F,6] = adm2, motion2, vif_scale0..3.
    `prev` [H,W]: the reference plane before ref_y[0] (without it motion of frame 0 is 0); `following` [H,W]: the one
    after ref_y[-1] (without it motion2 of the last frame is its motion).  With both, a clip cut into calls gives the
    bytes of one call.  The pyramids of four frames at a time and every tile partial live in one workspace, allocated
    before the first launch.  BUILD-DEFINED (module docstring)."""
    _chk_planes(ref_y, "ref_y")
    _chk_planes(dis_y, "dis_y")
    if ref_y.dim() != 3 or ref_y.shape != dis_y.shape or ref_y.device != dis_y.device:
        raise ValueError("vmaf: the two clips must be [F, H, W], of one shape and on one device")
    n, h, w = ref_y.shape
    if h < MIN_SIDE or w < MIN_SIDE:
        raise ValueError(f"vmaf: a {h} x {w} plane is smaller than {MIN_SIDE} x {MIN_SIDE}")
    for t, who in ((prev, "prev"), (following, "following")):
        if t is not None:
            _chk_planes(t, who, (h, w), ref_y.device)
    out = torch.empty((n, 6), dtype=torch.float64, device=ref_y.device)
    if n == 0:
        return out
    nbytes = lib().elvis_vmaf_workspace_bytes(n, h, w)
    if nbytes == 0:
        raise ValueError(f"vmaf: {n} frames of {h} x {w} are more than one call holds")
    with torch.cuda.device(ref_y.device):
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=ref_y.device)
        check(lib().elvis_vmaf_features_f64(ptr(ref_y), ptr(dis_y), ptr(prev), ptr(following), ptr(_device_tables(ref_y.device)), ptr(ws),
                                            ptr(out), n, h, w, _s(ref_y)), ref_y.device)
    return out


def vmaf_predict_device(feats: torch.Tensor, model: VmafModel) -> torch.Tensor:
    """float64 [F,6] features on the device -> float64 [F] scores."""
    if not isinstance(feats, torch.Tensor) or feats.dtype != torch.float64 or not feats.is_cuda or not feats.is_contiguous() \
            or feats.dim() != 2 or feats.shape[1] != 6:
        raise ValueError("vmaf: features must be a contiguous CUDA float64 tensor [F, 6]")
    out = torch.empty(feats.shape[0], dtype=torch.float64, device=feats.device)
    if feats.shape[0]:
        with torch.cuda.device(feats.device):
            check(lib().elvis_vmaf_predict_f64(ptr(feats), ptr(model.on(feats.device)), ptr(out), feats.shape[0], model.sv.shape[0],
                                               model.flags, _s(feats)), feats.device)
    return out


def vmaf_device(ref_y: torch.Tensor, dis_y: torch.Tensor, model: VmafModel, prev: Optional[torch.Tensor] = None,
                following: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The score of every frame pair of two resident luma clips: u8 [F,H,W] x2 -> float64 [F].  BUILD-DEFINED."""
    return vmaf_predict_device(vmaf_features_device(ref_y, dis_y, prev, following), model)


def _score_chunks(chunks, model: VmafModel) -> List[float]:
    """Scores of a clip that arrives as (ref_y, dis_y) chunks: each chunk is scored with the reference plane before it
    and the one after it, so the scores do not depend on how the clip is cut."""
    scores: List[float] = []
    chunks = iter(chunks)
    before, cur = None, next(chunks, None)
    while cur is not None:
        after = next(chunks, None)
        s = vmaf_device(cur[0], cur[1], model, prev=before, following=None if after is None else after[0][0])
        scores.extend(float(v) for v in s.cpu())
        before, cur = cur[0][-1], after
    return scores


# ----------------------------------------------------------------------------- the reference's call surfaces
def vmaf_stats(scores: Sequence[float]) -> Dict[str, float]:
    """elvis.py:3316-3331: mean, min, max, population std and the harmonic mean over max(score, 0.001)."""
    vmaf_scores = [float(s) for s in scores]
    if not vmaf_scores:
        raise ValueError("vmaf_stats: no scores")
    vmaf_array = np.array(vmaf_scores)
    harmonic_mean = len(vmaf_scores) / np.sum([1.0 / max(score, 0.001) for score in vmaf_scores])
    return {'mean': float(np.mean(vmaf_array)), 'min': float(np.min(vmaf_array)), 'max': float(np.max(vmaf_array)),
            'std': float(np.std(vmaf_array)), 'harmonic_mean': float(harmonic_mean)}


def _chunk_step(plane_bytes: int, chunk_frames: Optional[int], per_frame: int) -> int:
    if chunk_frames is None:
        return max(1, VMAF_CHUNK_BYTES // max(1, per_frame * plane_bytes))
    if int(chunk_frames) < 1:
        raise ValueError("chunk_frames must be at least 1")
    return int(chunk_frames)


def calculate_vmaf_frames(reference_frames: Sequence[np.ndarray], distorted_frames: Sequence[np.ndarray],
                          model_path: Optional[str] = None, device="cuda:0", *, chunk_frames: Optional[int] = None) -> List[float]:
    """presley.py:262-326 on the device: the score of every pair of RGB frames.  The clips are uploaded in chunks of
    `chunk_frames` pairs (by default about 64 MB) and reduced to luma there; the reference plane before and after a
    chunk is carried for motion, so the scores are the same bytes at every chunk size.  BUILD-DEFINED (module docstring)."""
    if len(reference_frames) != len(distorted_frames):
        raise ValueError(f"vmaf: {len(reference_frames)} reference frames and {len(distorted_frames)} distorted frames")
    if len(reference_frames) == 0:
        return []
    shape = np.asarray(reference_frames[0]).shape
    for f in list(reference_frames) + list(distorted_frames):
        f = np.asarray(f)
        if f.shape != shape or f.ndim != 3 or f.shape[2] != 3 or f.dtype != np.uint8:
            raise ValueError("vmaf: frames must be uint8 H x W x 3 arrays of one shape")
    if shape[0] < MIN_SIDE or shape[1] < MIN_SIDE:
        raise ValueError(f"vmaf: a {shape[0]} x {shape[1]} frame is smaller than {MIN_SIDE} x {MIN_SIDE}")
    step = _chunk_step(shape[0] * shape[1], chunk_frames, 6)
    dev = L.resolve_device(device)
    model = get_vmaf_model(model_path, dev)

    def chunks():
        for at in range(0, len(reference_frames), step):
            pair = []
            for clip in (reference_frames, distorted_frames):
                host = np.ascontiguousarray(np.stack([np.asarray(f) for f in clip[at:at + step]]))
                pair.append(luma_device(torch.from_numpy(host).to(dev), order="rgb"))
            yield tuple(pair)

    with torch.cuda.device(dev):
        return _score_chunks(chunks(), model)


def sampled_frames(count: int, frame_stride: int) -> List[int]:
    """The frames `select='not(mod(n, stride))'` keeps (elvis.py:3227-3229)."""
    if int(frame_stride) < 1:
        raise ValueError("frame_stride must be at least 1")
    return list(range(0, int(count), int(frame_stride)))


def luma_plane_offsets(path: str, width: int, height: int) -> List[int]:
    """Where every frame's Y plane (width x height bytes) starts in a `.yuv` (raw I420) or `.y4m` file.  HOST; no
    payload byte is read.  ValueError: another container, a `.y4m` whose header disagrees with width / height, a `.yuv`
    that is no whole number of frames."""
    from .handoff import parse_y4m, yuv420p_frame_count
    path = os.fspath(path)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".y4m":
        info = parse_y4m(path)
        if (info.width, info.height) != (int(width), int(height)):
            raise ValueError(f"{path}: the Y4M header says {info.width} x {info.height}, the call {width} x {height}")
        return list(info.frame_offsets)
    if ext == ".yuv":
        count = yuv420p_frame_count(os.path.getsize(path), width, height, path)
        return [i * (int(width) * int(height) * 3 // 2) for i in range(count)]
    raise ValueError(f"{path}: only .yuv (raw I420) and .y4m clips are read; there is no converter for {ext or 'this file'}")


def calculate_vmaf(reference_video: str, distorted_video: str, width: int, height: int, framerate: float,
                   model_path: Optional[str] = None, frame_stride: int = 1, device="cuda:0", *,
                   chunk_frames: Optional[int] = None) -> Dict[str, float]:
    """elvis.py:3197-3356 on the device: the statistics of the per-frame scores of two clips on disk, `.yuv` (raw
    I420) or `.y4m`.  ONLY the Y planes are read, at the offsets `parse_y4m` / the frame size give, into pinned staging;
    frames n % frame_stride == 0 are kept, and motion runs between consecutive kept frames.  `framerate` is accepted and
    unused, as in the reference.  Returns {'mean', 'min', 'max', 'std', 'harmonic_mean'} (`vmaf_stats`).
    DEPARTURES: any other container, a `.y4m` whose header disagrees with width / height, clips of different length, an
    empty clip and a plane under 64 x 64 raise ValueError; the reference converts with ffmpeg and reports zeros on any
    failure.  BUILD-DEFINED (module docstring)."""
    width, height = int(width), int(height)
    if width < MIN_SIDE or height < MIN_SIDE:
        raise ValueError(f"vmaf: a {height} x {width} plane is smaller than {MIN_SIDE} x {MIN_SIDE}")
    paths = (os.fspath(reference_video), os.fspath(distorted_video))
    offsets = [luma_plane_offsets(p, width, height) for p in paths]
    if len(offsets[0]) != len(offsets[1]):
        raise ValueError(f"vmaf: {paths[0]} holds {len(offsets[0])} frames, {paths[1]} {len(offsets[1])}")
    keep = sampled_frames(len(offsets[0]), frame_stride)
    if not keep:
        raise ValueError(f"vmaf: {paths[0]} holds no frame")
    step = min(_chunk_step(width * height, chunk_frames, 2), len(keep))
    dev = L.resolve_device(device)
    model = get_vmaf_model(model_path, dev)
    plane_bytes = width * height

    def chunks(files, staging):
        for at in range(0, len(keep), step):
            part = keep[at:at + step]
            pair = []
            for f, path, offs, host in zip(files, paths, offsets, staging):
                rows = host.numpy()
                for j, frame in enumerate(part):
                    f.seek(offs[frame])
                    got = f.readinto(memoryview(rows[j]).cast("B"))
                    if got != plane_bytes:
                        raise IOError(f"{path}: frame {frame} is cut short: {got} of {plane_bytes} bytes")
                plane = torch.empty((len(part), height, width), dtype=torch.uint8, device=dev)
                plane.copy_(host[:len(part)], non_blocking=True)
                pair.append(plane)
            torch.cuda.current_stream(dev).synchronize()              # the staging buffers are free for the next chunk
            yield tuple(pair)

    with torch.cuda.device(dev), open(paths[0], "rb", buffering=0) as fa, open(paths[1], "rb", buffering=0) as fb:
        staging = [torch.empty((step, height, width), dtype=torch.uint8).pin_memory() for _ in range(2)]
        return vmaf_stats(_score_chunks(chunks((fa, fb), staging), model))
