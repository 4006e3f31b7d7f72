"""LPIPS (AlexNet) of the evaluation report on the device.

The reference scores every sampled frame with `lpips.LPIPS(net='alex')`, twice - the foreground ROI and the
background: `_get_lpips_model` (elvis.py:437-447), `calculate_lpips_per_frame` (elvis.py:3163-3195), the evaluator
(elvis.py:3853-3893) and `calculate_lpips` (presley.py:329-357).  The `lpips` package and its trained weights are
available neither to the reference tree nor to this build.

BUILD-DEFINED: `LpipsAlex` is a restatement of the published network behind the reference's call surface - five
convolutions, two max-pools, a channel-normalised squared difference, five 1x1 weightings - with seeded synthetic
weights by default (`weights.make_lpips_weights`) and a loader for a real `state_dict`.  The contract is the one of
include/elvis_amd.h and DESIGN.md 7; tests/_lpips_ref.py states it in torch float64.  It does NOT claim parity with the
lpips package.
PINNED against the reference's own code (tests/golden/lpips.npz, tools/make_lpips_golden.py): the wrapper of
`calculate_lpips_per_frame` - the channel order, `/ 127.5 - 1`, the pairing of the lists and the skipping of `None`.

The stem, the 5x5 conv, the max-pools and the distance are csrc/lpips.hip; the three 3x3 layers run through
`ops.PackedConv` (fp32, exact MFMA).
"""
from __future__ import annotations

import threading
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import ops
from ._lib import check, lib, ptr
from .ops import Act, _s
from .weights import LPIPS_CONVS, LPIPS_TAP_CHANNELS, make_lpips_weights

MIN_SIDE = 31                      # a smaller input leaves no pixel for the second max-pool
LPIPS_CHUNK_BYTES = 64 << 20       # host clips are uploaded in chunks of about this size
LPIPS_PAIRS_PER_PASS = 4           # frame pairs whose activations are resident at once


def load_lpips_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A `state_dict` in the layout `LpipsAlex` takes (`weights.make_lpips_weights`'s): fp32 CPU tensors
    `features.{0,3,6,8,10}.{weight,bias}` and `lin{0..4}.model.1.weight`.  Accepted spellings of the convs:
    `net.slice{1..5}.{0,3,6,8,10}.{weight,bias}` (the lpips package's wrapped AlexNet) or `features.{0,3,6,8,10}.*`
    (torchvision's); the 1x1 weightings are `lin{0..4}.model.1.weight` of shape [1, C, 1, 1].  These names are recalled
    from lpips 0.1.x and torchvision and are UNVERIFIED here: neither package is available to this build.  Other keys
    (the scaling layer's buffers, a classifier) are ignored.  A missing key, a wrong shape or a negative 1x1 weight
    raises ValueError."""
    out: Dict[str, torch.Tensor] = {}
    for slice_no, (idx, cin, cout, k) in enumerate(LPIPS_CONVS, start=1):
        for part, shape in (("weight", (cout, cin, k, k)), ("bias", (cout,))):
            names = (f"features.{idx}.{part}", f"net.slice{slice_no}.{idx}.{part}")
            found = [n for n in names if n in sd]
            if not found:
                raise ValueError(f"lpips state_dict: none of {names} is present")
            t = torch.as_tensor(sd[found[0]]).detach().to(device="cpu", dtype=torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"lpips state_dict: {found[0]} has shape {tuple(t.shape)}, expected {shape}")
            out[f"features.{idx}.{part}"] = t
    for tap, c in enumerate(LPIPS_TAP_CHANNELS):
        name = f"lin{tap}.model.1.weight"
        if name not in sd:
            raise ValueError(f"lpips state_dict: {name} is missing")
        t = torch.as_tensor(sd[name]).detach().to(device="cpu", dtype=torch.float32).contiguous()
        if tuple(t.shape) != (1, c, 1, 1):
            raise ValueError(f"lpips state_dict: {name} has shape {tuple(t.shape)}, expected {(1, c, 1, 1)}")
        if bool((t < 0).any()):
            raise ValueError(f"lpips state_dict: {name} has a negative weight; the 1x1 weightings are non-negative")
        out[name] = t
    return out


class LpipsAlex:
    """The network's weights on one device, packed for the kernels.  `weights` is a state_dict in either spelling
    `load_lpips_state_dict` accepts; None is the seed-0 synthetic set.  BUILD-DEFINED (module docstring)."""

    def __init__(self, weights: Optional[Dict[str, torch.Tensor]] = None, device="cuda:0"):
        self.device = L.resolve_device(device)
        sd = load_lpips_state_dict(make_lpips_weights(0) if weights is None else weights)
        dev = self.device
        with torch.cuda.device(dev):
            # stem [363][64], row (ky 11 + kx) 3 + c; 5x5 conv [1600][192], row (ky 5 + kx) 64 + c
            self.stem_w = sd["features.0.weight"].permute(2, 3, 1, 0).reshape(363, 64).contiguous().to(dev)
            self.stem_b = sd["features.0.bias"].to(dev)
            self.conv5_w = sd["features.3.weight"].permute(2, 3, 1, 0).reshape(1600, 192).contiguous().to(dev)
            self.conv5_b = sd["features.3.bias"].to(dev)
            self.convs3 = [ops.PackedConv(sd[f"features.{idx}.weight"], sd[f"features.{idx}.bias"], torch.float32, dev, cin, x3=False)
                           for idx, cin, _, _ in LPIPS_CONVS[2:]]
            self.lin = [sd[f"lin{tap}.model.1.weight"].reshape(-1).contiguous().to(dev) for tap in range(5)]
            torch.cuda.current_stream(dev).synchronize()

    def parameters(self):
        """The reference reads `next(model.parameters()).device` (presley.py:336)."""
        return iter([self.stem_w, self.stem_b, self.conv5_w, self.conv5_b] + self.lin)


_LPIPS_MODEL_CACHE: Dict[str, LpipsAlex] = {}
_cache_lock = threading.Lock()


def get_lpips_model(device="cuda:0") -> LpipsAlex:
    """elvis.py:437-447: one model per device, built on first use, under a lock."""
    dev = L.resolve_device(device)
    with _cache_lock:
        model = _LPIPS_MODEL_CACHE.get(str(dev))
        if model is None:
            model = _LPIPS_MODEL_CACHE[str(dev)] = LpipsAlex(None, dev)
        return model


# ----------------------------------------------------------------------------- the device form, kernel by kernel
def stem_device(frames_d: torch.Tensor, model: LpipsAlex, masks: Optional[torch.Tensor], rect: Tuple[int, int, int, int],
                order: str, out: Optional[Act] = None) -> Act:
    n, h, w, _ = frames_d.shape
    y0, y1, x0, x1 = rect
    ho, wo = (y1 - y0 - 7) // 4 + 1, (x1 - x0 - 7) // 4 + 1
    if out is None:
        out = ops.new_act(n, ho, wo, 64, torch.float32, frames_d.device, zero=False)
    check(lib().elvis_lpips_stem_u8(ptr(frames_d), ptr(masks), ptr(model.stem_w), ptr(model.stem_b), ptr(out.t), n, h, w, y0, y1, x0, x1,
                                    int(order == "bgr"), out.pitch, _s(frames_d)), frames_d.device)
    return out


def maxpool_device(x: Act) -> Act:
    out = ops.new_act(x.n, (x.h - 3) // 2 + 1, (x.w - 3) // 2 + 1, x.c, torch.float32, x.t.device)
    check(lib().elvis_lpips_maxpool_f32(ptr(x.t), ptr(out.t), x.n, x.h, x.w, x.c, x.pitch, out.pitch, _s(x.t)), x.t.device)
    return out


def conv5_device(x: Act, model: LpipsAlex) -> Act:
    out = ops.new_act(x.n, x.h, x.w, 192, torch.float32, x.t.device, zero=False)
    check(lib().elvis_lpips_conv5_f32(ptr(x.t), ptr(model.conv5_w), ptr(model.conv5_b), ptr(out.t), x.n, x.h, x.w, x.pitch, out.pitch,
                                      _s(x.t)), x.t.device)
    return out


def distance_device(x: torch.Tensor, y: torch.Tensor, c: int, weight: torch.Tensor, out: torch.Tensor, accumulate: bool) -> torch.Tensor:
    """One tap: x, y fp32 [n,h,w,pitch] -> out float64 [n] (stored, or added to with `accumulate`)."""
    n, h, w, pitch = x.shape
    ws = torch.empty(max(1, lib().elvis_lpips_distance_workspace_bytes(n, h, w) // 8), dtype=torch.float64, device=x.device)
    check(lib().elvis_lpips_distance_f64(ptr(x), ptr(y), ptr(weight), ptr(ws), ptr(out), n, h, w, c, pitch, int(bool(accumulate)), _s(x)),
          x.device)
    return out


def features_device(frames_d: torch.Tensor, model: LpipsAlex, masks, rect, order) -> List[Act]:
    """The five taps of a resident u8 clip."""
    t0 = stem_device(frames_d, model, masks, rect, order)
    t1 = conv5_device(maxpool_device(t0), model)
    t2 = model.convs3[0](maxpool_device(t1), act=3)
    t3 = model.convs3[1](t2, act=3)
    t4 = model.convs3[2](t3, act=3)
    return [t0, t1, t2, t3, t4]


def _chk_clip(t, who):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or t.dim() != 4 or t.shape[3] != 3:
        raise ValueError(f"lpips: {who} must be a contiguous CUDA uint8 tensor [n, H, W, 3]")


def lpips_device(a_d: torch.Tensor, b_d: torch.Tensor, model: LpipsAlex, masks: Optional[torch.Tensor] = None,
                 rect: Optional[Tuple[int, int, int, int]] = None, order: str = "bgr") -> torch.Tensor:
    """The score of every frame pair of two resident clips: a_d, b_d u8 [n,H,W,3] -> float64 [n].  `masks` u8 [n,H,W]:
    where it is 0 the pixel's three bytes are taken as 0 in both clips (`_apply_binary_mask`); `rect` (y0, y1, x0, x1):
    the network sees that crop of the masked frames (the reference's `roi_slice`).  Nothing is copied or written back.
    A rect (or frame) under 31 x 31 raises ValueError - the package would raise inside a max-pool.  A frame's score does
    not depend on n.  BUILD-DEFINED (module docstring)."""
    _chk_clip(a_d, "a")
    _chk_clip(b_d, "b")
    if a_d.shape != b_d.shape or a_d.device != b_d.device:
        raise ValueError("lpips: the two clips must have one shape and one device")
    if order not in ("rgb", "bgr"):
        raise ValueError('lpips: order must be "rgb" or "bgr"')
    n, h, w, _ = a_d.shape
    if masks is not None and (not isinstance(masks, torch.Tensor) or masks.dtype != torch.uint8 or not masks.is_contiguous()
                              or masks.device != a_d.device or tuple(masks.shape) != (n, h, w)):
        raise ValueError(f"lpips: masks must be a contiguous uint8 tensor {(n, h, w)} on the clips' device")
    rect = (0, h, 0, w) if rect is None else tuple(int(v) for v in rect)
    y0, y1, x0, x1 = rect
    if len(rect) != 4 or y0 < 0 or x0 < 0 or y1 > h or x1 > w:
        raise ValueError(f"lpips: rect {rect} does not lie inside the {h} x {w} frame")
    if y1 - y0 < MIN_SIDE or x1 - x0 < MIN_SIDE:
        raise ValueError(f"lpips: the input must be at least {MIN_SIDE} x {MIN_SIDE}, got {y1 - y0} x {x1 - x0}")
    if model.device != a_d.device:
        raise ValueError(f"lpips: the model is on {model.device}, the clips on {a_d.device}")
    out = torch.empty(n, dtype=torch.float64, device=a_d.device)
    with torch.cuda.device(a_d.device):
        for at in range(0, n, LPIPS_PAIRS_PER_PASS):
            sl = slice(at, min(n, at + LPIPS_PAIRS_PER_PASS))
            m = None if masks is None else masks[sl]
            fa = features_device(a_d[sl], model, m, rect, order)
            fb = features_device(b_d[sl], model, m, rect, order)
            for tap in range(5):
                distance_device(fa[tap].t, fb[tap].t, fa[tap].c, model.lin[tap], out[sl], accumulate=tap > 0)
    return out


# ----------------------------------------------------------------------------- the reference's call surfaces
def _pairs(reference_frames, decoded_frames):
    pairs = []
    for ref, dec in zip(reference_frames, decoded_frames):
        if ref is None or dec is None:
            continue
        ref, dec = np.asarray(ref), np.asarray(dec)
        if ref.shape != dec.shape or ref.ndim != 3 or ref.shape[2] != 3 or ref.dtype != np.uint8 or dec.dtype != np.uint8:
            raise ValueError("lpips: frames must be uint8 H x W x 3 arrays, a pair of one shape")
        pairs.append((ref, dec))
    return pairs


def _score_pairs(pairs, model: LpipsAlex, order: str, chunk_frames: Optional[int]) -> List[float]:
    if chunk_frames is not None and int(chunk_frames) < 1:
        raise ValueError("chunk_frames must be at least 1")
    scores: List[float] = []
    dev = model.device
    with torch.cuda.device(dev):
        at = 0
        while at < len(pairs):                                 # runs of one shape, each uploaded in chunks
            shape = pairs[at][0].shape
            end = at
            while end < len(pairs) and pairs[end][0].shape == shape:
                end += 1
            step = int(chunk_frames) if chunk_frames is not None else max(1, LPIPS_CHUNK_BYTES // (2 * int(np.prod(shape))))
            for lo in range(at, end, step):
                part = pairs[lo:min(end, lo + step)]
                a = torch.from_numpy(np.ascontiguousarray(np.stack([p[0] for p in part]))).to(dev)
                b = torch.from_numpy(np.ascontiguousarray(np.stack([p[1] for p in part]))).to(dev)
                scores.extend(float(v) for v in lpips_device(a, b, model, order=order).cpu())
            at = end
    return scores


def calculate_lpips_per_frame(reference_frames: Sequence[Optional[np.ndarray]], decoded_frames: Sequence[Optional[np.ndarray]],
                              device="cuda:0", model: Optional[LpipsAlex] = None, chunk_frames: Optional[int] = None) -> List[float]:
    """elvis.py:3163-3195: the score of every aligned pair of BGR frames; a pair with a None is skipped, empty input
    gives [].  `model` defaults to `get_lpips_model(device)`; the clip is uploaded `chunk_frames` pairs at a time (by
    default about 64 MB) and the scores are the same bytes at every chunk size.  BUILD-DEFINED (module docstring)."""
    if reference_frames is None or decoded_frames is None or len(reference_frames) == 0 or len(decoded_frames) == 0:
        return []
    pairs = _pairs(reference_frames, decoded_frames)
    if not pairs:
        return []
    return _score_pairs(pairs, get_lpips_model(device) if model is None else model, "bgr", chunk_frames)


def calculate_lpips(reference_frames, decoded_frames, model: LpipsAlex) -> List[float]:
    """presley.py:329-357: the same loop with the model passed in."""
    if len(reference_frames) == 0 or len(decoded_frames) == 0:
        return []
    pairs = _pairs(reference_frames, decoded_frames)
    return _score_pairs(pairs, model, "bgr", None) if pairs else []
