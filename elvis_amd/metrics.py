"""On-device quality metrics of the parity / quality report: whole-frame and masked MSE / PSNR
(integer-exact sums of squared differences on the device, the reference's formulas on the host) and per-block SSIM.

  calculate_mse / calculate_psnr   presley.py:226-245  (PSNR = 10 log10(range^2 / mse), inf at mse == 0)
  masked_mse / masked_psnr         elvis.py:627-671    (PSNR = 20 log10(255 / sqrt(mse)) capped at 100 dB)
  calculate_block_ssim             utils.py:572-608    (pytorch_msssim.ssim per block; restated, package absent)

and the quality report of the evaluation loop (float64 windowed SSIM on the device, csrc/quality.hip):

  masked_ssim                      elvis.py:674-721    (skimage Gaussian SSIM on masked luma, cropped to the mask's box)
  calculate_ssim                   presley.py:248-259  (pytorch_msssim.ssim of whole frames)
  calculate_foreground_metric      presley.py:422-445  (a metric on the foreground's bounding box)
  compute_fg_bg_ssim               utils.py:611-656    (host arithmetic on block SSIM maps)
  apply_binary_mask, compute_mask_union_bbox           elvis.py:578-624
  evaluate_fg_bg_metrics           elvis.py:3799-3878  (the numeric core of _evaluate_single_video_metrics)

cv2, skimage and pytorch_msssim are absent: parity with the packages themselves is unpinned; what is
pinned is their published arithmetic (tests/_quality_ref.py) and the reference's own control flow (tests/golden/quality.npz).
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import ops
from ._lib import check, lib, ptr
from .recompose import frames_to_device
from .tiler import _nearest_rows


def _sse(reference_frames, distorted_frames, device, masks=None):
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        a, b = frames_to_device(list(reference_frames), dev), frames_to_device(list(distorted_frames), dev)
        if a.shape != b.shape:
            raise ValueError("frame sequences differ in shape")
        m = None
        if masks is not None:
            m = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(k).astype(bool) for k in masks]).astype(np.uint8))).to(dev)
        sse, cnt = ops.sse_u8(a, b, m)
        return sse.cpu().numpy(), cnt.cpu().numpy()


def calculate_mse(reference_frames: Sequence[np.ndarray], distorted_frames: Sequence[np.ndarray], device="cuda:0") -> List[float]:
    """Per-frame MSE (presley.py:226-232)."""
    if not len(reference_frames):
        return []
    sse, cnt = _sse(reference_frames, distorted_frames, device)
    return [float(s) / float(c) for s, c in zip(sse, cnt)]


def calculate_psnr(reference_frames, distorted_frames, data_range: float = 255.0, device="cuda:0") -> List[float]:
    """Per-frame PSNR, 10 log10(data_range^2 / mse), inf for identical frames (presley.py:235-245)."""
    return [float("inf") if m == 0 else 10.0 * math.log10(data_range ** 2 / m)
            for m in calculate_mse(reference_frames, distorted_frames, device)]


def masked_mse(ref: np.ndarray, dec: np.ndarray, mask: Optional[np.ndarray] = None, device="cuda:0") -> float:
    """elvis.py:653-671: MSE over the masked pixels (all channels), 0.0 for an empty mask."""
    sse, cnt = _sse([ref], [dec], device, None if mask is None else [mask])
    return 0.0 if cnt[0] == 0 else float(sse[0]) / float(cnt[0])


def masked_psnr(ref: np.ndarray, dec: np.ndarray, mask: Optional[np.ndarray] = None, device="cuda:0") -> float:
    """elvis.py:627-650: 20 log10(255 / sqrt(mse)) capped at 100 dB; 100 for an empty mask or mse < 1e-10."""
    if mask is not None and not np.any(np.asarray(mask).astype(bool)):
        return 100.0
    mse = masked_mse(ref, dec, mask, device)
    return 100.0 if mse < 1e-10 else float(min(20.0 * math.log10(255.0 / math.sqrt(mse)), 100.0))


def ssim_window(size: int = 11, sigma: float = 1.5) -> np.ndarray:
    coords = np.arange(size, dtype=np.float32) - size // 2
    g = np.exp(-(coords ** 2) / np.float32(2 * sigma ** 2)).astype(np.float32)
    return (g / g.sum()).astype(np.float32)


def block_ssim_device(a: torch.Tensor, b: torch.Tensor, block_size: int) -> torch.Tensor:
    """[n,H,W,C] uint8 x2 on the device -> float32 [n, H // b, W // b]."""
    ops._chk_u8(a, b)
    if a.shape != b.shape:
        raise ValueError("frame tensors differ in shape")
    n, h, w, c = a.shape
    out = torch.empty((n, h // block_size, w // block_size), dtype=torch.float32, device=a.device)
    win = torch.from_numpy(ssim_window()).to(a.device)
    check(lib().elvis_block_ssim_u8(ptr(a), ptr(b), ptr(out), ptr(win), n, h, w, c, block_size, ops._s(a)), a.device)
    return out


def calculate_block_ssim(frames1: Sequence[np.ndarray], frames2: Sequence[np.ndarray], block_size: int,
                         device="cuda:0") -> List[np.ndarray]:
    """Per-block SSIM maps (utils.py:572-608), one (H // b, W // b) float32 array per frame pair."""
    if not len(frames1):
        return []
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        m = block_ssim_device(frames_to_device(list(frames1), dev), frames_to_device(list(frames2), dev), block_size).cpu().numpy()
    return [m[i] for i in range(m.shape[0])]


# ----------------------------------------------------------------------------- quality report (csrc/quality.hip)
SSIM_C1_255, SSIM_C2_255 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def gaussian_window() -> np.ndarray:
    """The float64 window skimage's gaussian_weights=True applies: sigma 1.5, truncate 3.5 -> radius 5, normalised."""
    x = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-0.5 / (1.5 * 1.5) * x ** 2)
    return g / g.sum()


def _chk_masks(masks: torch.Tensor, a: torch.Tensor) -> None:
    ops._chk_u8(masks)
    if masks.dim() != 3 or tuple(masks.shape) != tuple(a.shape[:3]):
        raise ValueError(f"mask {tuple(masks.shape)} does not match frames {tuple(a.shape)}")


def _chk_mask_shapes(masks: Sequence[np.ndarray], shape) -> None:
    for m in masks:
        if np.asarray(m).shape != tuple(shape):
            raise ValueError(f"mask {np.asarray(m).shape} does not match frame {tuple(shape)}")


def masks_to_device(masks: Sequence[np.ndarray], shape, dev) -> torch.Tensor:
    """Boolean-ised masks (non-zero = set) as one [n,H,W] uint8 tensor; every mask must have the frames' H x W."""
    ms = [np.asarray(m) for m in masks]
    _chk_mask_shapes(ms, shape)
    return torch.from_numpy(np.ascontiguousarray(np.stack([m.astype(bool) for m in ms]).astype(np.uint8))).to(dev)


def mask_bbox_device(masks: torch.Tensor) -> torch.Tensor:
    """[n,H,W] uint8 -> int32 [n,4] = y0, y1, x0, x1 (exclusive ends), zeros for an empty mask."""
    ops._chk_u8(masks)
    if masks.dim() != 3:
        raise ValueError("masks must be [n,H,W]")
    n, h, w = masks.shape
    out = torch.empty((n, 4), dtype=torch.int32, device=masks.device)
    check(lib().elvis_mask_bbox_u8(ptr(masks), ptr(out), n, h, w, ops._s(masks)), masks.device)
    return out


def apply_mask_device(frames: torch.Tensor, masks: torch.Tensor, invert: bool = False) -> torch.Tensor:
    """out = mask ? frame : 0 (the other way round with invert) on [n,H,W,C] / [n,H,W] uint8 tensors."""
    ops._chk_u8(frames)
    if frames.dim() != 4:
        raise ValueError("frames must be [n,H,W,C]")
    _chk_masks(masks, frames)
    n, h, w, c = frames.shape
    out = torch.empty_like(frames)
    check(lib().elvis_apply_mask_u8(ptr(frames), ptr(masks), ptr(out), n, h, w, c, int(bool(invert)), ops._s(frames)), frames.device)
    return out


def ssim_mean_device(a: torch.Tensor, b: torch.Tensor, window: np.ndarray, *, source: int, border: int, C1: float, C2: float,
                     cov_norm: float = 1.0, pad: int = 0, scale: float = 1.0, masks: Optional[torch.Tensor] = None,
                     rects: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The windowed SSIM mean (elvis_ssim_mean_f64) -> float64 [n, C], C = 1 for the luma source."""
    ops._chk_u8(a, b)
    if a.dim() != 4 or a.shape != b.shape:
        raise ValueError("frame tensors must be [n,H,W,C] and equal in shape")
    n, h, w, c = a.shape
    if source == L.SSIM_LUMA and c != 3:
        raise ValueError(f"the luma SSIM needs 3-channel BGR frames, got {c} channels")
    if masks is not None:
        _chk_masks(masks, a)
    if rects is not None and (rects.dtype != torch.int32 or tuple(rects.shape) != (n, 4) or not rects.is_contiguous()):
        raise ValueError("rects must be contiguous int32 [n,4]")
    window = np.ascontiguousarray(window, dtype=np.float64)
    if window.shape != (11,):
        raise ValueError("the SSIM window has 11 taps")
    win = torch.from_numpy(window).to(a.device)
    ws = torch.empty(max(1, lib().elvis_ssim_workspace_bytes(n, h, w, c) // 8), dtype=torch.float64, device=a.device)
    out = torch.empty((n, 1 if source == L.SSIM_LUMA else c), dtype=torch.float64, device=a.device)
    check(lib().elvis_ssim_mean_f64(ptr(a), ptr(b), ptr(masks), ptr(rects), ptr(win), ptr(ws), ptr(out), n, h, w, c, source, border,
                                    float(C1), float(C2), float(cov_norm), int(pad), float(scale), ops._s(a)), a.device)
    return out


def masked_ssim_device(a: torch.Tensor, b: torch.Tensor, masks: Optional[torch.Tensor]) -> torch.Tensor:
    """elvis.py:674-721 for a batch: [n,H,W,3] BGR uint8 x2 and [n,H,W] uint8 masks (None: whole frames) -> float64 [n].
    Two steps on the device and no host round trip: the masks' bounding boxes, then the SSIM over each frame's own box
    with the window rule of elvis.py:702-711 taken per frame (an empty mask or a box under 3 pixels reports 1.0)."""
    rects = None if masks is None else mask_bbox_device(masks)
    return ssim_mean_device(a, b, gaussian_window(), source=L.SSIM_LUMA, border=L.SSIM_REFLECT, C1=SSIM_C1_255, C2=SSIM_C2_255,
                            pad=L.SSIM_PAD_AUTO, masks=masks, rects=rects)[:, 0]


def calculate_ssim_device(a: torch.Tensor, b: torch.Tensor, data_range: float = 255.0) -> torch.Tensor:
    """presley.py:248-259 for a batch: [n,H,W,C] uint8 x2 -> float64 [n] (mean over the channels' SSIM means)."""
    per_channel = ssim_mean_device(a, b, ssim_window().astype(np.float64), source=L.SSIM_CHANNELS, border=L.SSIM_VALID,
                                   C1=0.01 ** 2, C2=0.03 ** 2, cov_norm=1.0, pad=0, scale=float(data_range))
    return per_channel.mean(dim=1)


def _frame_pair(ref, dec):
    ref, dec = np.asarray(ref), np.asarray(dec)
    if ref.shape != dec.shape:
        raise ValueError(f"frames differ in shape: {ref.shape} vs {dec.shape}")
    if ref.ndim != 3:
        raise ValueError("frames must be H x W x C")
    return ref, dec


def masked_ssim(ref: np.ndarray, dec: np.ndarray, mask: Optional[np.ndarray] = None, device="cuda:0") -> float:
    """elvis.py:674-721: SSIM of the luma channel inside the mask's bounding box, pixels outside the mask zeroed;
    1.0 for an empty mask or a box with a side under 3."""
    ref, dec = _frame_pair(ref, dec)
    if ref.shape[2] != 3:
        raise ValueError(f"the luma SSIM needs 3-channel BGR frames, got {ref.shape[2]} channels")
    if mask is not None and np.asarray(mask).shape != ref.shape[:2]:
        raise ValueError(f"mask {np.asarray(mask).shape} does not match frame {ref.shape[:2]}")
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        m = None if mask is None else masks_to_device([mask], ref.shape[:2], dev)
        return float(masked_ssim_device(frames_to_device([ref], dev), frames_to_device([dec], dev), m).cpu()[0])


def calculate_ssim(reference_frames: Sequence[np.ndarray], distorted_frames: Sequence[np.ndarray], data_range: float = 255.0,
                   device="cuda:0") -> List[float]:
    """Per-frame whole-frame SSIM (presley.py:248-259)."""
    pairs = [_frame_pair(a, b) for a, b in zip(reference_frames, distorted_frames)]
    if not pairs:
        return []
    if any(p[0].shape != pairs[0][0].shape for p in pairs):
        raise ValueError("frame sequences differ in shape")
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        a, b = frames_to_device([p[0] for p in pairs], dev), frames_to_device([p[1] for p in pairs], dev)
        return [float(v) for v in calculate_ssim_device(a, b, data_range).cpu()]


def _box(present_rows: np.ndarray, present_cols: np.ndarray) -> Tuple[int, int, int, int]:
    ys, xs = np.nonzero(present_rows)[0], np.nonzero(present_cols)[0]
    return int(ys[0]), int(ys[-1]) + 1, int(xs[0]), int(xs[-1]) + 1


def calculate_foreground_metric(reference_frames: Sequence[np.ndarray], distorted_frames: Sequence[np.ndarray],
                                foreground_masks: Sequence[np.ndarray], metric_func: Callable, device="cuda:0") -> List[float]:
    """presley.py:422-445: the block-grid mask is INTER_NEAREST-resized to the frame (the index rule of
    tiler.blended_restoration), thresholded at >= 0.5, and metric_func runs on the frames cropped to the foreground's
    bounding box; a frame without foreground is skipped.  A nearest-resized mask's box follows from the rows and
    columns of the grid that hold foreground, so the full-size mask is never built."""
    own = metric_func in (calculate_mse, calculate_psnr, calculate_ssim)
    values = []
    for ref, dist, fg in zip(reference_frames, distorted_frames, foreground_masks):
        ref, dist = _frame_pair(ref, dist)
        fg = np.asarray(fg)
        if fg.ndim != 2:
            raise ValueError("a foreground mask is a 2-D block-grid map")
        binary = fg >= 0.5
        if not binary.any():
            continue
        h, w = ref.shape[:2]
        y0, y1, x0, x1 = _box(binary.any(axis=1)[_nearest_rows(fg.shape[0], h)], binary.any(axis=0)[_nearest_rows(fg.shape[1], w)])
        crops = [np.ascontiguousarray(ref[y0:y1, x0:x1])], [np.ascontiguousarray(dist[y0:y1, x0:x1])]
        values.append(metric_func(*crops, device=device)[0] if own else metric_func(*crops)[0])
    return values


def compute_fg_bg_ssim(ssim_maps: Sequence[np.ndarray], foreground_masks: Sequence[np.ndarray],
                       fg_threshold: float = 0.5) -> Tuple[float, float, float]:
    """utils.py:611-656: (overall, foreground, background) means of per-block SSIM maps; a side without blocks takes
    the overall mean.  Host arithmetic on block maps."""
    all_v, fg_v, bg_v = [], [], []
    for i, smap in enumerate(ssim_maps):
        smap = np.asarray(smap)
        m = np.asarray(foreground_masks[i] if i < len(foreground_masks) else foreground_masks[0])
        if m.shape != smap.shape:
            m = m.astype(np.float32)[_nearest_rows(m.shape[0], smap.shape[0])][:, _nearest_rows(m.shape[1], smap.shape[1])]
        fg = m >= fg_threshold
        all_v.extend(smap.flatten())
        fg_v.extend(smap[fg])
        bg_v.extend(smap[~fg])
    overall = float(np.mean(all_v)) if all_v else 0.0
    return overall, float(np.mean(fg_v)) if fg_v else overall, float(np.mean(bg_v)) if bg_v else overall


def apply_binary_mask(frame: np.ndarray, mask: np.ndarray, invert: bool = False, device="cuda:0") -> np.ndarray:
    """elvis.py:615-624: a copy of frame with the pixels outside mask (inside it, with invert) zeroed."""
    if frame is None or mask is None:
        return frame
    frame = np.asarray(frame)
    if frame.ndim != 3 or np.asarray(mask).shape != frame.shape[:2]:
        raise ValueError(f"mask {np.asarray(mask).shape} does not match frame {frame.shape}")
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        out = apply_mask_device(frames_to_device([frame], dev), masks_to_device([mask], frame.shape[:2], dev), invert)
        return out[0].cpu().numpy()


def _padded_union_bbox(boxes: np.ndarray, width: int, height: int, padding_ratio: float) -> Tuple[int, int, int, int]:
    boxes = boxes[boxes[:, 1] > boxes[:, 0]]               # per-frame y0, y1, x0, x1; empty frames drop out
    if not len(boxes):
        return (0, 0, width, height)
    y0, y1, x0, x1 = int(boxes[:, 0].min()), int(boxes[:, 1].max()), int(boxes[:, 2].min()), int(boxes[:, 3].max())
    bh, bw = y1 - y0, x1 - x0
    pad_y, pad_x = max(1, int(bh * padding_ratio)), max(1, int(bw * padding_ratio))
    y, x = max(0, y0 - pad_y), max(0, x0 - pad_x)
    return (x, y, min(width - x, bw + 2 * pad_x), min(height - y, bh + 2 * pad_y))


def compute_mask_union_bbox(masks: Sequence[np.ndarray], width: int, height: int, padding_ratio: float = 0.05,
                            device="cuda:0") -> Tuple[int, int, int, int]:
    """elvis.py:578-612: the padded (x, y, w, h) box over the union of the masks (None entries are skipped), the whole
    frame for no masks or an empty union.  The union's box is the min / max over the per-frame boxes."""
    masks = [m for m in masks if m is not None]
    if not masks:
        return (0, 0, width, height)
    _chk_mask_shapes(masks, (height, width))
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        boxes = mask_bbox_device(masks_to_device(masks, (height, width), dev)).cpu().numpy()
    return _padded_union_bbox(boxes, width, height, padding_ratio)


def metric_frame_indices(frame_count: int, metric_stride: int) -> List[int]:
    """elvis.py:3804-3809: every metric_stride-th frame, and always the last one."""
    idx = list(range(0, frame_count, metric_stride)) or [0]
    if idx[-1] != frame_count - 1:
        idx.append(frame_count - 1)
    return sorted(set(idx))


def evaluate_fg_bg_metrics(reference_frames: Sequence[np.ndarray], decoded_frames: Sequence[np.ndarray],
                           fg_masks: Sequence[np.ndarray], metric_stride: int = 1, device="cuda:0",
                           lpips_model=None, vmaf_model=None, fvmd=None) -> Dict[str, Dict[str, float]]:
    """The numeric core of _evaluate_single_video_metrics (elvis.py:3799-3878): masked PSNR, SSIM and MSE of the
    sampled frames, foreground (inside fg_masks) and background (outside), each as _mean and _std.  Bitrate keys are not
    produced; LPIPS, VMAF and FVMD keys only on request (below).  Per-frame MSE is a float32 number, as the reference's is.
    With `lpips_model` (an `elvis_amd.lpips.LpipsAlex` on `device`) both regions gain `lpips_mean` / `lpips_std` as
    elvis.py:3853-3893 forms them, on the tensors already uploaded: the foreground from the fg-masked frames cropped to
    the ROI around the union of all foreground masks (elvis.py:3639-3646), the background from the bg-masked whole
    frames.  An ROI under 31 x 31 raises ValueError.  Without it (None) the result is what it was.
    With `vmaf_model` (an `elvis_amd.vmaf.VmafModel`) both regions gain `vmaf_mean` / `vmaf_std`, on the same tensors and
    the same two regions: the luma (`vmaf.luma_device`, order "bgr") of the fg-masked frames cropped to that ROI, and of
    the bg-masked whole frames; motion runs between consecutive sampled frames.  The reference squeezes these masked
    clips through a lossy x264 encode before it scores them (elvis.py:3895-3929); that encode is NOT reproduced.  An ROI
    under 64 x 64 raises ValueError.  Without it (None) the result is what it was.
    With `fvmd` (an `elvis_amd.fvmd.FvmdConfig`, or True for the default one) both regions gain `fvmd` / `fvmd_std`, the
    reference's key names (elvis.py:4035-4038), from `fvmd.calculate_fvmd_device` on the luma of the same masked tensors
    and the same two regions.  The reference's frame sampling is kept (elvis.py:3954-3981): the config's `stride` is
    lowered until ten frames are sampled, `max_frames` cuts the list, and with fewer than ten sampled frames both keys
    are NaN (elvis.py:3882-3885).  BUILD-DEFINED: the score is this build's KLT restatement and does NOT claim parity with
    the `fvmd` package (elvis_amd/fvmd.py).  An ROI under 64 x 64 raises ValueError.  Without it (None) the result is
    what it was."""
    if metric_stride < 1:
        raise ValueError("metric_stride must be at least 1")
    count = min(len(reference_frames), len(decoded_frames))
    if count == 0:
        raise ValueError("no frames to evaluate")
    if len(fg_masks) < count:
        raise ValueError(f"{len(fg_masks)} masks for {count} frames")
    idx = metric_frame_indices(count, metric_stride)
    refs, decs = zip(*[_frame_pair(reference_frames[i], decoded_frames[i]) for i in idx])
    if refs[0].shape[2] != 3:
        raise ValueError(f"the luma SSIM needs 3-channel BGR frames, got {refs[0].shape[2]} channels")
    if any(r.shape != refs[0].shape for r in refs):
        raise ValueError("frame sequences differ in shape")
    _chk_mask_shapes([fg_masks[i] for i in idx], refs[0].shape[:2])
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        a, b = frames_to_device(list(refs), dev), frames_to_device(list(decs), dev)          # uploaded once
        fg = masks_to_device([fg_masks[i] for i in idx], refs[0].shape[:2], dev)
        bg = 1 - fg
        # The reference evaluates the foreground on the ROI around the union of all foreground masks (elvis.py:3639-3646,
        # 3846-3852).  Every foreground mask lies inside that ROI, so masked sums and counts over the ROI equal those over
        # the frame, and _masked_ssim crops to the mask's own box whichever it is given: no crop copy is needed.
        result = {}
        roi = None
        if lpips_model is not None:
            from .lpips import lpips_device
        if vmaf_model is not None:
            from .vmaf import luma_device, vmaf_device
        fvmd_idx = None
        if fvmd is not None and fvmd is not False:
            from . import fvmd as _fvmd
            from .vmaf import luma_device
            fvmd_cfg = _fvmd.FvmdConfig() if fvmd is True else fvmd
            if not isinstance(fvmd_cfg, _fvmd.FvmdConfig):
                raise ValueError("fvmd must be None, True or an elvis_amd.fvmd.FvmdConfig")
            fvmd_idx = _fvmd_sample_indices(len(idx), fvmd_cfg.stride, fvmd_cfg.max_frames)
        if lpips_model is not None or vmaf_model is not None or fvmd_idx is not None:
            h, w = refs[0].shape[:2]
            bx, by, bw, bh = compute_mask_union_bbox(list(fg_masks[:count]), w, h, device=dev)
            roi = (by, min(h, by + max(1, bh)), bx, min(w, bx + max(1, bw)))
        for region, m in (("foreground", fg), ("background", bg)):
            sse, cnt = (t.cpu().numpy() for t in ops.sse_u8(a, b, m))
            ssim = masked_ssim_device(a, b, m).cpu().numpy()
            # The reference's per-frame MSE is a float32 number (np.mean of float32 squares, elvis.py:670), and the _std
            # keys magnify a per-frame rounding by mean / std.  So the exact sum is divided and rounded once in float32:
            # numpy's float32 mean itself while the sum of squares stays below 2^24 (its partial sums are then exact),
            # within float32 summation error of it on larger frames.  PSNR follows from that number, as in the reference.
            mse = [0.0 if k == 0 else float(np.float32(s) / np.float32(k)) for s, k in zip(sse, cnt)]
            psnr = [100.0 if k == 0 or e < 1e-10 else float(min(20.0 * math.log10(255.0 / math.sqrt(e)), 100.0)) for e, k in zip(mse, cnt)]
            result[region] = {f"{name}_{stat}": float(getattr(np, stat)(vals))
                              for name, vals in (("psnr", psnr), ("ssim", [float(v) for v in ssim]), ("mse", mse)) for stat in ("mean", "std")}
            if lpips_model is not None:
                scores = lpips_device(a, b, lpips_model, masks=m, rect=roi if region == "foreground" else None, order="bgr").cpu().numpy()
                result[region]["lpips_mean"], result[region]["lpips_std"] = float(np.mean(scores)), float(np.std(scores))
            if vmaf_model is not None:
                rect = roi if region == "foreground" else None
                scores = vmaf_device(luma_device(a, "bgr", masks=m, rect=rect), luma_device(b, "bgr", masks=m, rect=rect),
                                     vmaf_model).cpu().numpy()
                result[region]["vmaf_mean"], result[region]["vmaf_std"] = float(np.mean(scores)), float(np.std(scores))
            if fvmd_idx is not None:
                value, std = float("nan"), float("nan")                     # elvis.py:3882-3885
                if len(fvmd_idx) >= 10:
                    rect = roi if region == "foreground" else None
                    planes = [luma_device(t, "bgr", masks=m, rect=rect) for t in (a, b)]
                    if fvmd_idx != list(range(len(idx))):
                        at = torch.as_tensor(fvmd_idx, dtype=torch.long, device=dev)
                        planes = [p.index_select(0, at) for p in planes]
                    value, std = _fvmd.calculate_fvmd_device(planes[0], planes[1], fvmd_cfg, stride=1, max_frames=None,
                                                             early_stop_delta=fvmd_cfg.early_stop_delta,
                                                             early_stop_window=fvmd_cfg.early_stop_window)
                result[region]["fvmd"], result[region]["fvmd_std"] = value, std
        return result


def _fvmd_sample_indices(frame_count: int, fvmd_stride: int, fvmd_max_frames: Optional[int]) -> List[int]:
    """elvis.py:3954-3976: the frames FVMD is given - the stride lowered so that ten frames are sampled where the clip
    has them, then `max_frames`."""
    min_fvmd_samples = 10
    total_available_frames = frame_count
    if fvmd_max_frames is not None and fvmd_max_frames > 0:
        total_available_frames = min(total_available_frames, fvmd_max_frames)
    effective_stride = max(1, fvmd_stride)
    if total_available_frames >= min_fvmd_samples:
        effective_stride = min(effective_stride, max(1, total_available_frames // min_fvmd_samples))
    else:
        effective_stride = 1
    fvmd_indices = list(range(0, frame_count, effective_stride)) or [0]
    if fvmd_max_frames is not None and fvmd_max_frames > 0:
        fvmd_indices = fvmd_indices[:fvmd_max_frames]
    return fvmd_indices
