"""numpy / scipy restatement of the reference's quality report, importable without a GPU (float64 unless noted).

  luma_bgr, skimage_ssim_gaussian, masked_ssim     elvis.py:674-721   (cv2.cvtColor + skimage structural_similarity)
  msssim_ssim                                      presley.py:248-259 (pytorch_msssim.ssim, size_average=True)
  mask_bbox, apply_binary_mask, compute_mask_union_bbox, roi_of_bbox   elvis.py:578-624, 3639-3646
  frame_indices, evaluate_fg_bg_metrics            elvis.py:3799-3878
  calculate_foreground_metric, compute_fg_bg_ssim  presley.py:422-445, utils.py:611-656

PARITY UNPINNED against cv2, skimage and pytorch_msssim themselves: the packages are absent, so their published
algorithms are restated here - OpenCV's 8-bit BGR2YCrCb luma rule, skimage's structural_similarity with
gaussian_weights=True and an explicit win_size (the filter is scipy.ndimage.gaussian_filter, sigma 1.5, truncate 3.5,
mode reflect: the call skimage makes), and pytorch_msssim's separable valid window.  tests/golden/quality.npz pins the
reference's control flow around them with the reference's own code (tools/make_quality_golden.py).

`ssim_mean` is the device kernel's contract written tap by tap (no scipy), for any source / border / pad.
"""
import math

import numpy as np

C1_255, C2_255 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
REGIONS = ("foreground", "background")
KEYS = ("psnr_mean", "psnr_std", "ssim_mean", "ssim_std", "mse_mean", "mse_std")


# ----------------------------------------------------------------------------- windows and filters
def gaussian_taps() -> np.ndarray:
    """scipy's gaussian_filter kernel for sigma 1.5, truncate 3.5: radius int(3.5 * 1.5 + 0.5) = 5."""
    x = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-0.5 / (1.5 * 1.5) * x ** 2)
    return g / g.sum()


def msssim_taps() -> np.ndarray:
    """pytorch_msssim's float32 window (size 11, sigma 1.5), up-cast: elvis_amd.metrics.ssim_window() as float64."""
    c = np.arange(11, dtype=np.float32) - 5
    g = np.exp(-(c ** 2) / np.float32(2 * 1.5 ** 2)).astype(np.float32)
    return (g / g.sum()).astype(np.float32).astype(np.float64)


def reflect_index(p, n: int):
    """ndimage `reflect` (d c b a | a b c d), repeated as often as the distance needs."""
    m = np.mod(p, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def _taps_along(x: np.ndarray, w: np.ndarray, axis: int, border: str) -> np.ndarray:
    x = np.moveaxis(x, axis, 0)
    n = x.shape[0]
    if border == "reflect":
        src, m = x[reflect_index(np.arange(-5, n + 5), n)], n
    elif n >= 11:
        src, m = x, n - 10
    else:                                   # valid, shorter than the window: not smoothed
        return np.moveaxis(x, 0, axis)
    out = np.zeros((m,) + x.shape[1:], np.float64)
    for k in range(11):
        out += w[k] * src[k:k + m]
    return np.moveaxis(out, 0, axis)


def filter_taps(x: np.ndarray, w: np.ndarray, border: str = "reflect") -> np.ndarray:
    """The separable 11-tap window, tap by tap: rows (along x) first, then columns, like the device kernel."""
    return _taps_along(_taps_along(np.asarray(x, np.float64), w, 1, border), w, 0, border)


def filter_scipy(x: np.ndarray) -> np.ndarray:
    from scipy.ndimage import gaussian_filter
    return gaussian_filter(np.asarray(x, np.float64), sigma=1.5, truncate=3.5, mode="reflect")


def _ssim_map(x, y, filt, C1, C2, cov_norm):
    ux, uy = filt(x), filt(y)
    uxx, uyy, uxy = filt(x * x), filt(y * y), filt(x * y)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def ssim_mean(x, y, w, border, C1, C2, cov_norm, pad) -> float:
    """Mean over the map shrunk by pad of the windowed SSIM of two float64 planes; 1.0 when nothing is left."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    S = _ssim_map(x, y, lambda v: filter_taps(v, w, border), C1, C2, cov_norm)
    S = S[pad:S.shape[0] - pad, pad:S.shape[1] - pad]
    return float(S.mean()) if S.size else 1.0


# ----------------------------------------------------------------------------- luma SSIM (elvis.py:674-721)
def luma_bgr(img: np.ndarray) -> np.ndarray:
    """OpenCV's 8-bit COLOR_BGR2YCrCb luma: (1868 B + 9617 G + 4899 R + 8192) >> 14."""
    i = img.astype(np.int64)
    return ((1868 * i[..., 0] + 9617 * i[..., 1] + 4899 * i[..., 2] + 8192) >> 14).astype(np.uint8)


def skimage_ssim_gaussian(x: np.ndarray, y: np.ndarray, win_size: int, filt=filter_scipy) -> float:
    """structural_similarity(x, y, data_range=255, gaussian_weights=True, win_size=win_size) on uint8 planes: the
    Gaussian stays sigma 1.5 / radius 5; win_size sets the sample-covariance factor and the cropped border."""
    if min(x.shape) < win_size:
        raise ValueError("win_size exceeds image extent")
    npix = win_size ** 2
    S = _ssim_map(x.astype(np.float64), y.astype(np.float64), filt, C1_255, C2_255, npix / (npix - 1))
    pad = (win_size - 1) // 2
    return float(S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean(dtype=np.float64))


def win_size_for(h: int, w: int):
    """elvis.py:702-711: None when the crop is too small (SSIM reported as 1.0)."""
    s = min(h, w)
    if s < 3:
        return None
    if s >= 7:
        return 7
    return s if s % 2 == 1 else max(3, s - 1)


def mask_bbox(mask) -> tuple:
    """(y0, y1, x0, x1) with exclusive ends; zeros for an empty mask."""
    ys, xs = np.nonzero(np.asarray(mask))
    if not len(ys):
        return (0, 0, 0, 0)
    return (int(ys.min()), int(ys.max()) + 1, int(xs.min()), int(xs.max()) + 1)


def masked_ssim(ref, dec, mask=None, ssim=skimage_ssim_gaussian) -> float:
    a, b = luma_bgr(ref), luma_bgr(dec)
    if mask is not None:
        m = np.asarray(mask).astype(bool)
        if not m.any():
            return 1.0
        y0, y1, x0, x1 = mask_bbox(m)
        a, b, m = a[y0:y1, x0:x1].copy(), b[y0:y1, x0:x1].copy(), m[y0:y1, x0:x1]
        a[~m] = 0
        b[~m] = 0
    win = win_size_for(*a.shape)
    return 1.0 if win is None else float(ssim(a, b, win))


def masked_ssim_taps(ref, dec, mask=None) -> float:
    """masked_ssim with the tap-by-tap filter: the device reference, free of scipy's internals."""
    return masked_ssim(ref, dec, mask, lambda a, b, win: skimage_ssim_gaussian(a, b, win, lambda v: filter_taps(v, gaussian_taps())))


# ----------------------------------------------------------------------------- whole-frame SSIM (presley.py:248-259)
def msssim_ssim(f1: np.ndarray, f2: np.ndarray, data_range: float = 255.0) -> float:
    """pytorch_msssim.ssim(x / data_range, y / data_range, data_range=1, size_average=True) in float64: valid window,
    a dimension shorter than 11 is not smoothed, mean over the map, then over channels (oracle.glue_ref.block_ssim's
    arithmetic for a frame of any H x W)."""
    w = msssim_taps()
    a, b = f1.astype(np.float64) / data_range, f2.astype(np.float64) / data_range
    return float(np.mean([ssim_mean(a[..., c], b[..., c], w, "valid", 0.01 ** 2, 0.03 ** 2, 1.0, 0) for c in range(f1.shape[2])]))


# ----------------------------------------------------------------------------- PSNR / MSE (float32, as the reference)
def masked_mse(ref, dec, mask=None) -> float:
    a, b = ref.astype(np.float32), dec.astype(np.float32)
    if mask is not None:
        v = np.asarray(mask).astype(bool)
        if not v.any():
            return 0.0
        d = a[v] - b[v]
    else:
        d = a - b
    return float(np.mean(d ** 2)) if d.size else 0.0


def masked_psnr(ref, dec, mask=None) -> float:
    if mask is not None and not np.asarray(mask).astype(bool).any():
        return 100.0
    mse = masked_mse(ref, dec, mask)
    return 100.0 if mse < 1e-10 else float(min(20 * math.log10(255.0 / math.sqrt(mse)), 100.0))


def calculate_mse(refs, dists):
    return [float(np.mean((a.astype(np.float32) - b.astype(np.float32)) ** 2)) for a, b in zip(refs, dists)]


def calculate_psnr(refs, dists, data_range=255.0):
    return [float("inf") if m == 0 else float(10 * np.log10(data_range ** 2 / m)) for m in calculate_mse(refs, dists)]


def calculate_ssim(refs, dists, data_range=255.0):
    return [msssim_ssim(a, b, data_range) for a, b in zip(refs, dists)]


# ----------------------------------------------------------------------------- masks and boxes
def apply_binary_mask(frame, mask, invert=False):
    m = np.asarray(mask).astype(bool)
    out = np.zeros_like(frame)
    keep = ~m if invert else m
    out[keep] = frame[keep]
    return out


def compute_mask_union_bbox(masks, width, height, padding_ratio=0.05):
    """elvis.py:578-612 -> (x, y, w, h); the whole frame for no masks or an empty union."""
    union = np.zeros((height, width), bool)
    for m in masks:
        if m is not None:
            union |= np.asarray(m).astype(bool)
    if not union.any():
        return (0, 0, width, height)
    y0, y1, x0, x1 = mask_bbox(union)
    bh, bw = y1 - y0, x1 - x0
    py, px = max(1, int(bh * padding_ratio)), max(1, int(bw * padding_ratio))
    y, x = max(0, y0 - py), max(0, x0 - px)
    return (x, y, min(width - x, bw + 2 * px), min(height - y, bh + 2 * py))


def roi_of_bbox(bbox, width, height):
    """elvis.py:3639-3646 -> (y_start, y_stop, x_start, x_stop)."""
    x, y, w, h = bbox
    return (y, min(height, y + max(1, h)), x, min(width, x + max(1, w)))


def nearest_resize(m: np.ndarray, h: int, w: int) -> np.ndarray:
    """cv2.resize(..., INTER_NEAREST): source index floor(dst * src_n / dst_n)."""
    return m[(np.arange(h) * m.shape[0]) // h][:, (np.arange(w) * m.shape[1]) // w]


def calculate_foreground_metric(refs, dists, fg_masks, metric_func):
    out = []
    for r, d, m in zip(refs, dists, fg_masks):
        binary = nearest_resize(np.asarray(m), r.shape[0], r.shape[1]) >= 0.5
        if not binary.any():
            continue
        y0, y1, x0, x1 = mask_bbox(binary)
        out.append(metric_func([r[y0:y1, x0:x1]], [d[y0:y1, x0:x1]])[0])
    return out


def compute_fg_bg_ssim(ssim_maps, foreground_masks, fg_threshold=0.5):
    all_v, fg_v, bg_v = [], [], []
    for i, s in enumerate(ssim_maps):
        m = foreground_masks[i] if i < len(foreground_masks) else foreground_masks[0]
        if m.shape != s.shape:
            m = nearest_resize(m.astype(np.float32), s.shape[0], s.shape[1])
        fg = m >= fg_threshold
        all_v.extend(s.flatten())
        if fg.any():
            fg_v.extend(s[fg])
        if (~fg).any():
            bg_v.extend(s[~fg])
    overall = float(np.mean(all_v)) if all_v else 0.0
    return overall, float(np.mean(fg_v)) if fg_v else overall, float(np.mean(bg_v)) if bg_v else overall


# ----------------------------------------------------------------------------- the evaluator (elvis.py:3799-3878)
def frame_indices(frame_count: int, metric_stride: int):
    idx = list(range(0, frame_count, metric_stride)) or [0]
    if idx[-1] != frame_count - 1:
        idx.append(frame_count - 1)
    return sorted(set(idx))


def aggregate(per_region: dict) -> dict:
    """{region: {metric: [values]}} -> the nested mean / std dict of elvis.py:3862-3878."""
    return {r: {f"{k}_{s}": (float(getattr(np, s)(v[k])) if v[k] else 0.0) for k in ("psnr", "ssim", "mse") for s in ("mean", "std")}
            for r, v in per_region.items()}


def evaluate_fg_bg_metrics(refs, decs, fg_masks, metric_stride=1, ssim=masked_ssim):
    count = min(len(refs), len(decs))
    h, w = refs[0].shape[:2]
    fg = [np.asarray(m).astype(bool) for m in fg_masks]
    y0, y1, x0, x1 = roi_of_bbox(compute_mask_union_bbox(fg, w, h), w, h)
    vals = {r: {"psnr": [], "ssim": [], "mse": []} for r in REGIONS}
    for i in frame_indices(count, metric_stride):
        rr, dr, mr = refs[i][y0:y1, x0:x1], decs[i][y0:y1, x0:x1], fg[i][y0:y1, x0:x1]
        for region, (a, b, m) in (("foreground", (rr, dr, mr)), ("background", (refs[i], decs[i], ~fg[i]))):
            vals[region]["psnr"].append(masked_psnr(a, b, m))
            vals[region]["ssim"].append(ssim(a, b, m))
            vals[region]["mse"].append(masked_mse(a, b, m))
    return aggregate(vals)


def flatten_result(result: dict) -> np.ndarray:
    return np.asarray([[result[r][k] for k in KEYS] for r in REGIONS], np.float64)
