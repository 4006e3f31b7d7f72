"""The VMAF contract in numpy float64 (include/elvis_amd.h): VIF on four scales, ADM2 on four scales,
motion2 and the nu-SVR score over them.  BUILD-DEFINED: a restatement of the published float feature extractors, not
libvmaf's numbers.  Explicit tap loops, no BLAS / tensordot / convolve: a filter is ((f0 x0 + f1 x1) + f2 x2) + ... in
ascending tap order, the vertical pass first, mirror border without repeating the edge - the one order the kernels of
csrc/vmaf.hip evaluate in, so every branch falls the same way on both sides."""
import math
from functools import lru_cache

import numpy as np

MIN_SIDE = 64
EPS, NSQ, GAIN_LIMIT = 1e-10, 2.0, 100.0
VIF_TAPS = (17, 9, 5, 3)
FEATURES = ("adm2", "motion2", "vif_scale0", "vif_scale1", "vif_scale2", "vif_scale3")
BAR = 1e-9                                        # |device - statement| <= BAR * max(1, |statement|)
SHAPES = ((64, 64), (66, 70), (71, 93), (270, 480))
FRAMES = 3
PASS_FRAMES, TILE_H = 4, 16                       # VMAF_PASS_FRAMES and VMAF_TH of csrc/vmaf.hip, for the mutants below
# One clause of the statement changed, selected by `mutant=`; the kernels are never changed.  tests/_vmafcases.py names
# the case each must move by a thousand bars.
MUTANTS = ("mirror_repeats_edge", "decimate_odd", "adm_window_floor", "adm_threshold_no_centre", "motion2_before",
           "vif_tile_row_more", "pass2_from_0", "adm_hw_swapped")

CSF_A = ((0.62171, 0.67234, 0.72709, 0.67234), (0.34537, 0.41317, 0.49428, 0.41317), (0.18004, 0.22727, 0.28688, 0.22727),
         (0.091401, 0.11792, 0.15214, 0.11792))
CSF_G = (1.501, 1.0, 0.534, 1.0)


# ----------------------------------------------------------------------------- the tables
def gaussian(n: int) -> np.ndarray:
    k = np.arange(n, dtype=np.float64) - n // 2
    g = np.exp(-(k * k) / (2.0 * (n / 5.0) ** 2))
    return g / g.sum()


def blur5() -> np.ndarray:
    k = np.arange(5, dtype=np.float64) - 2
    g = np.exp(-(k * k) / 2.0)
    return g / g.sum()


def db2():
    r3, d = math.sqrt(3.0), 4.0 * math.sqrt(2.0)
    lo = np.asarray([(1 + r3) / d, (3 + r3) / d, (3 - r3) / d, (1 - r3) / d], np.float64)
    hi = np.asarray([lo[3], -lo[2], lo[1], -lo[0]], np.float64)
    return lo, hi


def csf_q(lam: int, theta: int) -> float:
    r = 3.0 * 1080.0 * math.pi / 180.0
    return 2.0 * 0.495 * 10.0 ** (0.466 * math.log10(2.0 ** lam * 0.401 * CSF_G[theta] / r) ** 2) / CSF_A[lam - 1][theta]


COS2 = math.cos(math.pi / 180.0) ** 2


def tables() -> np.ndarray:
    """The 56 constants the kernels are handed, in their order."""
    lo, hi = db2()
    csf = [1.0 / csf_q(s + 1, th) for s in range(4) for th in (1, 2)]
    return np.concatenate([gaussian(17), gaussian(9), gaussian(5), gaussian(3), blur5(), lo, hi, [COS2], csf]).astype(np.float64)


# ----------------------------------------------------------------------------- filters
def reflect(idx: np.ndarray, n: int, mutant=None) -> np.ndarray:
    if mutant == "mirror_repeats_edge":
        idx = np.where(idx < 0, -idx - 1, idx)
        return np.where(idx >= n, 2 * n - 1 - idx, idx)
    idx = np.abs(idx)
    return np.where(idx >= n, 2 * n - 2 - idx, idx)


def filt(x: np.ndarray, f: np.ndarray, axis: int, mutant=None) -> np.ndarray:
    """Same-size filter along one axis, centred, mirror border."""
    n, r = x.shape[axis], len(f) // 2
    acc = None
    for k in range(len(f)):
        term = f[k] * np.take(x, reflect(np.arange(n) + k - r, n, mutant), axis=axis)
        acc = term if acc is None else acc + term
    return acc


def filt2(x: np.ndarray, f: np.ndarray, mutant=None) -> np.ndarray:
    return filt(filt(x, f, -2, mutant), f, -1, mutant)


def dwt_axis(x: np.ndarray, f: np.ndarray, axis: int, mutant=None) -> np.ndarray:
    n = x.shape[axis]
    m = (n + 1) // 2
    acc = None
    for k in range(4):
        term = f[k] * np.take(x, reflect(2 * np.arange(m) + k - 1, n, mutant), axis=axis)
        acc = term if acc is None else acc + term
    return acc


def planes(y: np.ndarray) -> np.ndarray:
    y = np.asarray(y)
    if y.dtype != np.uint8 or y.ndim != 3:
        raise ValueError("vmaf: luma must be uint8 [F, H, W]")
    if y.shape[1] < MIN_SIDE or y.shape[2] < MIN_SIDE:
        raise ValueError(f"vmaf: a {y.shape[1]} x {y.shape[2]} plane is smaller than {MIN_SIDE} x {MIN_SIDE}")
    return y.astype(np.float64) - 128.0


# ----------------------------------------------------------------------------- VIF
def vif(ref: np.ndarray, dis: np.ndarray, counts=None, mutant=None) -> np.ndarray:
    """[F,H,W] u8 x2 -> [F,4]."""
    first = 1 if mutant == "decimate_odd" else 0
    x, y = planes(ref), planes(dis)
    out = np.empty((x.shape[0], 4), np.float64)
    for s, taps in enumerate(VIF_TAPS):
        g = gaussian(taps)
        if s:
            h, w = x.shape[1] // 2, x.shape[2] // 2
            x, y = filt2(x, g, mutant)[:, first::2, first::2][:, :h, :w], filt2(y, g, mutant)[:, first::2, first::2][:, :h, :w]
        mu1, mu2 = filt2(x, g, mutant), filt2(y, g, mutant)
        s1 = np.maximum(filt2(x * x, g, mutant) - mu1 * mu1, 0.0)
        s2 = np.maximum(filt2(y * y, g, mutant) - mu2 * mu2, 0.0)
        s12 = filt2(x * y, g, mutant) - mu1 * mu2
        raw1 = s1
        gain = s12 / (s1 + EPS)
        sv = s2 - gain * s12
        c1 = s1 < EPS
        gain, sv, s1 = np.where(c1, 0.0, gain), np.where(c1, s2, sv), np.where(c1, 0.0, s1)
        c2 = s2 < EPS
        gain, sv = np.where(c2, 0.0, gain), np.where(c2, 0.0, sv)
        c3 = gain < 0.0
        sv, gain = np.where(c3, s2, sv), np.where(c3, 0.0, gain)
        sv = np.maximum(sv, EPS)
        unclamped = gain
        gain = np.minimum(gain, GAIN_LIMIT)
        big = s1 >= NSQ
        safe = np.where(big, s1, NSQ)
        num = np.where(big, np.log2(1.0 + gain * gain * safe / (sv + NSQ)), 1.0 - s2 * 4.0 / 65025.0)
        den = np.where(big, np.log2(1.0 + safe / NSQ), 1.0)
        if counts is not None:
            for name, c in (("s1_below_eps", c1), ("s2_below_eps", c2), ("gain_negative", c3), ("log_term", big), ("flat_term", ~big),
                            ("low_term", ~big & ~c1)):
                counts[name][s] += int(c.sum())
            counts["sv_floored"][s] += int((sv == EPS).sum())
            counts["nsq_margin"][s] = min(counts["nsq_margin"][s], float((np.abs(raw1 - NSQ) / NSQ).min()))
            counts["max_gain_log"][s] = max(counts["max_gain_log"][s], float(np.where(big, unclamped, 0.0).max()))
        if mutant == "vif_tile_row_more" and x.shape[1] % TILE_H:           # the ragged tile's guard one row late: row h is the mirror's
            rows = reflect(np.arange(x.shape[1] + 1), x.shape[1])
            num, den = num[:, rows], den[:, rows]
        n, d = num.sum(axis=(1, 2)), den.sum(axis=(1, 2))
        out[:, s] = np.where(d == 0.0, 1.0, n / np.where(d == 0.0, 1.0, d))
    return out


# ----------------------------------------------------------------------------- motion
def motion(ref: np.ndarray, prev=None, nxt=None, mutant=None):
    """-> (motion [F], motion2 [F]).  prev / nxt: the u8 [H,W] plane before the first / after the last frame."""
    x = planes(ref)
    b = filt2(x, blur5(), mutant)
    m = np.zeros(x.shape[0], np.float64)
    m[1:] = np.abs(b[1:] - b[:-1]).mean(axis=(1, 2))
    if prev is not None:
        m[0] = np.abs(b[0] - filt2(planes(prev[None]), blur5(), mutant)[0]).mean()
    after = m[1:].tolist()
    if nxt is not None:
        after.append(float(np.abs(filt2(planes(nxt[None]), blur5(), mutant)[0] - b[-1]).mean()))
    m2 = m.copy()
    m2[:len(after)] = np.minimum(m[:len(after)], np.asarray(after))
    if mutant == "motion2_before":
        m2 = m.copy()
        m2[1:] = np.minimum(m[1:], m[:-1])
    return m, m2


# ----------------------------------------------------------------------------- ADM
def dwt(x: np.ndarray, mutant=None):
    """One db2 step: (a, h, v, d), (vertical, horizontal) = (lo, lo), (hi, lo), (lo, hi), (hi, hi)."""
    lo, hi = db2()
    vl, vh = dwt_axis(x, lo, -2, mutant), dwt_axis(x, hi, -2, mutant)
    return dwt_axis(vl, lo, -1, mutant), dwt_axis(vh, lo, -1, mutant), dwt_axis(vl, hi, -1, mutant), dwt_axis(vh, hi, -1, mutant)


def clamp_shift(x: np.ndarray, dy: int, dx: int) -> np.ndarray:
    h, w = x.shape[-2:]
    return x[..., np.clip(np.arange(h) + dy, 0, h - 1), :][..., np.clip(np.arange(w) + dx, 0, w - 1)]


def adm(ref: np.ndarray, dis: np.ndarray, counts=None, mutant=None) -> np.ndarray:
    """[F,H,W] u8 x2 -> adm2 [F]."""
    x, y = planes(ref), planes(dis)
    num = np.zeros(x.shape[0], np.float64)
    den = np.zeros(x.shape[0], np.float64)
    for s in range(4):
        x, oh, ov, od = dwt(x, mutant)
        y, th, tv, td = dwt(y, mutant)
        dp = oh * th + ov * tv
        om, tm = oh * oh + ov * ov, th * th + tv * tv
        flag = (dp >= 0.0) & (dp * dp >= COS2 * om * tm)
        if counts is not None:
            counts["adm_flag_set"][s] += int(flag.sum())
            counts["adm_flag_clear"][s] += int((~flag).sum())
            counts["adm_dp_negative"][s] += int((dp < 0.0).sum())
            counts["adm_o_zero"][s] += int(sum(((o == 0.0) & (t != 0.0)).sum() for o, t in ((oh, th), (ov, tv), (od, td))))
        rf = (1.0 / csf_q(s + 1, 1), 1.0 / csf_q(s + 1, 1), 1.0 / csf_q(s + 1, 2))
        rest, art = [], []
        for o, t in ((oh, th), (ov, tv), (od, td)):
            k = np.clip(t / (o + 1e-30), 0.0, 1.0)
            r = np.where(flag, t, k * o)
            rest.append(r)
            art.append(t - r)
        thr = None
        for b in range(3):
            a = np.abs(rf[b] * art[b])
            acc = None
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    term = clamp_shift(a, dy, dx)
                    acc = term if acc is None else acc + term
            if mutant != "adm_threshold_no_centre":
                acc = acc + a
            thr = acc if thr is None else thr + acc
        thr = thr / 30.0
        h, w = oh.shape[-2:]
        left, top = max(0, int(w * 0.1 - 0.5)), max(0, int(h * 0.1 - 0.5))
        if mutant == "adm_window_floor":
            left, top = int(w * 0.1), int(h * 0.1)
        if mutant == "adm_hw_swapped":
            left, top = max(0, int(h * 0.1 - 0.5)), max(0, int(w * 0.1 - 0.5))
        win = (slice(None), slice(top, h - top), slice(left, w - left))
        floor_term = np.cbrt((w - 2 * left) * (h - 2 * top) / 32.0)
        for b, o in enumerate((oh, ov, od)):
            v = np.maximum(np.abs(rf[b] * rest[b]) - thr, 0.0)[win]
            u = np.abs(rf[b] * o)[win]
            num += np.cbrt((v * v * v).sum(axis=(1, 2))) + floor_term
            den += np.cbrt((u * u * u).sum(axis=(1, 2))) + floor_term
    return num / den


# ----------------------------------------------------------------------------- features and score
def new_counts():
    """Per scale, how many pixels took each way: the three VIF pixel classes - `s1_below_eps` (a flat reference window),
    `low_term` (eps <= s1 < nsq) and `log_term` (s1 >= nsq) - the corrections `s2_below_eps` and `gain_negative`,
    `flat_term` (= s1_below_eps + low_term), and the two values of the ADM flag.  For the edge matrix: `sv_floored` (the
    `sw` floor held), `adm_dp_negative` (dp < 0), `adm_o_zero` (a reference coefficient exactly 0 under a non-zero
    distorted one: the 1e-30 quotient is evaluated and clamps), and two figures that are no counts - `nsq_margin`,
    the smallest |s1 - nsq| / nsq (the one discontinuous branch), and `max_gain_log`, the largest gain in the log term before
    the clamp to 100."""
    counts = {k: [0, 0, 0, 0] for k in ("s1_below_eps", "s2_below_eps", "gain_negative", "log_term", "flat_term", "low_term",
                                        "adm_flag_set", "adm_flag_clear", "sv_floored", "adm_dp_negative", "adm_o_zero")}
    counts["nsq_margin"] = [math.inf] * 4
    counts["max_gain_log"] = [0.0] * 4
    return counts


def luma(frames: np.ndarray, order: str = "bgr", masks=None, invert: bool = False, rect=None) -> np.ndarray:
    """[n,H,W,3] u8 -> [n,h,w] u8: the 20-bit fixed-point Y of the I420 hand-off, of the masked, cropped frames."""
    f = np.asarray(frames).astype(np.int64)
    if masks is not None:
        keep = (np.asarray(masks) != 0) != bool(invert)
        f = f * keep[..., None]
    r, g, b = (f[..., 2], f[..., 1], f[..., 0]) if order == "bgr" else (f[..., 0], f[..., 1], f[..., 2])
    y = ((269484 * r + 528482 * g + 102760 * b + (1 << 19) + (16 << 20)) >> 20).astype(np.uint8)
    if rect is not None:
        y = y[:, rect[0]:rect[1], rect[2]:rect[3]]
    return np.ascontiguousarray(y)


def branch_pair(h: int = 64, w: int = 64):
    """A second pair, for the corrections the fixture does not reach: frame 0 textured against flat (s2 < eps
    everywhere), frame 1 noise against independent noise (the gain is negative in many windows)."""
    rng = np.random.default_rng(7)
    ref = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
    dis = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
    dis[0] = 90
    return ref, dis


def features(ref: np.ndarray, dis: np.ndarray, prev=None, nxt=None, counts=None, mutant=None) -> np.ndarray:
    """[F,H,W] u8 x2 -> [F,6] = adm2, motion2, vif_scale0..3."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(f"vmaf: unknown mutant {mutant!r}")
    ref, dis = np.asarray(ref), np.asarray(dis)
    if ref.shape != dis.shape:
        raise ValueError("vmaf: the two clips differ in shape")
    planes(ref), planes(dis)
    out = np.empty((ref.shape[0], 6), np.float64)
    pr, pd = ref, dis
    if mutant == "pass2_from_0":                  # a later pass reads the frames of the first: ref + f0 * size lost its f0
        at = np.arange(ref.shape[0]) % PASS_FRAMES
        pr, pd = ref[at], dis[at]
    out[:, 0] = adm(pr, pd, counts, mutant)
    out[:, 1] = motion(ref, prev, nxt, mutant)[1]
    out[:, 2:] = vif(pr, pd, counts, mutant)
    return out


def score(feats: np.ndarray, model) -> np.ndarray:
    """The nu-SVR of a `VmafModel`-like object (slopes, intercepts, sv, coef, rho, gamma, score_clip, transform,
    enable_transform), written out directly."""
    slopes, intercepts = np.asarray(model.slopes, np.float64), np.asarray(model.intercepts, np.float64)
    sv, coef = np.asarray(model.sv, np.float64), np.asarray(model.coef, np.float64)
    out = []
    for f in np.asarray(feats, np.float64):
        x = slopes[1:] * f + intercepts[1:]
        p = float((coef * np.exp(-model.gamma * ((sv - x) ** 2).sum(axis=1))).sum()) - model.rho
        s = (p - intercepts[0]) / slopes[0]
        if model.enable_transform:
            p0, p1, p2, out_gte_in = model.transform
            t = p0 + p1 * s + p2 * s * s
            s = max(t, s) if out_gte_in else t
        if model.score_clip is not None:
            s = min(max(s, model.score_clip[0]), model.score_clip[1])
        out.append(s)
    return np.asarray(out, np.float64)


def within_bar(got, want) -> bool:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and bool((np.abs(got - want) <= BAR * np.maximum(1.0, np.abs(want))).all())


# ----------------------------------------------------------------------------- the fixture
def blur_u8(y: np.ndarray, sigma_noise: float, rng) -> np.ndarray:
    b = filt2(y.astype(np.float64), blur5())
    return np.clip(np.rint(b + rng.normal(0.0, sigma_noise, y.shape)), 0, 255).astype(np.uint8)


@lru_cache(maxsize=None)
def fixture(h: int, w: int, frames: int = FRAMES):
    """(ref, dis) u8 [frames,h,w]: the left third flat (77), upper right a noisy ramp, lower right sinusoid texture plus
    noise, drifting from frame to frame; dis = 5-tap blur plus N(0, 1.5), rounded."""
    rng = np.random.default_rng(1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ref = np.empty((frames, h, w), np.uint8)
    for f in range(frames):
        ramp = 40.0 + 150.0 * xx / w + 2.0 * f + rng.normal(0.0, 6.0, (h, w))
        tex = 128.0 + 70.0 * np.sin(0.9 * xx + 0.4 * f) * np.sin(0.7 * yy) + rng.normal(0.0, 4.0, (h, w))
        img = np.where(yy < h // 2, ramp, tex)
        img[:, :w // 3] = 77.0
        ref[f] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    dis = blur_u8(ref, 1.5, rng)
    ref.setflags(write=False)
    dis.setflags(write=False)
    return ref, dis


@lru_cache(maxsize=None)
def expected(h: int, w: int):
    """The statement's features of the fixture, computed once and shared."""
    ref, dis = fixture(h, w)
    out = features(ref, dis)
    out.setflags(write=False)
    return out
