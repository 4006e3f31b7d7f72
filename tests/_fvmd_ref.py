"""The numpy float64 statement of the FVMD contract (include/elvis_amd.h) that csrc/fvmd.hip is pinned to.

BUILD-DEFINED: the `fvmd` package the reference calls (elvis.py:3476-3505) is not available; this states the published
form - tracks -> velocity / acceleration -> cell orientation histograms -> Frechet distance - with a pyramidal
Lucas-Kanade tracker in the network's place.  It does NOT claim parity with the `fvmd` package.

Every stage is written out: the pyramid loops over its taps, the tracker over the window's rows (vectorised over a row's
15 columns and over the points), the window sums add their terms in the device's order (lane partials, then the
butterfly), the histograms loop over a cell's points.  `frechet` is the Gram / nuclear-norm form of the contract;
`frechet_textbook` is np.cov + scipy.linalg.sqrtm, there to cross-check the identity.  `scripted_score` is the scoring
stub shared by tools/make_fvmd_golden.py and the control-flow test."""
from functools import lru_cache

import numpy as np

MIN_SIDE = 64
GRID = 20
POINTS = 400
RADIUS = 7
WIN = 15
WIN_PIXELS = 225
ITERS = 8
MIN_EIG = 1e-3
CELLS, CELL_SIDE, BINS = 4, 5, 8
QUARTER_PI = 0.78539816339744830962
TAPS = (0.0625, 0.25, 0.375, 0.25, 0.0625)
BAR = 1e-9                                        # |device - statement| <= BAR * max(1, |statement|)


class NoTrajectories(RuntimeError):
    pass


def seq_len_of(frames: int) -> int:
    """elvis.py:3452"""
    return max(10, min(16, frames))


def segments(frames: int, seq_len: int, step: int = 1) -> int:
    return 0 if frames < seq_len else (frames - seq_len) // step + 1


def reflect(idx: np.ndarray, n: int) -> np.ndarray:
    idx = np.abs(idx)
    return np.where(idx >= n, 2 * n - 2 - idx, idx)


def pyr_down(planes: np.ndarray) -> np.ndarray:
    """[F,h,w] -> [F,(h+1)//2,(w+1)//2]: [1,4,6,4,1]/16 down the columns, then along the rows, kept at even indices."""
    _, h, w = planes.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    rows = [reflect(2 * np.arange(ho) + k - 2, h) for k in range(5)]
    v = TAPS[0] * planes[:, rows[0], :]
    for k in range(1, 5):
        v = v + TAPS[k] * planes[:, rows[k], :]
    cols = [reflect(2 * np.arange(wo) + k - 2, w) for k in range(5)]
    out = TAPS[0] * v[:, :, cols[0]]
    for k in range(1, 5):
        out = out + TAPS[k] * v[:, :, cols[k]]
    return np.ascontiguousarray(out)


def pyramid(luma: np.ndarray):
    lv0 = np.ascontiguousarray(luma, dtype=np.float64)
    lv1 = pyr_down(lv0)
    return lv0, lv1, pyr_down(lv1)


def sample(planes: np.ndarray, frame: np.ndarray, x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """Bilinear sample of planes[frame] at (x, y), each coordinate clamped to [0, n - 1] first."""
    h, w = planes.shape[1:]
    x = np.minimum(np.maximum(x, 0.0), w - 1.0)
    y = np.minimum(np.maximum(y, 0.0), h - 1.0)
    fx0, fy0 = np.floor(x), np.floor(y)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    right, below = np.minimum(x0 + 1, w - 1) - x0, (np.minimum(y0 + 1, h - 1) - y0) * w
    ax, ay = x - fx0, y - fy0
    flat = planes.reshape(-1)                                               # a view: the levels are contiguous
    at = (frame * h + y0) * w + x0                                          # v00; the other three corners by offset
    top = (1.0 - ax) * flat.take(at) + ax * flat.take(at + right)
    bot = (1.0 - ax) * flat.take(at + below) + ax * flat.take(at + below + right)
    return (1.0 - ay) * top + ay * bot


def window_sum(terms: np.ndarray) -> np.ndarray:
    """[225, N] -> [N] in the device's order: lane L adds offsets L, L + 64, L + 128, L + 192, then the butterfly."""
    t = np.concatenate([terms, np.zeros((256 - WIN_PIXELS,) + terms.shape[1:])]).reshape(4, 64, -1)
    v = ((t[0] + t[1]) + t[2]) + t[3]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ o]
    return v[0]


def level(planes, frame, px, py, dx, dy, margins=None):
    """One pyramid level of one frame step for N points: (dx, dy) after the 8 updates."""
    n = px.shape[0]
    ox = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)[:, None]
    wx, wy = np.empty((WIN_PIXELS, n)), np.empty((WIN_PIXELS, n))
    tpl, gx, gy = np.empty((WIN_PIXELS, n)), np.empty((WIN_PIXELS, n)), np.empty((WIN_PIXELS, n))
    for r in range(WIN):                                                   # the window's rows, oy = r - 7
        sl = slice(r * WIN, (r + 1) * WIN)
        wx[sl] = px[None, :] + ox
        wy[sl] = np.broadcast_to(py[None, :] + float(r - RADIUS), (WIN, n))
        tpl[sl] = sample(planes, frame, wx[sl], wy[sl])
        gx[sl] = (sample(planes, frame, wx[sl] + 1.0, wy[sl]) - sample(planes, frame, wx[sl] - 1.0, wy[sl])) * 0.5
        gy[sl] = (sample(planes, frame, wx[sl], wy[sl] + 1.0) - sample(planes, frame, wx[sl], wy[sl] - 1.0)) * 0.5
    sxx, sxy, syy = window_sum(gx * gx), window_sum(gx * gy), window_sum(gy * gy)
    diff = sxx - syy
    lam = 0.5 * ((sxx + syy) - np.sqrt(diff * diff + 4.0 * (sxy * sxy)))
    if margins is not None:
        margins.append(lam / float(WIN_PIXELS))
    skip = lam / float(WIN_PIXELS) < MIN_EIG                               # THE data branch
    det = sxx * syy - sxy * sxy
    for _ in range(ITERS):
        r_ = np.empty((WIN_PIXELS, n))
        for r in range(WIN):
            sl = slice(r * WIN, (r + 1) * WIN)
            r_[sl] = tpl[sl] - sample(planes, frame + 1, wx[sl] + dx[None, :], wy[sl] + dy[None, :])
        bx, by = window_sum(r_ * gx), window_sum(r_ * gy)
        with np.errstate(divide="ignore", invalid="ignore"):
            dx = np.where(skip, dx, dx + (syy * bx - sxy * by) / det)
            dy = np.where(skip, dy, dy + (sxx * by - sxy * bx) / det)
    return dx, dy


def grid(h: int, w: int):
    j, i = np.meshgrid(np.arange(GRID, dtype=np.float64), np.arange(GRID, dtype=np.float64))
    return (((j + 0.5) * float(w)) / float(GRID) - 0.5).reshape(-1), (((i + 0.5) * float(h)) / float(GRID) - 0.5).reshape(-1)


def track(luma: np.ndarray, seq_len: int, step: int = 1, margins=None) -> np.ndarray:
    """u8 [F,h,w] -> tracks [B, seq_len, 400, 2] = (x, y); every segment from a fresh grid.  `margins`, a list, collects
    lambda_min / 225 of every (step, level, point)."""
    luma = np.asarray(luma)
    if luma.ndim != 3 or luma.dtype != np.uint8 or luma.shape[1] < MIN_SIDE or luma.shape[2] < MIN_SIDE:
        raise ValueError(f"fvmd: a clip is u8 [F, H, W] with H, W >= {MIN_SIDE}; a plane smaller than {MIN_SIDE} x {MIN_SIDE} is refused")
    frames, h, w = luma.shape
    b = segments(frames, seq_len, step)
    out = np.zeros((b, seq_len, POINTS, 2))
    if b == 0:
        return out
    lv0, lv1, lv2 = pyramid(luma)
    gx_, gy_ = grid(h, w)
    x, y = np.tile(gx_, b), np.tile(gy_, b)
    first = np.repeat(np.arange(b) * step, POINTS)
    out[:, 0, :, 0], out[:, 0, :, 1] = x.reshape(b, POINTS), y.reshape(b, POINTS)
    for t in range(seq_len - 1):
        f = first + t
        dx, dy = np.zeros_like(x), np.zeros_like(y)
        dx, dy = level(lv2, f, x * 0.25, y * 0.25, dx, dy, margins)
        dx, dy = 2.0 * dx, 2.0 * dy
        dx, dy = level(lv1, f, x * 0.5, y * 0.5, dx, dy, margins)
        dx, dy = 2.0 * dx, 2.0 * dy
        dx, dy = level(lv0, f, x, y, dx, dy, margins)
        x = np.minimum(np.maximum(x + dx, 0.0), w - 1.0)
        y = np.minimum(np.maximum(y + dy, 0.0), h - 1.0)
        out[:, t + 1, :, 0], out[:, t + 1, :, 1] = x.reshape(b, POINTS), y.reshape(b, POINTS)
    return out


def cell_point(c: int, a: int) -> int:
    return ((c // CELLS) * CELL_SIDE + a // CELL_SIDE) * GRID + (c % CELLS) * CELL_SIDE + a % CELL_SIDE


# One clause of the statement changed, selected by `mutant=`; the kernels are never changed.  tests/_fvmdcases.py names
# the case each must move by a thousand bars.
MUTANTS = ("vote_previous_bin", "cell_transposed", "acceleration_one_sided", "mean_over_n_minus_1", "centre_by_a")


def field_hist(vx: np.ndarray, vy: np.ndarray, mutant=None, counts=None) -> np.ndarray:
    """[..., 400] vectors -> [..., 128] = [cell][bin], the soft orientation vote, a cell summed in point order.  `counts`,
    a dict, collects what the vectors reach: `boundary` (per bin k, vectors with u == k exactly), `wrapped` (u < 0 took
    the + 8), `to_eight` (that sum rounded to 8.0, bin 8 & 7), `zero` (magnitude 0), `negative_zero` (a -0.0 component)."""
    m = np.sqrt(vx * vx + vy * vy)
    if counts is not None:
        u0 = np.arctan2(vy, vx) / QUARTER_PI
        u1 = np.where(u0 < 0.0, u0 + 8.0, u0)
        for k in range(BINS):
            counts["boundary"][k] += int(((u1 == float(k)) & (m > 0.0)).sum())
        counts["wrapped"] += int(((u0 < 0.0) & (m > 0.0)).sum())
        counts["to_eight"] += int(((u1 == 8.0) & (m > 0.0)).sum())
        counts["zero"] += int((m == 0.0).sum())
        counts["negative_zero"] += int((((vx == 0.0) & np.signbit(vx)) | ((vy == 0.0) & np.signbit(vy))).sum())
    u = np.arctan2(vy, vx) / QUARTER_PI
    u = np.where(u < 0.0, u + 8.0, u)
    k = np.floor(u)
    f = u - k
    kb = k.astype(np.int64) & (BINS - 1)
    w0, w1 = (1.0 - f) * m, f * m
    bins = np.arange(BINS)
    out = np.zeros(vx.shape[:-1] + (CELLS * CELLS, BINS))
    for c in range(CELLS * CELLS):
        acc = np.zeros(vx.shape[:-1] + (BINS,))
        for a in range(CELL_SIDE * CELL_SIDE):
            pt = cell_point(c, a)
            if mutant == "cell_transposed":                                  # the point's row and column change places
                pt = (pt % GRID) * GRID + pt // GRID
            kk = kb[..., pt, None]
            second = (kk - 1) if mutant == "vote_previous_bin" else (kk + 1)
            acc = (acc + np.where(kk == bins, w0[..., pt, None], 0.0)) + np.where((second & (BINS - 1)) == bins, w1[..., pt, None], 0.0)
        out[..., c, :] = acc
    return out.reshape(vx.shape[:-1] + (CELLS * CELLS * BINS,))


def new_counts():
    """What `field_hist` records of its vectors (see there)."""
    return dict(boundary=[0] * BINS, wrapped=0, to_eight=0, zero=0, negative_zero=0)


def features(tracks: np.ndarray, mutant=None, counts=None) -> np.ndarray:
    """[B,S,400,2] -> [B, (2 S - 3) 128]: velocity histograms, then acceleration histograms."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(f"fvmd: unknown mutant {mutant!r}")
    b = tracks.shape[0]
    v = tracks[:, 1:] - tracks[:, :-1]
    a = v[:, 1:] if mutant == "acceleration_one_sided" else v[:, 1:] - v[:, :-1]
    return np.concatenate([field_hist(v[..., 0], v[..., 1], mutant, counts).reshape(b, -1),
                           field_hist(a[..., 0], a[..., 1], mutant, counts).reshape(b, -1)], axis=1)


def gram_parts(a: np.ndarray, b: np.ndarray, mutant=None):
    """(centred A Bm^T [n,m], (|mu_A - mu_B|^2, |A|_F^2, |Bm|_F^2)); the means add the rows in order."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(f"fvmd: unknown mutant {mutant!r}")
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("fvmd: the two sets of rows must be [n, d] and [m, d]")
    if a.shape[0] < 2 or b.shape[0] < 2:
        raise NoTrajectories(f"fvmd: {a.shape[0]} and {b.shape[0]} feature rows; a Frechet distance needs two of each")
    mu = []
    for rows in (a, b):
        s = np.zeros(rows.shape[1])
        for r in rows:
            s = s + r
        mu.append(s / float(rows.shape[0] - 1 if mutant == "mean_over_n_minus_1" else rows.shape[0]))
    if mutant == "centre_by_a":
        mu[1] = mu[0]
    ac, bc = a - mu[0], b - mu[1]
    dm = mu[0] - mu[1]
    return ac @ bc.T, np.asarray([(dm * dm).sum(), (ac * ac).sum(), (bc * bc).sum()])


def fd_scale(a, b) -> float:
    """tr S1 + tr S2 + |mu_A - mu_B|^2: what the distance's terms cancel against."""
    _, s = gram_parts(a, b)
    return float(s[0] + s[1] / (len(a) - 1.0) + s[2] / (len(b) - 1.0))


def frechet(a, b) -> float:
    """The contract's form: |dmu|^2 + |A|_F^2 / (n-1) + |Bm|_F^2 / (m-1) - 2 |A Bm^T|_* / sqrt((n-1)(m-1)).  Equal to the
    textbook tr S1 + tr S2 - 2 tr (S1 S2)^(1/2) in exact arithmetic: the non-zero eigenvalues of S1 S2 are those of
    (A Bm^T)(A Bm^T)^T / ((n-1)(m-1)), so tr (S1 S2)^(1/2) is the sum of A Bm^T's singular values over that root."""
    gram, s = gram_parts(a, b)
    sv = np.linalg.svd(gram, compute_uv=False)
    na, nb = len(a) - 1.0, len(b) - 1.0
    return float(((s[0] + s[1] / na) + s[2] / nb) - (2.0 * sv.sum()) / np.sqrt(na * nb))


def frechet_textbook(a, b) -> float:
    from scipy.linalg import sqrtm
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s1, s2 = np.atleast_2d(np.cov(a, rowvar=False)), np.atleast_2d(np.cov(b, rowvar=False))
    dm = a.mean(axis=0) - b.mean(axis=0)
    root = sqrtm(s1 @ s2)
    return float((dm * dm).sum() + np.trace(s1) + np.trace(s2) - 2.0 * np.trace(np.real(root)))


def fvmd(ref_luma: np.ndarray, dec_luma: np.ndarray, step: int = 1) -> float:
    ref_luma, dec_luma = np.asarray(ref_luma), np.asarray(dec_luma)
    if ref_luma.shape != dec_luma.shape:
        raise ValueError("fvmd: the two clips differ in shape")
    s = seq_len_of(ref_luma.shape[0])
    if segments(ref_luma.shape[0], s, step) < 2:
        raise NoTrajectories("fvmd: fewer than two segments")
    return frechet(features(track(ref_luma, s, step)), features(track(dec_luma, s, step)))


def within_bar(got, want) -> bool:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and bool((np.abs(got - want) <= BAR * np.maximum(1.0, np.abs(want))).all())


# ----------------------------------------------------------------------------- fixtures
def texture(h: int, w: int, seed: int) -> np.ndarray:
    """A smooth field on a margin of 40 pixels: a sum of low-frequency sinusoids, values about 30 .. 225."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h + 80, :w + 80].astype(np.float64)
    f = np.zeros((h + 80, w + 80))
    for _ in range(12):
        ky, kx = rng.uniform(-0.45, 0.45, 2)
        f += rng.uniform(0.5, 1.0) * np.sin(ky * yy + kx * xx + rng.uniform(0, 2 * np.pi))
    return 128.0 + 97.0 * f / np.abs(f).max()


def shifted(field: np.ndarray, h: int, w: int, sy: float, sx: float) -> np.ndarray:
    """The h x w view of `field` whose content has moved by (sy, sx) pixels: out(y, x) = field(40 + y - sy, 40 + x - sx)."""
    y, x = np.arange(h) + 40.0 - sy, np.arange(w) + 40.0 - sx
    y0, x0 = np.floor(y).astype(int), np.floor(x).astype(int)
    ay, ax = (y - y0)[:, None], (x - x0)[None, :]
    g = lambda a, b: field[np.ix_(a, b)]                                      # noqa: E731
    return (1 - ay) * ((1 - ax) * g(y0, x0) + ax * g(y0, x0 + 1)) + ay * ((1 - ax) * g(y0 + 1, x0) + ax * g(y0 + 1, x0 + 1))


MOTION = {"pan": (0.6, -0.85), "decoded": (0.63, -0.8), "half": (0.6, -0.85), "static": (0.0, 0.0), "fast": (2.5, 3.5)}


@lru_cache(maxsize=None)
def clip(kind: str, frames: int, h: int, w: int) -> np.ndarray:
    """u8 [frames,h,w].  "pan": the texture moving by (vy, vx) = (0.6, -0.85) a frame plus noise of +-2; "decoded": the
    same with other noise and a slight drift; "half": "pan" with its left half at luma 16 (a masked region); "static":
    one frame repeated; "fast": a pan of (2.5, 3.5) a frame that pushes the points of two sides against the border."""
    field = texture(h, w, 7)
    rng = np.random.default_rng(100 + sorted(MOTION).index(kind))
    vy, vx = MOTION[kind]
    out = []
    for t in range(frames):
        f = shifted(field, h, w, vy * t, vx * t)
        if kind != "static":
            f = f + rng.integers(-2, 3, f.shape)
        out.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
    out = np.stack(out)
    if kind == "static":
        out[:] = out[0]
    if kind == "half":
        out[:, :, :w // 2] = 16
    out.setflags(write=False)
    return out


# name -> (clip kind, frames, h, w, seq_len, segment_step): B = 2 and 3, S = 10 and 16, both steps, an odd size.
# The half-black clip is 3200 wide so that the keypoint columns stand 160 pixels apart and the black / textured boundary
# at x = 1600 lies 80 from the nearest column: a level-2 window with its gradient and bilinear reach and the pyramid's
# leak spans 48 pixels, the textured points drift by under 8, so every window sees the black side alone (G = 0 exactly)
# or texture alone and no lambda_min falls near the threshold.
CLIPS = {"pan_67x81": ("pan", 18, 67, 81, 16, 2), "half_64x3200": ("half", 11, 64, 3200, 10, 1), "border_64": ("fast", 12, 64, 64, 10, 1),
         "static_67x81": ("static", 18, 67, 81, 16, 2), "static_64": ("static", 11, 64, 64, 10, 1)}
# (reference rows, decoded rows) of the distance stages: 2 x 2 with a zero side, 2 x 3 with both sides moving, 3 x 2
PAIRS = (("pan_67x81", "static_67x81"), ("half_64x3200", "border_64"), ("border_64", "static_64"))


@lru_cache(maxsize=None)
def tracked(name: str):
    """(clip, pyramid levels 1 and 2, tracks, rows, margins) of one fixture clip, computed once.  A static clip is not
    walked: its points stay on the grid exactly whichever way the singular test falls (b = 0 in every iteration), which
    tests/test_fvmd_host.py checks against `track` itself; it has no margins to report."""
    kind, frames, h, w, seq_len, step = CLIPS[name]
    c = clip(kind, frames, h, w)
    margins = []
    if kind == "static":
        gx_, gy_ = grid(h, w)
        tr = np.ascontiguousarray(np.broadcast_to(np.stack([gx_, gy_], axis=-1), (segments(frames, seq_len, step), seq_len, POINTS, 2)))
        margins.append(np.zeros(0))
    else:
        tr = track(c, seq_len, step, margins)
    return dict(clip=c, seq_len=seq_len, step=step, pyramid=pyramid(c)[1:], tracks=tr, rows=features(tr), margins=np.concatenate(margins))


@lru_cache(maxsize=None)
def expected_distance(ref: str, dec: str):
    """The distance stages between two fixture clips' rows: dict(gram, scalars, sv, fd, scale)."""
    a, b = tracked(ref)["rows"], tracked(dec)["rows"]
    gram, scalars = gram_parts(a, b)
    return dict(gram=gram, scalars=scalars, sv=np.linalg.svd(gram, compute_uv=False), fd=frechet(a, b), scale=fd_scale(a, b))


def margins_clear(margins: np.ndarray) -> bool:
    """No lambda_min / 225 within a factor 10 of the threshold."""
    return not ((margins >= MIN_EIG / 10.0) & (margins <= MIN_EIG * 10.0)).any()


# ----------------------------------------------------------------------------- the control-flow script
def scripted_score(kind: str, indices) -> float:
    """The scoring stub of the control-flow pin: a function of the sampled index list alone.  "converge" settles (the
    early stop fires), "grow" never does, "spread" depends on the first index (the std windows differ), "wide_fails"
    raises NoTrajectories while consecutive indices are more than one frame apart."""
    idx = [int(i) for i in indices]
    if kind == "converge":
        return 5.0 + 1.0 / len(idx)
    if kind == "grow":
        return 1.5 * len(idx) + 0.01 * idx[-1]
    if kind == "spread":
        return 3.0 + 0.125 * idx[0] + 1.0 / len(idx)
    if kind == "wide_fails":
        if len(idx) > 1 and idx[1] - idx[0] > 1:
            raise NoTrajectories(f"scripted: stride {idx[1] - idx[0]}")
        return 7.0 + 2.0 / len(idx)
    raise KeyError(kind)
