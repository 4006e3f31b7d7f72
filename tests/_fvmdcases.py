"""The edge matrix of csrc/fvmd.hip, importable without a GPU: the Jacobi sizes around the two LDS boundaries, hand-made
tracks for the histogram kernel, the Gram kernels' block edges, the shortest tracker clip; the float64 expected values
(tests/_fvmd_ref.py and np.linalg.svd); a numpy model of the one-sided Jacobi sweeps in the kernels' pairing order; and
the mutants - the statement with one clause changed, each of which must move a named case by at least 1e-6, a thousand
bars.

Every case is derived from a constant of the source: FVMD_LDS_DOUBLES = 16384 doubles of dynamic LDS (8192 is the
64 KiB above which the launch needs the opt-in), FVMD_MAX_ROWS = 1024, the 16 x 16 Gram tile, the 256 threads of the
mean, row-norm and scalars kernels, FVMD_MIN_SEQ / FVMD_MAX_SEQ, the 8 bins of a quarter pi.

Hand-made tracks are exact: a point either walks in integer steps or alternates between 0 and v, so every velocity is v
or -v and every acceleration +-2 v to the bit, and a vector meant to lie on a bin boundary lies on it."""
from functools import lru_cache

import numpy as np

import _fvmd_ref as R

BAR = R.BAR
LDS_DOUBLES, OPT_IN_DOUBLES, MAX_ROWS, TILE, THREADS, MIN_SEQ, MAX_SEQ, SWEEPS = 16384, 8192, 1024, 16, 256, 10, 16, 16
SOURCE = "fvmd.hip"

# ============================================================================================ Jacobi
# (k, len): what it covers
JACOBI = {
    (64, 128): "8192 doubles, exactly 64 KiB",
    (65, 128): "the first size above 64 KiB",
    (91, 91): "inside the opt-in range",
    (128, 128): "16384 doubles, the last in-LDS size",
    (129, 127): "16383 doubles, odd k, in LDS",
    (129, 128): "the first size on the per-round path",
    (128, 64): "k > len",
    (300, 40): "k >> len, still in LDS",
    (16, 1024): "the skinniest the LDS path admits, k << len",
    (1024, 16): "the skinniest the LDS path admits, k >> len",
}
FRECHET = ((128, 128, 384), (128, 129, 384))           # the Gram matrix is 128 x 128 (in LDS) and 128 x 129 (per round)
FRECHET_JACOBI = {(128, 128, 384): "fvmd_jacobi_lds_kernel", (128, 129, 384): "fvmd_jacobi_round_kernel"}


def jacobi_kernels(k: int, ln: int):
    """The dispatch rule of elvis_fvmd_singular_values_f64."""
    return ("fvmd_jacobi_lds_kernel",) if k * ln <= LDS_DOUBLES else ("fvmd_jacobi_round_kernel", "fvmd_norm_kernel")


def group_kernels():
    """group of tests/test_gpu_fvmd_matrix.py -> the kernels its cases launch."""
    gram = ("fvmd_mean_kernel", "fvmd_gram_kernel", "fvmd_row_norm_kernel", "fvmd_scalars_kernel")
    jacobi = tuple(sorted({k for shape in JACOBI for k in jacobi_kernels(*shape)}))
    grams = tuple(sorted({k for n, m, _ in FRECHET for k in jacobi_kernels(min(n, m), max(n, m))}))
    return {"jacobi": jacobi, "frechet": gram + grams + ("fvmd_finish_kernel",), "hist": ("fvmd_hist_kernel",) if HIST else (),
            "gram": gram if GRAM else (),
            "tracker": ("fvmd_pyr_down_kernel<true>", "fvmd_pyr_down_kernel<false>", "fvmd_track_kernel", "fvmd_hist_kernel")}


@lru_cache(maxsize=None)
def jacobi_matrix(k: int, ln: int) -> np.ndarray:
    """Random, column scales 0.1 to 10, as test_jacobi_against_numpy builds it."""
    rng = np.random.default_rng(1000 * k + ln)
    mat = rng.normal(0, 1, (k, ln)) * rng.uniform(0.1, 10.0, (1, ln))
    mat.setflags(write=False)
    return mat


@lru_cache(maxsize=None)
def jacobi_expected(k: int, ln: int) -> np.ndarray:
    return np.linalg.svd(jacobi_matrix(k, ln), compute_uv=False)


def pairing(r: int, K: int):
    """fvmd_pair for every p of round r: (i, j) arrays."""
    m = K - 1
    p = np.arange(K // 2)
    return np.where(p == 0, m, (r + p) % m), np.where(p == 0, r, (r - p + m) % m)


def jacobi_model(mat: np.ndarray, sweeps: int = SWEEPS, mutant=None):
    """The sweeps of the two Jacobi kernels in numpy: the same pairing, rotation and skip rule, a round's disjoint pairs
    at once; only the order inside a dot product differs.  -> (the vectors' norms, rotations made in the last sweep)."""
    x = np.array(mat, np.float64)
    k = x.shape[0]
    K = (k + 1) & ~1
    rounds = K - 2 if mutant == "pairing_skips_last_round" else K - 1
    last = 0
    for _ in range(sweeps):
        last = 0
        for r in range(rounds):
            i, j = pairing(r, K)
            ok = (i < k) & (j < k)
            i, j = i[ok], j[ok]
            xi, xj = x[i], x[j]
            al, be, ga = (xi * xi).sum(1), (xj * xj).sum(1), (xi * xj).sum(1)
            go = np.abs(ga) > 1e-15 * np.sqrt(al * be)
            with np.errstate(all="ignore"):
                zeta = (be - al) / (2.0 * ga)
                t = np.where(zeta < 0.0, -1.0, 1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = c * t
            c, s = np.where(go, c, 1.0)[:, None], np.where(go, s, 0.0)[:, None]
            x[i], x[j] = c * xi - s * xj, s * xi + c * xj
            last += int(go.sum())
    return np.sqrt((x * x).sum(1)), last


@lru_cache(maxsize=None)
def frechet_rows(n: int, m: int, d: int):
    rng = np.random.default_rng(n * 1000 + m)
    a, b = rng.normal(0, 3, (n, d)) + rng.normal(0, 1, d), rng.normal(0, 2, (m, d))
    a.setflags(write=False), b.setflags(write=False)
    return a, b


# ============================================================================================ Gram
GRAM = ((2, 2, 1), (2, 17, 15), (16, 16, 16), (17, 2, 17), (2, 17, 255), (16, 16, 256), (130, 131, 257))


@lru_cache(maxsize=None)
def gram_rows(n: int, m: int, d: int):
    rng = np.random.default_rng(n * 100000 + m * 1000 + d)
    a, b = rng.normal(0, 3, (n, d)) + rng.normal(0, 1, d), rng.normal(0, 2, (m, d)) + 0.5
    a.setflags(write=False), b.setflags(write=False)
    return a, b


# ============================================================================================ histograms
DIRECTIONS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))      # bin k: the angle k pi / 4
OFF_AXIS = ((2, 1), (1, 3), (-3, 1), (-2, -5), (1, -2), (5, -1), (-1, 4), (-4, -3))       # one inside each octant
UP, DOWN = np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)
TINY = 5e-324
# one-ulp neighbours of the eight directions, on either side
NEIGHBOURS = ((1.0, TINY), (1.0, -TINY), (UP, 1.0), (DOWN, 1.0), (TINY, 1.0), (-TINY, 1.0), (-UP, 1.0), (-DOWN, 1.0),
              (-1.0, TINY), (-1.0, -TINY), (-UP, -1.0), (-DOWN, -1.0), (TINY, -1.0), (-TINY, -1.0), (UP, -1.0), (DOWN, -1.0))
SINGLE_CELL = 6                                                                            # row 1, column 2: its transpose is cell 9

# name -> (B, S, what it holds)
HIST = {
    "axes_S10_B1": (1, 10, "every point walks the 8 exact directions in turn, integer lengths 1..3"),
    "mixed_S16_B3": (3, 16, "per point and step one of the 8 directions or of 8 off-axis integer vectors"),
    "negzero_S10_B1": (1, 10, "a coordinate that alternates +0.0 / -0.0 under an integer walk in the other"),
    "ulp_S16_B1": (1, 16, "one-ulp neighbours of the 8 directions, alternating v / -v"),
    "zero_S10_B3": (3, 10, "nothing moves"),
    "tiny_huge_S10_B1": (1, 10, "lengths 1e-300 and 1e6 on the 8 directions and between them, alternating v / -v"),
    "single_cell_S16_B1": (1, 16, "the 25 points of one cell move, the rest stand still"),
    "constant_velocity_S10_B3": (3, 10, "every point a constant non-zero integer velocity: the acceleration is exactly 0"),
}


def _walk(start, steps):
    """[B,400,2] start and [B,S-1,400,2] steps -> tracks [B,S,400,2], summed in order."""
    out = [start]
    for t in range(steps.shape[1]):
        out.append(out[-1] + steps[:, t])
    return np.stack(out, axis=1)


def _alternate(v, s):
    """[B,400,2] vectors -> tracks [B,S,400,2] that stand at 0 on even frames and at v on odd ones."""
    return np.stack([v * float(t & 1) for t in range(s)], axis=1)


@lru_cache(maxsize=None)
def hist_tracks(name: str) -> np.ndarray:
    b, s, _ = HIST[name]
    pt = np.arange(R.POINTS)
    start = np.broadcast_to(np.stack([pt % R.GRID, pt // R.GRID], axis=-1).astype(np.float64) * 3.0, (b, R.POINTS, 2))
    dirs, off = np.asarray(DIRECTIONS, np.float64), np.asarray(OFF_AXIS, np.float64)
    seg, step = np.arange(b)[:, None, None], np.arange(s - 1)[None, :, None]
    if name.startswith("axes"):
        tr = _walk(start, dirs[(step + 0 * seg + 0 * pt) % 8] * (1.0 + (pt % 3))[None, None, :, None])
    elif name.startswith("mixed"):
        pick = (pt[None, None, :] + 3 * step + 5 * seg) % 16
        tr = _walk(start, np.concatenate([dirs, off])[pick] * (1.0 + (pt % 2))[None, None, :, None])
    elif name.startswith("negzero"):
        walk = np.cumsum(np.ones((b, s, R.POINTS)), axis=1) * np.where(pt % 4 < 2, 1.0, -1.0)
        flip = np.where((np.arange(s) & 1)[None, :, None] == 1, -0.0, 0.0) * np.ones((b, s, R.POINTS))
        tr = np.where((pt % 2 == 0)[None, None, :, None], np.stack([flip, walk], axis=-1), np.stack([walk, flip], axis=-1))
    elif name.startswith("ulp"):
        tr = _alternate(np.broadcast_to(np.asarray(NEIGHBOURS, np.float64)[pt % 16], (b, R.POINTS, 2)), s)
    elif name.startswith("zero"):
        tr = np.broadcast_to(start[:, None], (b, s, R.POINTS, 2))
    elif name.startswith("tiny_huge"):
        v = np.concatenate([dirs, off])[pt % 16] * np.where((pt // 16) % 2 == 0, 1e-300, 1e6)[:, None]
        tr = _alternate(np.broadcast_to(v, (b, R.POINTS, 2)), s)
    elif name.startswith("single_cell"):
        moving = np.zeros(R.POINTS, bool)
        moving[[R.cell_point(SINGLE_CELL, a) for a in range(R.CELL_SIDE * R.CELL_SIDE)]] = True
        pick = (pt[None, None, :] + step) % 16
        tr = _walk(start, np.concatenate([dirs, off])[pick] * moving[None, None, :, None] + 0.0 * seg[..., None])
    elif name.startswith("constant_velocity"):
        v = np.concatenate([dirs, off])[(pt[None, :] + 3 * np.arange(b)[:, None]) % 16]
        tr = _walk(start, np.broadcast_to(v[:, None], (b, s - 1, R.POINTS, 2)))
    else:
        raise ValueError(name)
    tr = np.ascontiguousarray(tr, np.float64)
    assert tr.shape == (b, s, R.POINTS, 2)
    tr.setflags(write=False)
    return tr


@lru_cache(maxsize=None)
def hist_expected(name: str, mutant=None) -> np.ndarray:
    out = R.features(hist_tracks(name), mutant=mutant)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def hist_counts(name: str):
    c = R.new_counts()
    R.features(hist_tracks(name), counts=c)
    return c


# ============================================================================================ tracker
TRACKER = ("pan", 64, 65, MIN_SEQ)                         # kind, h, w, seq_len: a clip of exactly seq_len frames, and one frame less


@lru_cache(maxsize=None)
def tracker_expected():
    kind, h, w, s = TRACKER
    clip = R.clip(kind, s, h, w)
    margins = []
    tracks = R.track(clip, s, 1, margins)
    return dict(clip=clip, tracks=tracks, rows=R.features(tracks), margins=np.concatenate(margins))


# ============================================================================================ mutants
# mutant -> (stage, the case on which it must differ from the statement by >= 1e-6)
MUTANTS = {
    "vote_previous_bin": ("hist", "mixed_S16_B3"),
    "cell_transposed": ("hist", "single_cell_S16_B1"),
    "acceleration_one_sided": ("hist", "constant_velocity_S10_B3"),
    "mean_over_n_minus_1": ("gram", (2, 17, 15)),
    "centre_by_a": ("gram", (2, 17, 15)),
    "pairing_skips_last_round": ("jacobi", (64, 128)),
}
assert set(MUTANTS) == set(R.MUTANTS) | {"pairing_skips_last_round"}


def mutant_distance(mutant: str) -> float:
    """max |mutant - statement| on the mutant's case."""
    stage, case = MUTANTS[mutant]
    if stage == "hist":
        return float(np.abs(hist_expected(case, mutant) - hist_expected(case)).max())
    if stage == "gram":
        a, b = gram_rows(*case)
        (g0, s0), (g1, s1) = R.gram_parts(a, b), R.gram_parts(a, b, mutant=mutant)
        return float(max(np.abs(g1 - g0).max(), np.abs(s1 - s0).max()))
    r = min(case)                                     # the values the GPU test holds to the bar; what lies past them it holds apart
    got = np.sort(jacobi_model(jacobi_matrix(*case), mutant=mutant)[0])[::-1]
    return float(np.abs(got[:r] - jacobi_expected(*case)).max())
