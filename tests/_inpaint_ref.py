"""Numpy statement of the wavefront Telea inpainter: float32 throughout, every operation in the order the
contract writes it, vectorised over the pixels of a wave.  The device code (csrc/inpaint.hip) equals it bit for bit
(tests/test_gpu_inpaint.py).  It is a specification, not a baseline, and not cv2's Telea.

Also here: the case list of the GPU test and the mutants - the contract with one clause changed - each of which must
give other bytes than the true statement on the small case named next to it (tests/test_inpaint_host.py)."""
import numpy as np

f32 = np.float32
R = 3
DISC = [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if 0 < dy * dy + dx * dx <= R * R]
BOX = [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if (dy, dx) != (0, 0)]
assert len(DISC) == 28

# mutant -> the case of `mutant_cases()` on which it must differ from the contract
MUTANTS = {
    "raster_order": "block8",       # same-wave pixels read in raster order (Gauss-Seidel instead of Jacobi)
    "box": "block8",                # the 7x7 box instead of the disc
    "no_factor_2": "block8",        # the factor 2 of gI dropped
    "t_known_zero": "block8",       # T(known) = 0
    "half_up": "half",              # floor(v + 0.5) instead of half to even without the +0.5
    "no_small_dir": "random60",     # the small-dir branch dropped
    "reads_hole_bytes": "block8",   # gI reads neighbours that are not available (bytes under the hole)
}


# ----------------------------------------------------------------------------- distances
def row_distance(known):
    """[H,W] int64: the distance of every pixel to the nearest known pixel of its row; a large value where none."""
    h, w = known.shape
    far = 1 << 20
    x = np.arange(w)[None, :]
    left = np.maximum.accumulate(np.where(known, x, -far), axis=1)
    right = np.minimum.accumulate(np.where(known, x, far)[:, ::-1], axis=1)[:, ::-1]
    return np.minimum(x - left, right - x).astype(np.int64)


def squared_distance(known):
    """[H,W] int64: the exact squared Euclidean distance to the nearest known pixel (rows first, then all row pairs)."""
    g = row_distance(known)
    h = known.shape[0]
    dy = np.arange(h)[:, None] - np.arange(h)[None, :]
    return (dy[:, :, None] ** 2 + g[None, :, :] ** 2).min(axis=1)


def wave_index(d2):
    """The smallest integer k with k * k >= d2, in integers."""
    k = np.floor(np.sqrt(d2.astype(np.float64))).astype(np.int64)
    k = np.where(k * k < d2, k + 1, k)
    k = np.where((k > 0) & ((k - 1) * (k - 1) >= d2), k - 1, k)
    assert ((k * k >= d2) & ((k == 0) | ((k - 1) * (k - 1) < d2))).all()
    return k


def known_side_d2(hole):
    """[H,W] int64: the squared distance to the nearest hole among |dx|, |dy| <= 3; -1 where the window has none."""
    h, w = hole.shape
    pad = np.zeros((h + 2 * R, w + 2 * R), bool)
    pad[R:R + h, R:R + w] = hole
    best = np.full((h, w), 1 << 20, np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            there = pad[R + dy:R + dy + h, R + dx:R + dx + w]
            best = np.where(there, np.minimum(best, dy * dy + dx * dx), best)
    return np.where(best == 1 << 20, -1, best)


def level_set(hole, mutant=None):
    """(T float32 [H,W], wave int64 [H,W]) of one frame that has holes and known pixels."""
    d2 = np.where(hole, squared_distance(~hole), 0)
    wave = wave_index(d2)
    t_hole = np.sqrt(d2.astype(f32))
    d2h = known_side_d2(hole)
    t_known = np.where(d2h >= 0, f32(1) - np.sqrt(np.maximum(d2h, 0).astype(f32)), f32(0)).astype(f32)
    if mutant == "t_known_zero":
        t_known = np.zeros_like(t_known)
    return np.where(hole, t_hole, t_known).astype(f32), wave


# ----------------------------------------------------------------------------- one wave
def _estimate(img, avail, T, gtx, gty, ys, xs, mutant):
    """The values of the hole pixels (ys, xs) from the available pixels: float32 [len, C] before rounding, and s."""
    h, w, c = img.shape
    n = len(ys)
    I = img.astype(f32)

    def av(y, x):
        inside = (y >= 0) & (y < h) & (x >= 0) & (x < w)
        if mutant == "reads_hole_bytes":
            return inside
        return inside & avail[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]

    def val(y, x):
        return I[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]

    def grad(ap, am, vp, vq, vm):
        two = f32(1) if mutant == "no_factor_2" else f32(2)
        ap, am = ap[:, None], am[:, None]
        return np.where(ap & am, (vp - vm) * two, np.where(ap, vp - vq, np.where(am, vq - vm, f32(0)))).astype(f32)

    ia, jx, jy = (np.zeros((n, c), f32) for _ in range(3))
    s = np.zeros(n, f32)
    tp, gx, gy = T[ys, xs], gtx[ys, xs], gty[ys, xs]
    for dy, dx in (BOX if mutant == "box" else DISC):
        qy, qx = ys + dy, xs + dx
        inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
        qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
        ok = inside & avail[qy, qx]
        ry, rx = f32(-dy), f32(-dx)
        d2 = f32(dy * dy + dx * dx)
        dst = f32(1) / (d2 * np.sqrt(d2))
        lev = f32(1) / (f32(1) + np.abs(T[qy, qx] - tp))
        dr = rx * gx + ry * gy
        if mutant != "no_small_dir":
            dr = np.where(np.abs(dr) <= f32(0.01), f32(1e-6), dr)
        wgt = np.abs((dst * lev) * dr).astype(f32)
        vq = val(qy, qx)
        gix = grad(av(qy, qx + 1), av(qy, qx - 1), val(qy, qx + 1), vq, val(qy, qx - 1))
        giy = grad(av(qy + 1, qx), av(qy - 1, qx), val(qy + 1, qx), vq, val(qy - 1, qx))
        wc, okc = wgt[:, None], ok[:, None]
        ia = np.where(okc, ia + wc * vq, ia)
        jx = np.where(okc, jx - (wc * gix) * rx, jx)
        jy = np.where(okc, jy - (wc * giy) * ry, jy)
        s = np.where(ok, s + wgt, s)
    assert ia.dtype == jx.dtype == jy.dtype == s.dtype == f32
    if mutant != "no_small_dir":
        assert (s > 0).all(), "a hole pixel without an available neighbour"
    with np.errstate(divide="ignore", invalid="ignore"):
        v = ia / s[:, None] + (jx + jy) / (np.sqrt(jx * jx + jy * jy) + f32(1e-20))
    assert v.dtype == f32
    return v, s


def _to_u8(v, mutant):
    r = np.floor(v + f32(0.5)) if mutant == "half_up" else np.rint(v)
    return np.clip(np.nan_to_num(r, nan=0.0), 0, 255).astype(np.uint8)


def inpaint_frame(img, hole, mutant=None, stats=None):
    """One frame [H,W,C] u8 and its hole mask [H,W] bool.  `stats` (a dict) receives the deepest wave and the
    smallest s."""
    img = np.asarray(img)
    hole = np.asarray(hole) != 0
    out = img.copy()
    if not hole.any() or hole.all():
        return out
    h, w = hole.shape
    T, wave = level_set(hole, mutant)
    tpad = np.pad(T, 1, mode="edge")
    gtx = ((tpad[1:-1, 2:] - tpad[1:-1, :-2]) * f32(0.5)).astype(f32)
    gty = ((tpad[2:, 1:-1] - tpad[:-2, 1:-1]) * f32(0.5)).astype(f32)
    if mutant != "reads_hole_bytes":
        out[hole] = 0                                   # the bytes under the hole are ignored: nothing may depend on them
    last = int(wave.max())
    smin = np.inf
    for k in range(1, last + 1):
        ys, xs = np.nonzero(wave == k)
        avail = wave < k
        if mutant == "raster_order":
            avail = avail.copy()
            for y, x in zip(ys, xs):
                v, s = _estimate(out, avail, T, gtx, gty, np.array([y]), np.array([x]), mutant)
                out[y, x] = _to_u8(v, mutant)[0]
                avail[y, x] = True
        else:
            v, s = _estimate(out, avail, T, gtx, gty, ys, xs, mutant)
            out[ys, xs] = _to_u8(v, mutant)
        smin = min(smin, float(s.min())) if len(ys) else smin
    if stats is not None:
        stats["waves"] = max(stats.get("waves", 0), last)
        stats["min_s"] = min(stats.get("min_s", np.inf), smin)
    if mutant != "reads_hole_bytes":
        assert np.array_equal(out[~hole], img[~hole])
    return out


def inpaint(frames, masks, mutant=None, stats=None):
    """frames [n,H,W,C] u8, masks [n,H,W] (non-zero = hole) -> [n,H,W,C] u8."""
    frames, masks = np.asarray(frames), np.asarray(masks)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and masks.shape == frames.shape[:3]
    return np.stack([inpaint_frame(frames[i], masks[i], mutant, stats) for i in range(len(frames))])


def expand_block_mask(block_masks, block, h, w):
    """[n,By,Bx] -> [n,h,w] u8 0/255 over whole blocks; pixels past the last whole block are known."""
    m = np.asarray(block_masks) != 0
    full = np.zeros((m.shape[0], h, w), np.uint8)
    e = np.repeat(np.repeat(m, block, axis=1), block, axis=2)
    full[:, :e.shape[1], :e.shape[2]] = e[:, :h, :w] * np.uint8(255)
    return full


# ----------------------------------------------------------------------------- test images and cases
def make_image(h, w, c=3, seed=0):
    """Smooth structure plus texture, full byte range, channels that differ."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [x * 1.9 + y * 0.6, 128 + 100 * np.sin(x / 5.0) * np.cos(y / 4.0), 255 - y * 2.3 + 40 * np.sin(x / 3.0)]
    img = np.stack(planes[:c], axis=-1) + rng.integers(-20, 21, size=(h, w, c))
    return np.clip(img, 0, 255).astype(np.uint8)


def _blocks(h, w, b, cells, value=255):
    m = np.zeros((h, w), np.uint8)
    for by, bx in cells:
        m[by * b:(by + 1) * b, bx * b:(bx + 1) * b] = value
    return m


def half_case():
    """A 1 x 3 frame [0, hole, 1]: both neighbours get the same weight w, w * 0 + w * 1 and w + w are exact, so the
    value is exactly 0.5 - half to even gives 0, half up gives 1 (channel 2: 0 and 0, no tie)."""
    frame = np.array([[[0, 1, 0], [77, 77, 77], [1, 0, 0]]], np.uint8)
    return frame[None], np.array([[[0, 255, 0]]], np.uint8)


def mutant_cases():
    """name -> (frames [1,H,W,3], masks [1,H,W]): the small cases the mutants are judged on."""
    rng = np.random.default_rng(5)
    img = make_image(24, 28, 3, seed=2)
    holed = img.copy()
    m8 = _blocks(24, 28, 8, [(1, 1)])
    holed[m8 != 0] = rng.integers(0, 256, size=(int((m8 != 0).sum()), 3), dtype=np.uint8)
    img2 = make_image(21, 26, 3, seed=3)
    m60 = ((rng.random((21, 26)) < 0.6) * 255).astype(np.uint8)
    return {"block8": (holed[None], m8[None]), "random60": (img2[None], m60[None]), "half": half_case()}


def cases():
    """name -> (frames [n,H,W,C] u8, masks [n,H,W] u8): the matrix of tests/test_gpu_inpaint.py.  The block cases are at
    most 96 x 128; the preparation cases (`preparation_cases`) reach 300 rows, 513 columns and 130 x 125."""
    out = {}
    rng = np.random.default_rng(11)
    for b in (8, 16):
        for c in (1, 3):
            h, w = (40, 56) if b == 8 else (64, 80)
            out[f"interior_b{b}_c{c}"] = (make_image(h, w, c, seed=b + c)[None], _blocks(h, w, b, [(2, 3)])[None])
    h, w, b = 48, 64, 8
    gy, gx = h // b - 1, w // b - 1
    corners = [(0, 0), (0, gx), (gy, 0), (gy, gx)]
    edges = [(0, 3), (gy, 4), (2, 0), (3, gx)]
    out["corners"] = (make_image(h, w, 3, seed=20)[None], _blocks(h, w, b, corners)[None])
    out["edges"] = (make_image(h, w, 3, seed=21)[None], _blocks(h, w, b, edges)[None])
    out["merged_2_3_L"] = (make_image(96, 128, 3, seed=22)[None],
                           _blocks(96, 128, 16, [(0, 1), (0, 2), (2, 0), (2, 1), (2, 2), (3, 5), (4, 5), (4, 6)])[None])
    out["removed_30_percent"] = (make_image(96, 128, 3, seed=23)[None],
                                 expand_block_mask(rng.random((1, 6, 8)) < 0.3, 16, 96, 128))
    out["odd_random60"] = (make_image(37, 53, 3, seed=24)[None], ((rng.random((1, 37, 53)) < 0.6) * 255).astype(np.uint8))
    deep = np.ones((1, 40, 50), np.uint8)
    deep[0, 0, 0] = 0
    out["deep_63_waves"] = (rng.integers(0, 256, size=(1, 40, 50, 3), dtype=np.uint8), deep)
    values = np.zeros((48, 64), np.uint8)
    for v, cell in zip((1, 2, 255), [(1, 1), (3, 4), (4, 6)]):
        values += _blocks(48, 64, 8, [cell], v)
    out["tiny_1x3_half"] = half_case()
    out["mask_values_1_2_255"] = (make_image(48, 64, 3, seed=25)[None], values[None])
    # different depths in one clip: no hole, no known pixel, one deep hole, ordinary blocks
    mixed = np.zeros((4, 40, 50), np.uint8)
    mixed[1] = 255
    mixed[2, 3:38, 5:47] = 255
    mixed[3] = _blocks(40, 50, 8, [(1, 1), (3, 4)])
    out["mixed_clip"] = (np.stack([make_image(40, 50, 3, seed=30 + i) for i in range(4)]), mixed)
    out.update(preparation_cases())
    return out


LOCAL_BINS, THREADS = 64, 256        # kLocalBins and the workgroup size of csrc/inpaint.hip (the ledger reads them there)


def preparation_cases():
    """The cases derived from the constants of the preparation kernels: waves at and past kLocalBins (global atomics in
    the histogram and the scatter), rows wider than a workgroup (a thread owns 2 or 3 pixels of a row), h + w + 2 bins
    past 256 (a thread of the scan owns 2 bins), frames of one row and of one column.

    A row or column with a single known pixel fills with nearly constant values (2 to 3 distinct bytes): those cases test
    the preparation pass and the lists, not the estimator.  The textured ones (`wide_5x257`, `deep_70x40`, `bins_25x`)
    test the estimator at these shapes too."""
    out = {}
    rng = np.random.default_rng(12)

    def one_known(h, w, y, x, c=3, seed=0):
        m = np.full((1, h, w), 255, np.uint8)
        m[0, y, x] = 0
        return make_image(h, w, c, seed=seed)[None], m

    out["row_1x300_left"] = one_known(1, 300, 0, 0, seed=41)            # 299 waves, 303 bins, two pixels per thread
    out["row_1x300_mid"] = one_known(1, 300, 0, 137, seed=42)           # the known pixel is the second of a thread's run
    out["row_1x65"] = one_known(1, 65, 0, 0, seed=43)                   # waves 1..64: exactly one pixel on the global-atomic path
    out["row_1x64"] = one_known(1, 64, 0, 0, seed=44)                   # its twin: no pixel on that path
    out["col_300x1"] = one_known(300, 1, 299, 0, seed=45)
    m = np.full((1, 3, 513), 255, np.uint8)                             # three pixels per thread; the outer rows have no known pixel
    m[0, 1, [0, 2, 3, 5, 256, 257, 512]] = 0
    out["wide_3x513"] = (make_image(3, 513, 3, seed=46)[None], m)
    m = ((rng.random((1, 5, 257)) < 0.6) * 255).astype(np.uint8)        # two pixels per thread, the trailing threads own empty runs
    m[0, 2] = 255
    m[0, 3] = 255
    m[0, 3, 256] = 0
    out["wide_5x257"] = (make_image(5, 257, 3, seed=47)[None], m)
    m = np.full((2, 70, 40), 255, np.uint8)                             # both frames add to the same waves >= 64
    m[0, 0] = 0                                                         # frame 0: row 0 known, waves 1..69
    m[1, 69, ::2] = 0                                                   # frame 1: every second pixel of the last row, waves 1..70
    deep = np.stack([make_image(70, 40, 3, seed=48), make_image(70, 40, 3, seed=49)])
    out["deep_70x40"] = (deep, m)
    out["deep_70x40_c1"] = (np.ascontiguousarray(deep[..., 1:2]), m)
    for w in (124, 125):                                                # h + w + 2 = 256 and 257
        m = np.full((1, 130, w), 255, np.uint8)
        m[0, 0, ::3] = 0
        out[f"bins_{130 + w + 2}"] = (make_image(130, w, 1, seed=50 + w)[None], m)
    return out


def wave_counts(masks):
    """int64 [h + w + 2]: per wave, the hole pixels of the frames that have a known pixel - the first h + w + 2 int32 of
    the workspace after elvis_inpaint_prepare (include/elvis_amd.h)."""
    masks = np.asarray(masks) != 0
    n, h, w = masks.shape
    counts = np.zeros(h + w + 2, np.int64)
    for hole in masks:
        if hole.any() and not hole.all():
            counts += np.bincount(level_set(hole)[1][hole], minlength=h + w + 2)
    return counts
