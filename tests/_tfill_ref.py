"""Numpy statement of the temporal fill: integers only, vectorised over the pixels of every displacement.
The device code (csrc/tfill.hip) equals it bit for bit (tests/test_gpu_tfill.py).  It is a specification, not a baseline,
and neither ProPainter nor E2FGVI: the part of their image propagation that needs no training - find where a block's
surroundings are in a neighbouring frame and copy the pixels the hole hides.

"Known" always means the INPUT mask of a frame (zero = known) and source bytes are always INPUT bytes: nothing a fill
writes is read by another fill, so every (frame, block) is independent.

Also here: the panning-clip generator, the case list of the GPU test and the mutants - the contract with one clause
changed - each of which must give other bytes than the true statement on the small case named next to it
(tests/test_tfill_host.py)."""
import numpy as np

MIN_CONTEXT = 64
DEFAULTS = dict(block=16, margin=8, radius=2, search=7, max_mad=6)
LIMITS = dict(block=(1, 32), margin=(0, 16), radius=(0, 8), search=(0, 7), max_mad=(0, 255))

# mutant -> the case of `mutant_cases()` on which it must differ from the contract
MUTANTS = {
    "ties_later": "tint",            # ties go to the later displacement in raster order
    "no_half_rule": "sliver",   # 2 * cnt >= nk dropped (cnt >= 1 in its place)
    "next_first": "pan",             # t+1 comes before t-1
    "source_holes_known": "pan",     # a source's hole bytes are read as if known
    "no_max_mad": "strangers",       # the max_mad acceptance dropped
    "float32_division": "near_tie",  # float32(cost) / float32(cnt) in the cross-multiplication's place
    "filled_as_context": "tint_context",  # pixels a source filled are context (known, with their new bytes) for the next
    "product_32bit": "contrast",     # the cross-multiplication wrapped to 32 bits
}


def source_order(t, n, radius, mutant=None):
    """t-1, t+1, t-2, t+2, ... up to +-radius, frames inside the clip only."""
    signs = (1, -1) if mutant == "next_first" else (-1, 1)
    return [t + s * k for k in range(1, radius + 1) for s in signs if 0 <= t + s * k < n]


def _beats(cost_a, cnt_a, cost_b, cnt_b, mutant):
    """Is cost_a / cnt_a strictly below cost_b / cnt_b: exact, in integers (the products stay below 2^34)."""
    if mutant == "float32_division":
        return bool(np.float32(cost_a) / np.float32(cnt_a) < np.float32(cost_b) / np.float32(cnt_b))
    if mutant == "product_32bit":
        return ((cost_a * cnt_b) & 0xFFFFFFFF) < ((cost_b * cnt_a) & 0xFFFFFFFF)
    return cost_a * cnt_b < cost_b * cnt_a


def _displacement_sums(tgt, kt, src, ks, y0, y1, x0, x1, S):
    """cnt and cost [2S+1, 2S+1] int64 of every displacement of the window rows [y0, y1), columns [x0, x1): over
    P(d) = {p in the window: p + d inside the frame, known_t(p), known_s(p + d)}."""
    h, w, c = src.shape
    sp = np.zeros((h + 2 * S, w + 2 * S, c), np.int64)
    kp = np.zeros((h + 2 * S, w + 2 * S), bool)                 # outside the frame: never in P(d)
    sp[S:S + h, S:S + w] = src
    kp[S:S + h, S:S + w] = ks
    wh, ww = y1 - y0, x1 - x0
    sv = np.lib.stride_tricks.sliding_window_view(sp[y0:y1 + 2 * S, x0:x1 + 2 * S], (wh, ww), axis=(0, 1))   # [D,D,C,wh,ww]
    kv = np.lib.stride_tricks.sliding_window_view(kp[y0:y1 + 2 * S, x0:x1 + 2 * S], (wh, ww), axis=(0, 1))   # [D,D,wh,ww]
    valid = kv & kt[y0:y1, x0:x1][None, None]
    tw = tgt[y0:y1, x0:x1].astype(np.int64).transpose(2, 0, 1)                                               # [C,wh,ww]
    diff = np.abs(sv - tw[None, None]).sum(axis=2)
    return valid.sum(axis=(2, 3)), np.where(valid, diff, 0).sum(axis=(2, 3))


def best_displacement(cnt, cost, nk, S, M, C, mutant=None):
    """The accepted displacement with the least cost / cnt, ties to the earlier one in raster order; None if none."""
    best = None
    for iy in range(2 * S + 1):
        for ix in range(2 * S + 1):
            n, s = int(cnt[iy, ix]), int(cost[iy, ix])
            if (n < 1) if mutant == "no_half_rule" else (2 * n < nk):
                continue
            if mutant != "no_max_mad" and s > M * n * C:
                continue
            if best is None or _beats(s, n, best[0], best[1], mutant) or \
                    (mutant == "ties_later" and not _beats(best[0], best[1], s, n, mutant)):
                best = (s, n, iy - S, ix - S)
    return None if best is None else best[2:]


def temporal_fill(frames, masks, block=16, margin=8, radius=2, search=7, max_mad=6, mutant=None, stats=None):
    """frames [n,H,W,C] u8, masks [n,H,W] (non-zero = hole) -> (out [n,H,W,C] u8, left [n,H,W] u8: 255 where a hole
    stayed unfilled).  `stats` (a dict) receives the displacements chosen, by (t, by, bx, s)."""
    frames, masks = np.asarray(frames), np.asarray(masks)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and masks.shape == frames.shape[:3]
    for name, v in dict(block=block, margin=margin, radius=radius, search=search, max_mad=max_mad).items():
        assert LIMITS[name][0] <= v <= LIMITS[name][1] and int(v) == v, (name, v)
    n, H, W, C = frames.shape
    B, G, S = block, margin, search
    known = masks == 0
    if mutant == "source_holes_known":
        known_src = np.ones_like(known)
    else:
        known_src = known
    out = frames.copy()
    left = np.where(known, 0, 255).astype(np.uint8)
    for t in range(n):
        for by in range(0, H, B):
            for bx in range(0, W, B):
                ye, xe = min(H, by + B), min(W, bx + B)
                unfilled = ~known[t, by:ye, bx:xe]
                if not unfilled.any():
                    continue
                y0, y1, x0, x1 = max(0, by - G), min(H, by + B + G), max(0, bx - G), min(W, bx + B + G)
                nk = int(known[t, y0:y1, x0:x1].sum())
                if nk < MIN_CONTEXT:
                    continue
                tgt, kt = frames[t], known[t]
                for s in source_order(t, n, radius, mutant):
                    if not unfilled.any():
                        break
                    cnt, cost = _displacement_sums(tgt, kt, frames[s], known_src[s], y0, y1, x0, x1, S)
                    d = best_displacement(cnt, cost, nk, S, max_mad, C, mutant)
                    if stats is not None:
                        stats[(t, by, bx, s)] = d
                    if d is None:
                        continue
                    ys, xs = np.nonzero(unfilled)
                    qy, qx = ys + by + d[0], xs + bx + d[1]
                    ok = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    ok &= known_src[s][np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
                    out[t, ys[ok] + by, xs[ok] + bx] = frames[s, qy[ok], qx[ok]]
                    unfilled[ys[ok], xs[ok]] = False
                    if mutant == "filled_as_context":
                        tgt, kt = out[t], kt.copy()
                        kt[by:ye, bx:xe] |= ~unfilled & ~known[t, by:ye, bx:xe]
                left[t, by:ye, bx:xe][~unfilled] = 0
    if mutant is None:
        still = left != 0
        assert np.array_equal(out[known], frames[known]) and np.array_equal(out[still], frames[still])
    return out, left


def expand_block_mask(block_masks, block, h, w):
    """[n,By,Bx] -> [n,h,w] u8 0/255 over whole blocks; pixels past the last whole block are known."""
    m = np.asarray(block_masks) != 0
    full = np.zeros((m.shape[0], h, w), np.uint8)
    e = np.repeat(np.repeat(m, block, axis=1), block, axis=2)
    full[:, :e.shape[1], :e.shape[2]] = e[:, :h, :w] * np.uint8(255)
    return full


# ----------------------------------------------------------------------------- clips
def textured_scene(h, w, c=3, seed=0):
    """A float64 [h,w,c] scene in about [20, 235]: smooth structure at three scales plus a fine texture, channels that
    differ - no displacement but the true one matches a window of it."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, c))
    for ch in range(c):
        for cell, amp in ((16, 45.0), (6, 30.0), (3, 18.0)):
            coarse = rng.normal(size=(h // cell + 3, w // cell + 3))
            fy, fx = y / cell, x / cell
            iy, ix = fy.astype(int), fx.astype(int)
            ay, ax = fy - iy, fx - ix
            img[..., ch] += amp * ((1 - ay) * (1 - ax) * coarse[iy, ix] + (1 - ay) * ax * coarse[iy, ix + 1]
                                   + ay * (1 - ax) * coarse[iy + 1, ix] + ay * ax * coarse[iy + 1, ix + 1])
        img[..., ch] += rng.normal(scale=6.0, size=(h, w))
    return np.clip(128 + img, 20, 235)


def pan_clip(n, h, w, c=3, seed=0, step=(2, 3), sigma=1.0):
    """(noisy, clean) [n,h,w,c] u8: the textured scene cropped at (2t, 3t); `noisy` has N(0, sigma) noise on every
    frame, `clean` is the crop rounded."""
    scene = textured_scene(h + step[0] * n, w + step[1] * n, c, seed)
    rng = np.random.default_rng(seed + 1000)
    to_u8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    noisy, clean = (np.empty((n, h, w, c), np.uint8) for _ in range(2))
    for t in range(n):                                                      # frame by frame: a 1080p clip stays small
        crop = scene[step[0] * t:step[0] * t + h, step[1] * t:step[1] * t + w]
        noisy[t] = to_u8(crop + rng.normal(scale=sigma, size=crop.shape))
        clean[t] = to_u8(crop)
    return noisy, clean


def random_block_masks(n, h, w, block, fraction, seed=0):
    """[n,h,w] u8 0/255: `fraction` of the blocks (ragged last ones included) removed at random in every frame."""
    rng = np.random.default_rng(seed)
    by, bx = -(-h // block), -(-w // block)
    bm = rng.random((n, by, bx)) < fraction
    return (np.repeat(np.repeat(bm, block, axis=1), block, axis=2)[:, :h, :w] * np.uint8(255)).astype(np.uint8)


def holed(frames, masks, value=None, seed=0):
    """The clip with the bytes under the holes replaced: by `value`, or by random bytes - what nothing may depend on."""
    out = np.array(frames)
    hole = np.asarray(masks) != 0
    if value is None:
        out[hole] = np.random.default_rng(seed).integers(0, 256, size=(int(hole.sum()), out.shape[3]), dtype=np.uint8)
    else:
        out[hole] = value
    return out


def psnr(a, b, where):
    """PSNR in dB of the pixels `where` ([n,H,W] bool), all channels."""
    d = (np.asarray(a, np.float64) - np.asarray(b, np.float64))[where]
    return float(10 * np.log10(255.0 ** 2 / max((d ** 2).mean(), 1e-12)))


# ----------------------------------------------------------------------------- the mutants' cases
def near_tie_case():
    """A 2 x 64 x 64 x 1 clip (B = 32, G = 16, S = 1, M = 255) on which (0, -1) and (0, 0) have mean differences that
    float32 division cannot tell apart while the integers can: cost(0,0) * cnt(0,-1) < cost(0,-1) * cnt(0,0), and the
    two float32 quotients are equal - the earlier displacement (0, -1) keeps the tie in float32, the contract takes (0, 0).
    Rows alternate 0 / 200 in both frames, so every dy != 0 costs about 200 a pixel; column 48 of the source is bright,
    so dx = +1 loses too."""
    rng = np.random.default_rng(7)
    H = W = 64
    tgt = np.zeros((H, W), np.int64)
    tgt[1::2] = 200
    holes = [(5, 9), (6, 20), (11, 3), (17, 30), (30, 14)]                 # all in block (0, 0), none in column 0
    mask = np.zeros((2, H, W), np.uint8)
    for y, x in holes:
        mask[0, y, x] = 255
    e = rng.integers(20, 40, size=(H, W))
    e[:, 48] = 55
    for y, x in holes:                                                      # the bytes that arrive tell the two apart
        e[y, x - 1], e[y, x] = 21, 38
    kt = mask[0, :48, :48] == 0
    cnt_b = int(kt.sum())                                                   # (0, 0): the whole window
    cnt_a = int(kt[:, 1:].sum())                                            # (0, -1): column 0 has no partner
    cost_a = int((e[:48, 0:47] * kt[:, 1:]).sum())
    base_b = int((e[:48, 0:47] * kt[:, 0:47]).sum())                        # (0, 0) without column 47
    # rows 32..47, columns 0..46 of e count in both sums: `extra` more there, then column 47 (in (0, 0)'s sum only)
    found = None
    for extra in range(16 * 47 * 15):
        a = cost_a + extra
        b = (a * cnt_b - 1) // cnt_a                                        # the largest cost with b / cnt_b < a / cnt_a
        if np.float32(a) / np.float32(cnt_a) <= np.float32(b) / np.float32(cnt_b) and 0 <= b - base_b - extra <= 48 * 55:
            found = (extra, b - base_b - extra)
            break
    assert found is not None
    q, r = divmod(found[0], 16 * 47)
    e[32:48, 0:47] += q
    flat = np.argwhere(np.ones((16, 47), bool))[:r]
    e[32 + flat[:, 0], flat[:, 1]] += 1
    q, r = divmod(found[1], 48)
    e[:48, 47] = q
    e[:r, 47] += 1
    assert e.max() <= 55
    src = tgt + e
    frames = np.stack([tgt, src]).astype(np.uint8)[..., None]
    return frames, mask, dict(block=32, margin=16, radius=1, search=1, max_mad=255)


def mutant_cases():
    """name -> (frames [n,H,W,C], masks [n,H,W], params): the small cases the mutants are judged on."""
    out = {}
    noisy, _ = pan_clip(3, 40, 48, 3, seed=3)
    m = random_block_masks(3, 40, 48, 8, 0.3, seed=4)
    out["pan"] = (holed(noisy, m, seed=5), m, dict(block=8, margin=8, radius=1, search=4, max_mad=6))
    # constant frames with a tint per frame: every displacement ties, the raster order alone decides which pixels
    # frame 0 can give (the others come from frame 2, in its tint)
    frames = np.empty((3, 24, 24, 3), np.uint8)
    for t, tint in enumerate((100, 101, 102)):
        frames[t] = tint
    m = np.zeros((3, 24, 24), np.uint8)
    m[1, 8:16, 8:16] = 255
    m[0, 4:12, 4:12] = 255
    m[2, 0:3, 0:3] = 255
    out["tint"] = (frames, m, dict(block=8, margin=8, radius=1, search=2, max_mad=6))
    # after frame 0 gave rows 14 and 15 of the hole in its tint, those rows are context that frame 2 cannot match:
    # the displacements that keep them out of P(d) win
    m = np.zeros((3, 24, 24), np.uint8)
    m[1, 8:16, 8:16] = 255
    m[0, 4:12, 4:24] = 255
    m[2, 14:20, 8:16] = 255
    m[2, 6:8, 6:14] = 255
    out["tint_context"] = (frames, m, dict(block=8, margin=8, radius=1, search=2, max_mad=6))
    # frame 0 knows the block and two columns on either side of it, an exact copy: 32 context pixels of 512
    noisy, _ = pan_clip(2, 32, 32, 1, seed=8, step=(0, 0), sigma=8.0)
    m = np.zeros((2, 32, 32), np.uint8)
    m[1, 8:16, 8:16] = 255
    noisy[0] = noisy[1]
    m[0] = 255
    m[0, 8:16, 6:18] = 0
    noisy[1, 8:16, 8:16] = 0
    out["sliver"] = (noisy, m, dict(block=8, margin=8, radius=1, search=7, max_mad=2))
    # two unrelated frames: nothing is accepted
    a, _ = pan_clip(1, 32, 32, 3, seed=10)
    b, _ = pan_clip(1, 32, 32, 3, seed=11)
    m = np.zeros((2, 32, 32), np.uint8)
    m[0, 8:24, 8:24] = 255
    out["strangers"] = (np.concatenate([a, b]), m, dict(block=16, margin=8, radius=1, search=3, max_mad=6))
    out["near_tie"] = near_tie_case()
    out["contrast"] = contrast_case()
    return out


def contrast_case():
    """cost * cnt above 2^32: B = 32, G = 16, two frames of 0 / 255 noise (a mean difference of about 128 a channel
    between strangers) on a 4096-pixel window, max_mad 255."""
    rng = np.random.default_rng(13)
    frames = (rng.integers(0, 2, size=(2, 96, 96, 3)) * 255).astype(np.uint8)
    # frame 1 is frame 0 moved by (1, 2) with 23 % of its values flipped: about 3.0e9 at the true displacement, below
    # 2^32, and about 6.4e9 everywhere else - 2.1e9 once wrapped
    flip = (rng.random((96, 96, 3)) < 0.23) * np.uint8(255)
    frames[1] = np.roll(frames[0], (1, 2), axis=(0, 1)) ^ flip
    m = np.zeros((2, 96, 96), np.uint8)
    m[0, 34:38, 40:44] = 255                                               # block (32, 32): the window is 64 x 64
    return frames, m, dict(block=32, margin=16, radius=1, search=3, max_mad=255)


# ----------------------------------------------------------------------------- the GPU test's matrix
def cases():
    """name -> (frames, masks, params): the matrix of tests/test_gpu_tfill.py - the mutants' cases and clips of at most
    5 x 48 x 64 (only `contrast` is larger, 2 x 96 x 96: a 64 x 64 window needs a block with 16 pixels on every side)."""
    out = dict(mutant_cases())
    d = DEFAULTS

    def pan(n, h, w, c, seed, frac=0.3, mb=None, **kw):
        p = dict(d, **kw)
        noisy, _ = pan_clip(n, h, w, c, seed=seed)
        m = random_block_masks(n, h, w, mb or p["block"], frac, seed=seed + 1)
        return holed(noisy, m, seed=seed + 2), m, p

    out["tiny_5x7"] = pan(3, 5, 7, 3, 20, frac=0.5, block=8, margin=0, mb=2)             # nk < MIN_CONTEXT everywhere
    f, m, p = pan(2, 16, 16, 3, 21)
    m[:] = 0
    m[0] = 255                                                                           # its one block removed: nk = 0
    out["one_block_16x16"] = (f, m, p)
    for c in (1, 3):
        # without a margin the window is the block: 64 pixels, fewer than MIN_CONTEXT known once one is a hole
        out[f"b8_g0_24x40_c{c}"] = pan(5, 24, 40, c, 22 + c, block=8, margin=0, search=3, radius=1, mb=2)
        out[f"ragged_33x49_c{c}"] = pan(5, 33, 49, c, 25 + c)                            # windows cut by every frame edge
    out["b32_g16_48x64"] = pan(5, 48, 64, 3, 30, frac=0.4, block=32, margin=16, radius=3, mb=8)
    out["defaults_48x64"] = pan(5, 48, 64, 3, 31)
    out["n1_no_sources"] = pan(1, 24, 40, 3, 32)
    out["n2_radius3"] = pan(2, 24, 40, 3, 33, radius=3)                                  # R > n
    out["radius0"] = pan(3, 24, 40, 3, 34, radius=0)
    out["search0"] = pan(3, 24, 40, 1, 35, search=0, max_mad=40)
    out["search3"] = pan(3, 33, 49, 3, 36, search=3)
    out["block1"] = pan(2, 13, 15, 1, 37, frac=0.1, block=1, margin=4, search=3, mb=1)   # MIN_CONTEXT needs 64 of <= 81
    out["block5_g3"] = pan(3, 24, 40, 3, 38, block=5, margin=3, search=5, mb=5)
    rng = np.random.default_rng(40)
    noisy, _ = pan_clip(5, 33, 49, 3, seed=41)
    m = ((rng.random((5, 33, 49)) < 0.35) * 255).astype(np.uint8)                        # random pixel masks
    out["pixel_masks"] = (holed(noisy, m, seed=42), m, dict(d))
    m = ((rng.random((3, 24, 40)) < 0.5) * np.array([1, 2, 255], np.uint8)[:, None, None]).astype(np.uint8)
    out["mask_values_1_2_255"] = (holed(pan_clip(3, 24, 40, 1, seed=43)[0], m, seed=44), m, dict(d, block=8))
    f, m, p = pan(5, 33, 49, 3, 45)
    m[2] = 255                                                                           # a frame that is all hole
    out["all_hole_frame"] = (holed(f, m, seed=46), m, p)
    f, m, p = pan(3, 33, 49, 3, 47)
    out["no_holes"] = (f, np.zeros_like(m), p)
    noisy, _ = pan_clip(5, 48, 64, 3, seed=48)
    m = np.repeat(random_block_masks(1, 48, 64, 16, 0.3, seed=49), 5, axis=0)            # the same mask in every frame:
    out["same_mask_every_frame"] = (holed(noisy, m, seed=50), m, dict(d))                # the pan uncovers strips only
    return out
