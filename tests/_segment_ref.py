"""The foreground segmenter of elvis_amd/segment.py (csrc/segment.hip), stated in numpy: int64 throughout, one float64
threshold search.  BUILD-DEFINED and training-free; it stands in UFO's slot and claims no parity with UFO.  The device
equals every array below byte for byte (tests/test_gpu_segment.py).

The clip a call sees is `before + frames + after` (the "extended" clip, m frames).  Every stage up to the cleaned mask
runs on all m frames; the vote, the fallback and the upsample on the `frames` alone.  Frame e > 0 of the extended clip
is paired with e - 1, frame 0 with frame 1: with two frames of `before` the first is a partner only (its own mask is
computed against the wrong partner and read by nobody), with one it is the clip's true first frame.
"""
from dataclasses import dataclass

import numpy as np

Q = 4                       # the reduction: one reduced pixel is the sum of Q x Q pixels
SHARE_DEN = 10000           # max_share is compared in integers, to four decimals
SHIFT, HALF = 20, 1 << 19


@dataclass
class SegmentConfig:
    radius: int = 8
    motion_weight: int = 2
    spatial_weight: int = 1
    motion_floor: int = 864          # 16 * 9 * 6: nine reduced pixels, six grey levels a pixel
    spatial_floor: int = 384         # 16 * 24
    min_peak: int = 48
    dilation: int = 1
    max_share: float = 0.7
    temporal_vote: bool = True


# ----------------------------------------------------------------------------- 1. reduce
def yuv(frames, order="rgb"):
    """[n,H,W,C] u8 -> int64 [n,H,W,3]: Y, U, V by i420_y / i420_u / i420_v of csrc/i420.h; C == 1 is Y, U = V = 128."""
    f = np.asarray(frames).astype(np.int64)
    if f.shape[3] == 1:
        return np.stack([f[..., 0], np.full_like(f[..., 0], 128), np.full_like(f[..., 0], 128)], axis=-1)
    r, g, b = (f[..., 0], f[..., 1], f[..., 2]) if order == "rgb" else (f[..., 2], f[..., 1], f[..., 0])
    y = (269484 * r + 528482 * g + 102760 * b + HALF + (16 << SHIFT)) >> SHIFT
    u = (-155188 * r - 305135 * g + 460324 * b + HALF + (128 << SHIFT)) >> SHIFT
    v = (460324 * r - 385875 * g - 74448 * b + HALF + (128 << SHIFT)) >> SHIFT
    return np.stack([y, u, v], axis=-1)


def reduce(frames, order="rgb"):
    """int64 [n, H // 4, W // 4, 3]: the sum over each 4 x 4 cell; pixels past the last whole cell take no part."""
    p = yuv(frames, order)
    n, h, w, _ = p.shape
    ry, rx = h // Q, w // Q
    return p[:, :ry * Q, :rx * Q].reshape(n, ry, Q, rx, Q, 3).sum(axis=(2, 4))


# ----------------------------------------------------------------------------- 2. global motion
def sad_table(c, o, radius):
    """int64 [2R+1, 2R+1]: entry (dy + R, dx + R) is sum |c[y, x] - o[y + dy, x + dx]| over the window
    y in [R, Ry - R), x in [R, Rx - R) - the same window for every candidate."""
    ry, rx = c.shape
    r = radius
    win = c[r:ry - r, r:rx - r]
    d = 2 * r + 1
    table = np.zeros((d, d), np.int64)
    for i in range(d):
        for j in range(d):
            table[i, j] = np.abs(win - o[i:i + ry - 2 * r, j:j + rx - 2 * r]).sum()
    return table


def pick_shift(table, radius):
    """The least (sad, dy*dy + dx*dx, dy, dx), lexicographically."""
    best = None
    for i in range(table.shape[0]):
        for j in range(table.shape[1]):
            dy, dx = i - radius, j - radius
            key = (int(table[i, j]), dy * dy + dx * dx, dy, dx)
            if best is None or key < best:
                best = key
    return best[2], best[3]


# ----------------------------------------------------------------------------- 3. motion residual
def _box(a, k):
    """The (2k+1) x (2k+1) sum with edge replication."""
    p = np.pad(a, k, mode="edge")
    out = np.zeros_like(a)
    for i in range(2 * k + 1):
        for j in range(2 * k + 1):
            out += p[i:i + a.shape[0], j:j + a.shape[1]]
    return out


def residual(c, o, dy, dx):
    """res: the least |c[y, x] - o| over the 3 x 3 around (y + dy, x + dx), coordinates clamped; 0 where
    (y + dy, x + dx) itself lies outside the frame."""
    ry, rx = c.shape
    yy, xx = np.mgrid[0:ry, 0:rx]
    res = None
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            d = np.abs(c - o[np.clip(yy + dy + a, 0, ry - 1), np.clip(xx + dx + b, 0, rx - 1)])
            res = d if res is None else np.minimum(res, d)
    inside = (yy + dy >= 0) & (yy + dy < ry) & (xx + dx >= 0) & (xx + dx < rx)
    return np.where(inside, res, 0)


def motion_term(c, o, dy, dx):
    return _box(residual(c, o, dy, dx), 1)


def normalise(v, floor):
    return np.minimum(255, v * 255 // max(int(v.max()), int(floor)))


# ----------------------------------------------------------------------------- 4. spatial term
def strip_means(red):
    """int64 [4, 3]: the mean colour (sum // count) of the top, bottom, left and right border strips."""
    ry, rx, _ = red.shape
    bw = max(1, min(ry, rx) // 16)
    strips = (red[:bw], red[ry - bw:], red[:, :bw], red[:, rx - bw:])
    return np.stack([s.reshape(-1, 3).sum(axis=0) // (s.shape[0] * s.shape[1]) for s in strips])


def spatial_term(red):
    means = strip_means(red)
    return np.abs(red[:, :, None, :] - means[None, None]).sum(axis=3).min(axis=2)


# ----------------------------------------------------------------------------- 5, 6. fuse and threshold
def fuse(mn, sn, cfg):
    if mn is None:
        f = sn
    else:
        f = (cfg.motion_weight * mn + cfg.spatial_weight * sn) // (cfg.motion_weight + cfg.spatial_weight)
    return _box(f, 2) // 25


def otsu(hist):
    """float64, in this order; 255 when no candidate splits the histogram."""
    h = np.asarray(hist, np.float64)
    n = float(h.sum())
    tot = float((h * np.arange(256)).sum())
    w0 = s0 = 0.0
    best_v, best_t = -1.0, 255
    for t in range(255):
        w0 += h[t]
        s0 += h[t] * t
        w1 = n - w0
        if w0 == 0 or w1 == 0:
            continue
        d = tot * w0 - s0 * n
        v = d * d / (w0 * w1)
        if v > best_v:
            best_v, best_t = v, t
    return best_t


def threshold(f, cfg):
    """The threshold as the mask uses it: 255 (nothing is above it) where max(F) < min_peak."""
    if int(f.max()) < cfg.min_peak:
        return 255
    return otsu(np.bincount(f.ravel(), minlength=256))


# ----------------------------------------------------------------------------- 7. clean
def _morph(m, dilate):
    p = np.pad(m, 1, mode="edge")
    out = m.copy()
    for i in range(3):
        for j in range(3):
            s = p[i:i + m.shape[0], j:j + m.shape[1]]
            out = np.maximum(out, s) if dilate else np.minimum(out, s)
    return out


def clean(mask, dilation):
    m = mask.astype(np.int64)
    for dilate in (True, False, False, True) + (True,) * dilation:
        m = _morph(m, dilate)
    return m


# ----------------------------------------------------------------------------- 8-10. vote, fallback, upsample
def vote(pre, e, m):
    """pre: [m, Ry, Rx]; frame e of the extended clip with both neighbours present."""
    if e - 1 < 0 or e + 1 >= m:
        return pre[e]
    return (pre[e - 1] + pre[e] + pre[e + 1] >= 2).astype(np.int64)


def share_num(max_share):
    return int(round(float(max_share) * SHARE_DEN))


def fallback(mask, max_share):
    """All ones where the foreground share is 0 or above max_share (to four decimals, in integers)."""
    cnt = int(mask.sum())
    if cnt == 0 or cnt * SHARE_DEN > share_num(max_share) * mask.size:
        return np.ones_like(mask)
    return mask


def upsample(mask, h, w):
    ry, rx = mask.shape
    return mask[np.minimum(np.arange(h) // Q, ry - 1)][:, np.minimum(np.arange(w) // Q, rx - 1)].astype(np.uint8)


# ----------------------------------------------------------------------------- the whole statement
def segment(frames, order="rgb", cfg=None, before=None, after=None, details=False):
    """frames [n,H,W,C] u8 -> u8 [n,H,W] of 0 / 1; with details=True also a dict of every intermediate over the
    extended clip: red [m,Ry,Rx,3], sad [m,D,D], shift [m,2], M, S, Mn, Sn, F, pre [m,Ry,Rx], thr [m]."""
    cfg = SegmentConfig() if cfg is None else cfg
    frames = np.asarray(frames)
    parts = [np.asarray(p) for p in (before, frames, after) if p is not None and len(p)]
    nb = 0 if before is None else len(before)
    ext = np.concatenate(parts, axis=0)
    m, h, w, _ = ext.shape
    n = frames.shape[0]
    r = cfg.radius
    red = reduce(ext, order)
    ry, rx = red.shape[1:3]
    d = 2 * r + 1
    sad = np.zeros((m, d, d), np.int64)
    shift = np.zeros((m, 2), np.int64)
    mn = np.zeros((m, ry, rx), np.int64)
    sn, f, pre, mraw, sraw = (np.zeros_like(mn) for _ in range(5))
    thr = np.zeros(m, np.int64)
    for e in range(m):
        c = red[e, :, :, 0]
        if m > 1:
            o = red[e - 1 if e > 0 else 1, :, :, 0]
            sad[e] = sad_table(c, o, r)
            shift[e] = pick_shift(sad[e], r)
            mraw[e] = motion_term(c, o, *shift[e])
            mn[e] = normalise(mraw[e], cfg.motion_floor)
        sraw[e] = spatial_term(red[e])
        sn[e] = normalise(sraw[e], cfg.spatial_floor)
        f[e] = fuse(mn[e] if m > 1 else None, sn[e], cfg)
        thr[e] = threshold(f[e], cfg)
        pre[e] = clean(f[e] > thr[e], cfg.dilation)
    out = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        e = nb + i
        v = vote(pre, e, m) if cfg.temporal_vote else pre[e]
        out[i] = upsample(fallback(v, cfg.max_share), h, w)
    if not details:
        return out
    return out, dict(red=red, sad=sad, shift=shift, M=mraw, S=sraw, Mn=mn, Sn=sn, F=f, pre=pre, thr=thr)


# ----------------------------------------------------------------------------- the scenes of the checks
def scene(pan, move, noise, n=6, h=240, w=320, obj=(64, 96), seed=0):
    """A field of random 8 x 8 colour patches panning by `pan` = (py, px) pixels a frame, with a rectangle of its own
    colour and texture moving over it by `move` a frame, and uniform noise up to +-`noise`.  Returns (frames u8
    [n,h,w,3] RGB, boxes [(y0, x0, y1, x1)] of the object per frame).  `pan` is the camera's: the view moves over the
    world by +pan a frame, frame_t[y, x] = world[y + t py, x + t px], so against frame t - 1 the content of frame t is
    found at (y + py, x + px) and the shift the statement recovers is (+py, +px) / 4 (frame 0, paired with frame 1:
    the negative).  `move` is the object's step in frame coordinates."""
    rng = np.random.default_rng(seed)
    py, px = pan
    my, mx = move
    margin_y, margin_x = abs(py) * n + 8, abs(px) * n + 8
    wh, ww = h + 2 * margin_y, w + 2 * margin_x
    patches = rng.integers(40, 216, size=((wh + 7) // 8, (ww + 7) // 8, 3))
    world = np.repeat(np.repeat(patches, 8, axis=0), 8, axis=1)[:wh, :ww]
    oh, ow = obj
    # the object: a saturated colour no patch has, with a fine checker texture of its own
    yy, xx = np.mgrid[0:oh, 0:ow]
    tex = (((yy // 4) + (xx // 4)) % 2) * 30
    body = np.stack([235 - tex, 20 + tex // 2, 20 + tex], axis=-1)
    y0 = (h - oh) // 2 - my * (n // 2)
    x0 = (w - ow) // 2 - mx * (n // 2)
    frames = np.zeros((n, h, w, 3), np.uint8)
    boxes = []
    for t in range(n):
        oy, ox = margin_y + t * py, margin_x + t * px
        img = world[oy:oy + h, ox:ox + w].copy()
        by, bx = y0 + t * my, x0 + t * mx
        img[by:by + oh, bx:bx + ow] = body
        if noise:
            img = img + rng.integers(-noise, noise + 1, size=img.shape)
        frames[t] = np.clip(img, 0, 255).astype(np.uint8)
        boxes.append((by, bx, by + oh, bx + ow))
    return frames, boxes


SCENES = {                              # (background pan, object motion, noise)
    "pan_x4_obj_4_-4": ((0, 4), (4, -4), 0),
    "pan_4_8_obj_0_8": ((4, 8), (0, 8), 2),
    "static_obj_4_4": ((0, 0), (4, 4), 2),
    "static_static": ((0, 0), (0, 0), 2),
    "pan_4_4_obj_-4_0": ((4, 4), (-4, 0), 3),
}
BLOCK = 16


def scene_conditions(masks, boxes, block=BLOCK):
    """The two conditions on the block grid (`resize_masks_nearest`: block (i, j) reads pixel (i block, j block)):
    (every block wholly inside the object is foreground in every frame, no block two or more blocks away from the
    blocks the object touches is foreground in any frame)."""
    n, h, w = masks.shape
    by, bx = h // block, w // block
    grid = masks[:, (np.arange(by) * h) // by][:, :, (np.arange(bx) * w) // bx]
    inside_ok = far_ok = True
    for t, (y0, x0, y1, x1) in enumerate(boxes):
        inside = np.zeros((by, bx), bool)
        inside[-(-y0 // block):y1 // block, -(-x0 // block):x1 // block] = True
        near = np.zeros((by, bx), bool)
        near[max(0, y0 // block - 1):-(-y1 // block) + 1, max(0, x0 // block - 1):-(-x1 // block) + 1] = True
        inside_ok &= bool(inside.any() and grid[t][inside].all())
        far_ok &= not grid[t][~near].any()
    return inside_ok, far_ok


def pan_clip(n, h, w, c, step, seed=0, noise=0, flat=None):
    """A random texture (4 x 4 patches: one value a reduced pixel) seen by a camera that moves by `step` = (sy, sx)
    REDUCED pixels a frame: the statement recovers (sy, sx) for every frame but the first, (-sy, -sx) for that.
    `flat`: a constant clip of that value instead."""
    rng = np.random.default_rng(seed)
    if flat is not None:
        return np.full((n, h, w, c), flat, np.uint8)
    sy, sx = step
    my, mx = abs(sy) * Q * n, abs(sx) * Q * n
    cells = rng.integers(30, 226, size=((h + 2 * my) // Q + 2, (w + 2 * mx) // Q + 2, c))
    world = np.repeat(np.repeat(cells, Q, axis=0), Q, axis=1)
    out = np.zeros((n, h, w, c), np.uint8)
    for t in range(n):
        oy, ox = my + t * sy * Q, mx + t * sx * Q
        img = world[oy:oy + h, ox:ox + w]
        if noise:
            img = img + rng.integers(-noise, noise + 1, size=img.shape)
        out[t] = np.clip(img, 0, 255)
    return out


def object_clip(n, h, w, c, seed=0, step=(0, 1), move=(1, 0), noise=2):
    """`pan_clip` with a dark rectangle of a third of the frame moving over it by `move` reduced pixels a frame."""
    rng = np.random.default_rng(seed + 1000)
    out = pan_clip(n, h, w, c, step, seed, noise=0).astype(np.int64)
    oh, ow = max(Q, h // 3), max(Q, w // 3)
    for t in range(n):
        y0 = min(max(0, h // 3 + t * move[0] * Q), h - oh)
        x0 = min(max(0, w // 3 + t * move[1] * Q), w - ow)
        out[t, y0:y0 + oh, x0:x0 + ow] = [250, 10, 10][:c] if c == 3 else [5]
        out[t] += rng.integers(-noise, noise + 1, size=out[t].shape)
    return np.clip(out, 0, 255).astype(np.uint8)


def framed_clip(n, h, w, c):
    """A one-colour border one reduced pixel wide around an interior of another colour, a little of it moving: more
    than max_share of the frame stands apart from the border."""
    out = np.full((n, h, w, c), 40, np.uint8)
    bw = Q * max(1, min(h // Q, w // Q) // 16)
    for t in range(n):
        out[t, bw:h - bw, bw:w - bw] = 200 + 5 * (t % 2)
    return out



# ----------------------------------------------------------------------------- the matrix of the device tests
def kernel_tiles():
    """(kSadTileY, kSadTileX, kTile, kMorphTile) as csrc/segment.hip has them."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    source = open(os.path.join(root, "elvis_amd", "csrc", "segment.hip")).read()
    return tuple(int(re.search(rf"\b{k} = (\d+)\b", source).group(1)) for k in ("kSadTileY", "kSadTileX", "kTile", "kMorphTile"))


def tile_edges(radius=2):
    """The smallest frames (H, W) at which a kernel has a second tile in a direction: one reduced pixel more than a
    tile, for the SAD kernel a window (the frame less 2 R) of one more than a tile.  Pixels = 4 x reduced pixels."""
    sad_ty, sad_tx, tile, morph = kernel_tiles()
    return {
        "sad_rows": (Q * (sad_ty + 2 * radius + 1), 20),
        "sad_columns": (20, Q * (sad_tx + 2 * radius + 1)),
        "terms_fuse_rows": (Q * (tile + 1), 20),
        "terms_fuse_columns": (20, Q * (tile + 1)),
        "morph_rows": (Q * (morph + 1), 24),
        "morph_columns": (24, Q * (morph + 1)),
    }


def _cfg(**kw):
    return dict(dict(radius=2), **kw)


def cases(edges=None):
    """The matrix of tests/test_gpu_segment.py: name -> (frames, order, cfg fields).  R = 2 unless a name says otherwise."""
    edges = tile_edges() if edges is None else edges
    c = {}
    # the shapes: the smallest legal, the remainders (rows of 69 and 81 bytes), several tiles of every kernel, R = 8
    for (h, w) in ((20, 20), (21, 23), (22, 27), (48, 64)):
        for n in (1, 2, 3, 5):
            c[f"{h}x{w}_n{n}"] = (object_clip(n, h, w, 3, seed=h + n), "rgb", _cfg())
    c["72x130_r8_n3"] = (object_clip(3, 72, 130, 3, seed=9, step=(1, -2)), "rgb", _cfg(radius=8))
    c["72x130_r8_n1_c1"] = (object_clip(1, 72, 130, 1, seed=10), "rgb", _cfg(radius=8))
    for name, (h, w) in edges.items():
        c[f"edge_{name}_{h}x{w}"] = (object_clip(2, h, w, 3, seed=len(name)), "rgb", _cfg())
    c["all_tiles_133x282_n3"] = (object_clip(3, 133, 282, 3, seed=11, step=(-1, 2), move=(2, -1)), "bgr", _cfg())
    # the other factors
    c["c1_22x27_n3"] = (object_clip(3, 22, 27, 1, seed=12), "rgb", _cfg())
    c["c1_48x64_n5"] = (object_clip(5, 48, 64, 1, seed=13), "bgr", _cfg())          # the order does not matter for C = 1
    c["bgr_21x23_n3"] = (object_clip(3, 21, 23, 3, seed=14), "bgr", _cfg())
    c["bgr_48x64_n2"] = (object_clip(2, 48, 64, 3, seed=15), "bgr", _cfg())
    for d in (0, 1, 4):
        for vote in (False, True):
            c[f"dilation{d}_vote{int(vote)}_48x64_n5"] = (object_clip(5, 48, 64, 3, seed=16, move=(1, 2)), "rgb",
                                                          _cfg(dilation=d, temporal_vote=vote))
    c["dilation4_22x27_n3"] = (object_clip(3, 22, 27, 3, seed=17), "rgb", _cfg(dilation=4))
    c["r0_20x20_n2"] = (object_clip(2, 20, 20, 3, seed=18, step=(0, 0)), "rgb", _cfg(radius=0))
    c["r16_133x140_n2"] = (object_clip(2, 133, 140, 3, seed=19, step=(3, -5)), "rgb", _cfg(radius=16))
    c["weights_floors_48x64_n3"] = (object_clip(3, 48, 64, 3, seed=20), "rgb",
                                    _cfg(motion_weight=1, spatial_weight=3, motion_floor=100, spatial_floor=5000, min_peak=10,
                                         max_share=0.3))
    # the clips that force a branch
    c["flat_40x52_n3"] = (pan_clip(3, 40, 52, 3, None, flat=128), "rgb", _cfg())
    c["flat_40x52_n1_c1"] = (pan_clip(1, 40, 52, 1, None, flat=7), "rgb", _cfg())
    c["framed_48x64_n3"] = (framed_clip(3, 48, 64, 3), "rgb", _cfg())
    c["quiet_48x64_n3"] = (np.clip(pan_clip(3, 48, 64, 3, None, flat=100).astype(np.int64)
                                   + np.random.default_rng(21).integers(-1, 2, size=(3, 48, 64, 3)), 0, 255).astype(np.uint8),
                           "rgb", _cfg())
    c["shift_plus_r_minus_r_48x64_n3"] = (pan_clip(3, 48, 64, 3, (2, -2), seed=22, noise=1), "rgb", _cfg())
    c["shift_plus_r_minus_r_r8_100x112_n2"] = (pan_clip(2, 100, 112, 3, (8, -8), seed=23, noise=1), "rgb", _cfg(radius=8))
    return c
