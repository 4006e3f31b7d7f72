"""The numpy statement behind elvis_amd/enhance.py and csrc/sr_enhance.hip: cv2's 8-bit INTER_LANCZOS4 resize at any
ratio in exact int64, `RealESRGANer.tile_process` as its literal double loop, the reflect paddings of `pre_process` as
index maps, and the composition of the three around any `forward`.  Every function takes a `mutant` that breaks one
rule; tests/test_enhance_ledger.py shows that the stated inputs tell each one apart.

The coefficients are `classical.lanczos4_coeffs` (cv::interpolateLanczos4, pinned by the classical tests)."""
import math
import re

import numpy as np

from elvis_amd.classical import lanczos4_coeffs

MUTANTS = ("round0", "clamp", "trunc", "edge", "crop_no_s")

# (hs, ws, hd, wd): the resize cases of tests/test_gpu_enhance.py
RESIZE_CASES = {
    "down2": (16, 24, 8, 12),
    "down4": (32, 48, 8, 12),
    "up2": (8, 12, 16, 24),
    "mixed": (13, 17, 9, 31),
    "identity": (8, 12, 8, 12),
    "narrow": (3, 5, 7, 2),
    "degenerate": (1, 1, 4, 4),
    # one more than the workgroup's destination tile in each direction: 16 x 64 at a mild ratio (c = 1 and 3), 16 x 32 at
    # 4:1 with three channels (one channel still fits 16 x 64 there: a single partial tile)
    "tile16x64_plus1": (20, 70, 17, 65),
    "tile16x32_plus1": (68, 132, 17, 33),
}
RESIZE_TILE_OF = {("tile16x64_plus1", 1): (16, 64), ("tile16x64_plus1", 3): (16, 64), ("tile16x32_plus1", 3): (16, 32),
                  ("tile16x32_plus1", 1): (16, 64)}
# the channel counts every resize case runs with, and the case that also runs the other two the entry point takes
CHANNELS = (3, 1)
EXTRA_CHANNELS = {"mixed": (2, 4)}
# the 9 x 13 image of test_enhance_host_and_outscale through an x4 network, and the sizes its outscales give
OUTSCALE_SOURCE = (9, 13)
OUTSCALES = {2: (18, 26), 3: (27, 39), 2.5: (22, 32), 1: (9, 13)}


def gpu_resizes():
    """(hs, ws, hd, wd) of every resize the cases of tests/test_gpu_enhance.py launch: the resize cases, the outscales, the
    naive and Presley compositions on 12 x 20 frames, and the 2x stages of an x4 network from 8 x 12 and 16 x 24."""
    out = list(RESIZE_CASES.values())
    H, W = OUTSCALE_SOURCE
    out += [(4 * H, 4 * W, hd, wd) for hd, wd in OUTSCALES.values()]
    out += [(48, 80, 12, 20), (48, 80, 36, 60), (36, 60, 12, 20)]
    out += [(32, 48, 16, 24), (64, 96, 32, 48)]
    return out


# (n_src, n_dst) per axis of what the paths produce: enhance(outscale=2) and the resize back of an x4 and an x2 network at
# 1080p and at the test sizes, Presley's levels 1..4 (x4 -> level, then back to 1)
DRIVER_RATIOS = [(4320, 2160), (7680, 3840), (4320, 1080), (7680, 1920), (2160, 1080), (3840, 1920), (4320, 3240), (7680, 5760),
                 (3240, 1080), (5760, 1920), (2160, 4320), (3840, 7680), (32, 16), (48, 24), (64, 32), (96, 48), (128, 32), (192, 48),
                 (64, 48), (96, 72), (48, 16), (72, 24), (36, 18), (52, 26), (36, 27), (52, 39), (27, 9), (39, 13), (36, 9), (52, 13)]


def taps(n_src, n_dst, mutant=None):
    """(first int64 [n_dst], taps int64 [n_dst, 8]) of one axis."""
    scale = float(n_src) / float(n_dst)
    first = np.zeros(n_dst, np.int64)
    t = np.zeros((n_dst, 8), np.int64)
    for d in range(n_dst):
        fx = np.float32((d + 0.5) * scale - 0.5)
        sx = int(fx) if mutant == "trunc" else int(math.floor(fx))
        first[d] = sx - 3
        t[d] = np.rint(lanczos4_coeffs(np.float32(fx - np.float32(sx))) * np.float32(2048)).astype(np.int64)
    return first, t


def resize_raw(src, hd, wd, mutant=None):
    """The exact integer sum_ky sum_kx p * tx * ty of every destination pixel, int64 [n, hd, wd, c]."""
    n, hs, ws, c = src.shape
    xf, xt = taps(ws, wd, mutant)
    yf, yt = taps(hs, hd, mutant)
    hi_x, hi_y = (max(ws - 2, 0), max(hs - 2, 0)) if mutant == "clamp" else (ws - 1, hs - 1)
    ix = np.clip(xf[:, None] + np.arange(8), 0, hi_x)                  # [wd, 8]
    iy = np.clip(yf[:, None] + np.arange(8), 0, hi_y)                  # [hd, 8]
    p = src.astype(np.int64)
    mid = (p[:, :, ix, :] * xt[None, None, :, :, None]).sum(3)         # [n, hs, wd, c]
    return (mid[:, iy] * yt[None, :, :, None, None]).sum(2)            # [n, hd, wd, c]


def resize(src, hd, wd, mutant=None):
    """cv2.resize(src, (wd, hd), interpolation=cv2.INTER_LANCZOS4) of uint8 [n, hs, ws, c]; equal sizes: a copy."""
    if src.shape[1:3] == (hd, wd):
        return src.copy()
    raw = resize_raw(src, hd, wd, mutant)
    return np.clip((raw + (0 if mutant == "round0" else 1 << 21)) >> 22, 0, 255).astype(np.uint8)


def resize_inputs(name, c, kind, n=2):
    hs, ws, _, _ = RESIZE_CASES[name]
    if kind == "random":
        seed = sum(ord(ch) for ch in name) * 10 + c
        return np.random.default_rng(seed).integers(0, 256, size=(n, hs, ws, c), dtype=np.uint8)
    cell = 4 if min(hs, ws) >= 8 else 1
    y, x = np.mgrid[0:hs, 0:ws]
    board = ((((y // cell) + (x // cell)) % 2) * 255).astype(np.uint8)
    out = np.stack([board, 255 - board][:n] if n <= 2 else [board] * n)
    return np.ascontiguousarray(np.repeat(out[..., None], c, 3))


def sum_bound(xt, yt):
    """255 * max(Px * Py + Nx * Ny) + 2^21 by brute force over all pairs of rows of the two tables."""
    px, nx = np.maximum(xt, 0).sum(1), np.maximum(-xt, 0).sum(1)
    py, ny = np.maximum(yt, 0).sum(1), np.maximum(-yt, 0).sum(1)
    return 255 * int((px[:, None] * py[None] + nx[:, None] * ny[None]).max()) + (1 << 21)


def index_maps(H, W, pre_pad, mod, mutant=None):
    """Row and column maps of F.pad(img, (0, pre_pad, 0, pre_pad), 'reflect') followed by the reflect pad to a
    multiple of `mod` of the padded image."""
    def right(idx, p):
        k = np.arange(p)
        return np.concatenate([idx, idx[len(idx) - (1 if mutant == "edge" else 2) - k]])
    maps = []
    for size in (H, W):
        idx = right(np.arange(size), pre_pad)
        idx = right(idx, (-len(idx)) % mod)
        maps.append(idx)
    return maps


def plan_tiles(H, W, tile, tile_pad, s, mutant=None):
    """tile_process, line by line: per tile (input box y0, x0, h, w; crop origin cy, cx in the output tile; output origin
    oy, ox; output size oh, ow)."""
    if tile == 0:
        return [(0, 0, H, W, 0, 0, 0, 0, H * s, W * s)]
    out = []
    tiles_x = math.ceil(W / tile)
    tiles_y = math.ceil(H / tile)
    for y in range(tiles_y):
        for x in range(tiles_x):
            ofs_x = x * tile
            ofs_y = y * tile
            input_start_x = ofs_x
            input_end_x = min(ofs_x + tile, W)
            input_start_y = ofs_y
            input_end_y = min(ofs_y + tile, H)
            input_start_x_pad = max(input_start_x - tile_pad, 0)
            input_end_x_pad = min(input_end_x + tile_pad, W)
            input_start_y_pad = max(input_start_y - tile_pad, 0)
            input_end_y_pad = min(input_end_y + tile_pad, H)
            input_tile_width = input_end_x - input_start_x
            input_tile_height = input_end_y - input_start_y
            k = 1 if mutant == "crop_no_s" else s
            output_start_x_tile = (input_start_x - input_start_x_pad) * k
            output_start_y_tile = (input_start_y - input_start_y_pad) * k
            out.append((input_start_y_pad, input_start_x_pad, input_end_y_pad - input_start_y_pad, input_end_x_pad - input_start_x_pad,
                        output_start_y_tile, output_start_x_tile, input_start_y * s, input_start_x * s,
                        input_tile_height * s, input_tile_width * s))
    return out


def compose(frames, forward, s, tile, tile_pad, pre_pad=0, mod=1, mutant=None):
    """pre_process, tile_process, post_process around `forward` ([n, h, w, 3] uint8 -> [n, s*h, s*w, 3] uint8)."""
    n, H, W, _ = frames.shape
    rows, cols = index_maps(H, W, pre_pad, mod, mutant)
    padded = frames[:, rows][:, :, cols]
    Hp, Wp = len(rows), len(cols)
    out = np.zeros((n, s * Hp, s * Wp, 3), np.uint8)
    for (y0, x0, h, w, cy, cx, oy, ox, oh, ow) in plan_tiles(Hp, Wp, tile, tile_pad, s, mutant):
        sr = forward(np.ascontiguousarray(padded[:, y0:y0 + h, x0:x0 + w]))
        out[:, oy:oy + oh, ox:ox + ow] = sr[:, cy:cy + oh, cx:cx + ow]
    return out[:, :s * H, :s * W]


def nearest_forward(s):
    """A stand-in network for the CPU tests: every pixel repeated s x s, plus a ramp that makes a shifted crop differ."""
    def forward(x):
        up = np.repeat(np.repeat(x, s, 1), s, 2).astype(np.int64)
        yy, xx = np.mgrid[0:up.shape[1], 0:up.shape[2]]
        return ((up + (3 * yy + 7 * xx)[None, :, :, None]) % 256).astype(np.uint8)
    return forward


def kernel_names(lib_path, source_path):
    """The kernels of one source file in the built library, integer template arguments spelled out:
    `resize_lanczos4_u8_kernel<3>`."""
    from _glueref import elf_symbols, kernel_stems
    stems = kernel_stems(source_path)
    names = set()
    for sym in elf_symbols(lib_path):
        t = re.match(r"_Z(?:N12_GLOBAL__N_1)?(\d+)", sym)
        if not t:
            continue
        ln, pos = int(t.group(1)), t.end()
        name, rest = sym[pos:pos + ln], sym[pos + ln:]
        if name not in stems:
            continue
        i = re.match(r"ILi(\d+)EE", rest)
        names.add(f"{name}<{i.group(1)}>" if i else name)
    return names
