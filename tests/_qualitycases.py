"""The edge matrix of csrc/quality.hip, importable without a GPU: the case list, the float64 expected values built on
tests/_quality_ref.py, a restatement of the kernel's geometry (work area, map, tiles, staged words) from which the ledger
(tests/test_quality_inpaint_ledger.py) derives what the cases reach, and the mutants - the reference with one clause
changed, each of which must move the value of a named small case by at least 1e-6, a thousand bars.

Every case is derived from a constant of the kernel: the 16 x 32 map tile and its 26 x 42 apron, the 4-byte words of the
wide staging and their shift, the `aligned` switch, the 11-tap threshold of VALID, the automatic window rule, the
8-byte words of the box scan and the 16 pixels a lane of the mask kernel takes.

The window contract the `asym` window pins (written above ssim_area in the source): REFLECT output i is
sum_k w[k] x[i - 5 + k], VALID output i is sum_k w[k] x[i + k] - what Q._taps_along computes.

Constants are the two evaluators' own (C1_255 / C2_255 with scale 1; 0.01^2 / 0.03^2 with scale 255), so the 1e-9 bar
of tests/test_gpu_quality.py holds unchanged: its derivation needs only a non-negative window of sum 1.
"""
import re
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import _quality_ref as Q
from _convref import elf_symbols
from _glueref import demangle_kernel, kernel_stems

BAR = 1e-9
TH, TW, ROWS, COLS, MAX_C = 16, 32, 26, 42, 4      # SSIM_TH, SSIM_TW, + 10 each; the ledger reads them from the source
BBOX_WORD, APPLY_GROUP, APPLY_THREADS = 8, 16, 256
SOURCES = ("quality.hip",)
SRC_NAMES, BORDER_NAMES = ("luma", "channels"), ("reflect", "valid")


# ============================================================================================ kernel names
def kernel_names(lib_path: str, source_path: str):
    """The kernels of one source file in the built library, spelled as elvis_last_launch spells them:
    `_Z16ssim_tile_kernelILi0ELi1EEv10SsimParams` -> `ssim_tile_kernel<luma,valid>`, `..ssim_finish_kernelILi1EE..`
    -> `ssim_finish_kernel<valid>`, `_ZN12_GLOBAL__N_119inpaint_fill_kernelILi3EEEv..` -> `inpaint_fill_kernel<3>`,
    `..srvgg_conv3x3_kernelILi64ELb0EE..` -> `srvgg_conv3x3_kernel<64,false>`."""
    stems = kernel_stems(source_path)
    out = set()
    for sym in elf_symbols(lib_path):
        stem = demangle_kernel(sym, stems)
        if stem is None:
            continue
        t = re.match(r"_Z(?:N12_GLOBAL__N_1)?\d+" + stem + r"I((?:L[ib]\d+E)+)E", sym)
        args = [int(v) if k == "i" else ("false", "true")[int(v)] for k, v in re.findall(r"L([ib])(\d+)E", t.group(1))] if t else []
        if stem == "ssim_tile_kernel":
            out.add(f"{stem}<{SRC_NAMES[args[0]]},{BORDER_NAMES[args[1]]}>")
        elif stem == "ssim_finish_kernel":
            out.add(f"{stem}<{BORDER_NAMES[args[0]]}>")
        else:
            out.add(f"{stem}<{','.join(map(str, args))}>" if args else stem)
    return out


# ============================================================================================ cases
@dataclass(frozen=True)
class Case:
    id: str
    op: str                                   # ssim | bbox | apply
    kernel: str                               # what elvis_last_launch reports after the call
    shape: Tuple[int, int, int, int]          # n, h, w, c (bbox: c = 1, the mask itself)
    source: str = "channels"                  # ssim: luma | channels
    border: str = "reflect"                   # ssim: reflect | valid
    pad: Optional[int] = 0                    # ssim: None = automatic (ELVIS_SSIM_PAD_AUTO)
    rects: Optional[Tuple[Tuple[int, int, int, int], ...]] = None     # ssim: (y0, y1, x0, x1) per frame
    mask: Optional[str] = None                # ssim: random | ring.  bbox: the recipe of the plane
    offs: Tuple[int, ...] = (0, 0, 0)         # byte offset from a 16-byte boundary: ssim a, b, mask; apply frame, mask, out; bbox mask
    window: str = "gaussian"                  # ssim: gaussian | msssim | asym
    scale: float = 1.0                        # ssim: 1 -> C1_255, C2_255; 255 -> 0.01^2, 0.03^2
    invert: bool = False                      # apply
    group: str = ""                           # which gap of the issue the case closes

    @property
    def kernels(self):
        return (self.kernel, f"ssim_finish_kernel<{self.border}>") if self.op == "ssim" else (self.kernel,)

    @property
    def constants(self):
        return (Q.C1_255, Q.C2_255) if self.scale == 1.0 else (0.01 ** 2, 0.03 ** 2)

    @property
    def seed(self):
        return zlib.crc32(self.id.encode())


def window(kind: str) -> np.ndarray:
    if kind == "gaussian":
        return Q.gaussian_taps()
    if kind == "msssim":
        return Q.msssim_taps()
    if kind == "asym":                        # multiples of 1 / 128, strictly increasing, sum exactly 1 in any order
        w = np.array([1, 2, 3, 5, 7, 9, 11, 14, 18, 24, 34], np.float64) / 128.0
        assert w.sum() == 1.0 and (np.diff(w) > 0).all() and w[0] > 0
        return w
    raise ValueError(kind)


def _ssim_cases(add):
    def ssim(id, shape, source="channels", border="reflect", **kw):
        if border == "valid" and "window" not in kw:
            kw["window"] = "msssim"
        if border == "valid" and source == "channels" and "scale" not in kw:
            kw["scale"] = 255.0
        add(Case(id, "ssim", f"ssim_tile_kernel<{source},{border}>", shape, source, border, **kw))

    for border in BORDER_NAMES:
        bpad = 5 if border == "reflect" else 0      # reflect, pad 5: the first tile's apron starts at column 0 and is staged wide
        # channels: c = 1..4 at width 53 (never staged before: 1, 2, 4); the row shift of the 4-byte words follows x0
        for c in (1, 2, 3, 4):
            ssim(f"c{c}_{border}", (2, 29, 53, c), border=border, pad=bpad, group="channels")
        for x0 in range(4):
            rects = ((1, 28, x0, x0 + 49), (0, 29, x0, 53))
            ssim(f"c4_x{x0}_{border}", (2, 29, 53, 4), border=border, pad=bpad, rects=rects, mask="random", group="channels")
            ssim(f"c1_x{x0}_{border}", (2, 29, 53, 1), border=border, pad=bpad, rects=rects, mask="random", group="channels")
            ssim(f"luma_x{x0}_{border}", (2, 29, 53, 3), "luma", border, pad=bpad, rects=rects, mask="random", group="channels")
        # reflect without pad goes wide from the second tile column on: 27 + 42 <= 100
        for c in (2, 3):
            ssim(f"wide_40x100_c{c}_{border}", (1, 40, 100, c), border=border, group="channels")
        # map sizes at the tile's boundaries, as a whole frame and as a rectangle strictly inside a larger one
        shrink = 0 if border == "reflect" else 10
        for mh in (TH - 1, TH, TH + 1):
            for mw in (TW - 1, TW, TW + 1):
                lh, lw = mh + shrink, mw + shrink
                ssim(f"tile_{mh}x{mw}_{border}", (1, lh, lw, 1), border=border, group="tiles")
                ssim(f"tile_{mh}x{mw}_{border}_inner", (1, lh + 7, lw + 9, 3), "luma", border, window="asym",
                     rects=((3, 3 + lh, 5, 5 + lw),), group="tiles")
        # frames and mask 1, 2, 3 bytes off a dword: aligned == 0, every tile staged per pixel
        for offs in ((1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 0, 1), (1, 0, 0), (0, 2, 0)):
            ssim(f"off{''.join(map(str, offs))}_{border}", (2, 29, 53, 3), border=border, pad=bpad, mask="random", offs=offs,
                 group="misaligned")
        ssim(f"off111_c1_{border}", (1, 29, 53, 1), border=border, pad=bpad, mask="ring", offs=(1, 1, 1), group="misaligned")
        ssim(f"off333_c4_{border}", (1, 29, 53, 4), border=border, pad=bpad, mask="ring", offs=(3, 3, 3), group="misaligned")
        ssim(f"off321_luma_{border}", (1, 29, 53, 3), "luma", border, pad=bpad, mask="random", offs=(3, 2, 1), group="misaligned")
        # rectangles: clipped by the frame, empty, inverted, wholly outside
        h, w = 40, 56
        for name, r in (("neg", (-3, 20, -2, 30)), ("past", (5, h + 4, 7, w + 9)), ("empty", (10, 10, 0, w)),
                        ("inverted", (12, 8, 0, w)), ("outside_y", (h + 10, h + 20, 0, w)), ("outside_x", (0, h, -9, 0))):
            ssim(f"rect_{name}_{border}", (1, h, w, 3), border=border, pad=2, rects=(r,), mask="ring", group="rects")
        # an explicit pad that eats the whole area (2 pad == the smaller side), and one that leaves a single row
        ssim(f"pad_eats_{border}", (1, 29, 53, 3), border=border, pad=4, rects=((3, 11, 4, 24),), group="rects")
        ssim(f"pad_leaves_1_{border}", (1, 29, 53, 3), border=border, pad=4, rects=((3, 12, 4, 24),), group="rects")
        ssim(f"pad_eats_cols_{border}", (1, 29, 53, 3), border=border, pad=3, rects=((3, 20, 4, 10),), group="rects")
        # a batch of three different rectangles and masks: each frame's value is what it gives alone
        for source in SRC_NAMES:
            ssim(f"batch_{source}_{border}", (3, 37, 53, 3), source, border, pad=bpad if source == "channels" else None,
                 rects=((0, 37, 0, 53), (3, 30, 2, 49), (11, 31, 5, 22)), mask="random", group="batch")
    # the tensor-end fallback: the last wide tile stages the last row up to the row's end, and the size is no multiple of 4
    ssim("tensor_end_c3", (1, 27, 42, 3), border="valid", group="tensor_end")
    ssim("tensor_end_c1", (1, 27, 42, 1), border="valid", group="tensor_end")
    ssim("tensor_end_c3_masked", (1, 27, 42, 3), "luma", "valid", mask="random", group="tensor_end")
    # VALID at the smoothing threshold with the asymmetric window: a swap of the row and column windows shows here
    for lh, lw in ((10, 40), (12, 40), (40, 9), (40, 10), (9, 70), (70, 9), (10, 10), (12, 12), (11, 40), (40, 11), (40, 12)):
        ssim(f"valid_{lh}x{lw}", (1, lh, lw, 2), border="valid", window="asym", group="threshold")
    ssim("valid_9x70_inner", (1, 15, 80, 3), "luma", "valid", window="asym", rects=((2, 11, 3, 73),), mask="random", group="threshold")
    # the automatic window rule on boxes whose smallest side is 2..8 (1.0 below 3), wide and tall
    for s in range(2, 9):
        ssim(f"auto_{s}_wide", (1, 29, 53, 3), "luma", pad=None, rects=((5, 5 + s, 7, 10 + s),), mask="random", group="auto")
        ssim(f"auto_{s}_tall", (1, 29, 53, 3), "luma", pad=None, rects=((5, 9 + s, 7, 7 + s),), group="auto")
    ssim("auto_4_channels_valid", (1, 29, 53, 2), border="valid", pad=None, rects=((5, 9, 7, 30),), group="auto")


BBOX_KINDS = ("first", "last", "byte7", "tail", "values", "empty_middle", "random", "empty")


def _bbox_cases(add):
    def bbox(id, shape, kind, off=0):
        add(Case(id, "bbox", "mask_bbox_kernel", shape + (1,), mask=kind, offs=(off,), group="bbox"))

    big = 1024 * BBOX_WORD + BBOX_WORD + 3            # every lane one word, one word more, a byte tail: 8203 = 13 * 631
    for plane, hw in ((1, (1, 1)), (7, (7, 1)), (8, (2, 4)), (9, (3, 3)), (big, (13, 631))):
        assert hw[0] * hw[1] == plane
        for kind in ("first", "last", "random"):
            bbox(f"bbox_{plane}_{kind}", (1,) + hw, kind)
    bbox("bbox_8203_tail", (1, 13, 631), "tail")
    bbox("bbox_8203_byte7", (1, 13, 631), "byte7")
    bbox("bbox_8203_empty", (1, 13, 631), "empty")
    # a 4 x 13 plane: word 1 holds bytes 8..15 and straddles rows 0 and 1; bytes 48..51 are the tail
    for kind in ("byte7", "tail", "values", "first", "last"):
        bbox(f"bbox_4x13_{kind}", (1, 4, 13), kind)
    # planes of 35 bytes: frame 0 is scanned by words, frames 1 and 2 start off a word and go byte by byte
    for kind in ("random", "values", "empty_middle", "last", "byte7"):
        bbox(f"bbox_n3_5x7_{kind}", (3, 5, 7), kind)
    bbox("bbox_n3_13x631_empty_middle", (3, 13, 631), "empty_middle")
    for off in range(1, 8):
        bbox(f"bbox_off{off}", (2, 6, 12), "values", off)


APPLY_PIXELS = {1: (1, 1), 15: (3, 5), 16: (4, 4), 17: (1, 17), APPLY_GROUP * APPLY_THREADS + 5: (3, 1367)}


def apply_launch(c: int, offs) -> str:
    """The dispatch rule of elvis_apply_mask_u8."""
    return f"apply_mask_u8_kernel<{c if c in (1, 3, 4) and not any(o % 16 for o in offs) else 0}>"


def _apply_cases(add):
    def apply(id, hw, c, offs, invert):
        add(Case(id, "apply", apply_launch(c, offs), (1,) + hw + (c,), offs=offs, invert=invert, mask="random", group="apply"))

    for c in (1, 2, 3, 4, 5):
        for px, hw in APPLY_PIXELS.items():
            assert hw[0] * hw[1] == px
            for offs in ((0, 0, 0), (1, 1, 1)):
                for invert in (False, True):
                    apply(f"apply_c{c}_p{px}_off{offs[0]}_{'inv' if invert else 'keep'}", hw, c, offs, invert)
    for offs in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (16, 32, 48), (0, 0, 8)):
        apply(f"apply_c3_p4101_offs{'_'.join(map(str, offs))}", APPLY_PIXELS[4101], 3, offs, False)
    add(Case("apply_n2_c4", "apply", apply_launch(4, (0, 0, 0)), (2, 33, 47, 4), invert=True, mask="random", group="apply"))


def _build():
    cases = []
    _ssim_cases(cases.append)
    _bbox_cases(cases.append)
    _apply_cases(cases.append)
    assert len({c.id for c in cases}) == len(cases)
    return tuple(cases)


CASES = _build()
BY_ID = {c.id: c for c in CASES}
OPS = ("ssim", "bbox", "apply")


def of(op):
    return [c for c in CASES if c.op == op]


# ============================================================================================ inputs
def _mask(kind, h, w, rng):
    if kind == "random":
        return (rng.random((h, w)) < 0.7).astype(np.uint8) * rng.choice(np.array([1, 2, 128, 255], np.uint8), (h, w))
    if kind == "ring":
        m = np.ones((h, w), np.uint8)
        m[3:h - 3, 3:w - 3] = 0
        m[h // 2, w // 2] = 7
        return m
    raise ValueError(kind)


def _bbox_plane(kind, n, h, w, rng):
    m = np.zeros((n, h * w), np.uint8)
    plane = h * w
    words = plane // BBOX_WORD
    for f in range(n):
        if kind == "first":
            m[f, 0] = 1
        elif kind == "last":
            m[f, plane - 1] = 128
        elif kind == "byte7":             # byte 7 of a word that straddles two rows (of frame 0's word grid)
            hit = [i for i in range(words) if (i * 8) // w != (i * 8 + 7) // w]
            m[f, hit[len(hit) // 2] * 8 + 7 if hit else plane - 1] = 2
        elif kind == "tail":
            m[f, min(plane - 1, words * 8 + (plane - words * 8) // 2)] = 255
        elif kind in ("values", "random", "empty_middle"):
            k = max(1, plane // 9)
            at = rng.choice(plane, k, replace=False)
            m[f, at] = rng.choice(np.array([1, 2, 128, 255], np.uint8), k) if kind != "random" else 1
            if kind == "empty_middle" and f == 1:
                m[f] = 0
    return m.reshape(n, h, w)


def inputs(case: Case):
    """ssim: (a, b, mask or None); bbox: (mask,); apply: (frames, mask).  Read-only uint8 arrays, the same for every call."""
    if case.id not in _INPUTS:
        rng = np.random.default_rng(case.seed)
        n, h, w, c = case.shape
        if case.op == "bbox":
            out = (_bbox_plane(case.mask, n, h, w, rng),)
        elif case.op == "apply":
            m = np.stack([_mask("random", h, w, rng) for _ in range(n)])
            if h * w > 1:                         # both kept and dropped pixels, whatever the draw
                m.reshape(n, -1)[:, 0], m.reshape(n, -1)[:, 1] = 255, 0
            out = (rng.integers(1, 256, (n, h, w, c), dtype=np.uint8), m)
        else:
            yy, xx = np.mgrid[:h, :w]
            base = np.stack([100 + 75 * np.sin(yy / 5.0 + k) * np.cos(xx / 7.0 - k) for k in range(c)], axis=-1)[None].repeat(n, 0)
            a = np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
            b = np.clip(a.astype(np.float64) + rng.normal(0, 9, a.shape), 0, 255).astype(np.uint8)
            m = None if case.mask is None else np.stack([_mask(case.mask, h, w, rng) for _ in range(n)])
            out = (a, b, m)
        for arr in out:
            if arr is not None:
                arr.setflags(write=False)
        _INPUTS[case.id] = out
    return _INPUTS[case.id]


_INPUTS = {}


# ============================================================================================ expected
def clipped_rect(case: Case, f: int):
    n, h, w, c = case.shape
    if case.rects is None:
        return 0, h, 0, w
    y0, y1, x0, x1 = case.rects[f]
    return max(0, y0), min(h, y1), max(0, x0), min(w, x1)


def _auto(lh, lw, mutant=None):
    """(pad, cov_norm) of the automatic rule, or None where the frame reports 1.0."""
    win = Q.win_size_for(lh, lw)
    if mutant == "win_4_as_5" and min(lh, lw) == 4:
        win = 5
    if win is None:
        return None
    return (win - 1) // 2, (1.0 if mutant == "cov_norm_1" else win * win / (win * win - 1.0))


def _axis(x, taps, off, m, axis, index):
    """The kernel's pass along one axis: m outputs, output i = sum_k taps[k] x[index(i + off + k)]."""
    x = np.moveaxis(x, axis, 0)
    n = x.shape[0]
    out = np.zeros((m,) + x.shape[1:], np.float64)
    for k in range(11):
        out += taps[k] * x[index(np.arange(m) + off + k, n)]
    return np.moveaxis(out, 0, axis)


def _model_mean(x, y, w, border, C1, C2, cov, pad, mutant=None):
    """Q.ssim_mean written the way the kernel indexes (a window, a tap offset and a map size per axis), so that one
    clause can be changed.  Without a mutant it equals Q.ssim_mean (the ledger asserts it)."""
    delta = np.zeros(11)
    delta[0] = 1.0
    index = (lambda p, n: np.clip(p, 0, n - 1)) if mutant == "edge_clamp" else Q.reflect_index
    if mutant == "window_reversed":
        w = w[::-1]
    spec = []
    for n in x.shape:
        if border == "reflect":
            spec.append((w, -5, n))
        elif n >= 11:
            spec.append((w, -5 if mutant == "valid_from_minus_5" else 0, n - 10))
        else:
            spec.append((delta, 0, n))
    (wy, oy, mh), (wx, ox, mw) = spec
    if mutant == "windows_swapped":
        wy, wx = wx, wy

    def filt(v):
        return _axis(_axis(v, wx, ox, mw, 1, index), wy, oy, mh, 0, index)
    S = Q._ssim_map(x, y, filt, C1, C2, cov)
    r0, r1, c0, c1 = pad, mh - pad, pad, mw - pad
    if r1 <= r0 or c1 <= c0:
        return 1.0
    count = (r1 - r0) * (c1 - c0)
    if mutant == "map_row_more":          # the guard one row late: needs a row below the map, that is pad >= 1
        r1 += 1
    if mutant == "map_row_less":
        r1 -= 1
    if mutant == "map_col_less":
        c1 -= 1
    assert r1 <= S.shape[0]
    return float(S[r0:r1, c0:c1].sum() / count)


def expected(case: Case, mutant: Optional[str] = None):
    """float64 numpy throughout, never the library.  ssim: [n, cout]; bbox: int32 [n, 4]; apply: uint8 [n, h, w, c]."""
    n, h, w, c = case.shape
    if case.op == "bbox":
        return np.array([Q.mask_bbox(m) for m in inputs(case)[0]], np.int32)
    if case.op == "apply":
        frames, mask = inputs(case)
        return np.stack([Q.apply_binary_mask(frames[f], mask[f], case.invert) for f in range(n)])
    a, b, m = inputs(case)
    win = window(case.window)
    C1, C2 = case.constants
    cout = 1 if case.source == "luma" else c
    out = np.ones((n, cout), np.float64)
    for f in range(n):
        y0, y1, x0, x1 = clipped_rect(case, f)
        if y1 <= y0 or x1 <= x0:
            continue
        if case.pad is None:
            rule = _auto(y1 - y0, x1 - x0, mutant)
            if rule is None:
                continue
            pad, cov = rule
        else:
            pad, cov = case.pad, 1.0
        ca, cb = a[f, y0:y1, x0:x1], b[f, y0:y1, x0:x1]
        if case.source == "luma":
            if mutant == "luma_rb":
                ca, cb = ca[..., ::-1], cb[..., ::-1]
            planes = [(Q.luma_bgr(ca).astype(np.float64), Q.luma_bgr(cb).astype(np.float64))]
        else:
            planes = [(ca[..., k].astype(np.float64) / case.scale, cb[..., k].astype(np.float64) / case.scale) for k in range(c)]
        keep = None
        if m is not None:
            mx0 = x0
            if mutant == "mask_at_frame_shift":      # the mask byte fetched at the frames' shift inside the 4-byte word
                mx0 = x0 + frame_shift(case, f) - mask_shift(case, f)
            cols = np.clip(np.arange(mx0, mx0 + (x1 - x0)), 0, w - 1)
            keep = m[f, y0:y1][:, cols] != 0
        for k, (x, y) in enumerate(planes):
            if keep is not None:
                x = np.where(keep, x, 0.0)
                y = y if mutant == "mask_one_input" else np.where(keep, y, 0.0)
            if mutant is None:
                out[f, k] = Q.ssim_mean(x, y, win, case.border, C1, C2, cov, pad)
            else:
                out[f, k] = _model_mean(x, y, win, case.border, C1, C2, cov, pad, mutant)
    return out


def frame_shift(case: Case, f: int) -> int:
    y0, _, x0, _ = clipped_rect(case, f)
    n, h, w, c = case.shape
    return (case.offs[0] + ((f * h + y0) * w + x0) * c) & 3


def mask_shift(case: Case, f: int) -> int:
    y0, _, x0, _ = clipped_rect(case, f)
    n, h, w, c = case.shape
    return (case.offs[2] + (f * h + y0) * w + x0) & 3


# mutant -> the small case on which it must differ from `expected` by >= 1e-6
MUTANTS = {
    "map_row_more": "pad_leaves_1_reflect",
    "map_row_less": "tile_17x33_reflect",
    "map_col_less": "tile_17x33_valid",
    "edge_clamp": "auto_4_wide",                 # a box narrower than 5: the reflection repeats
    "window_reversed": "tile_15x31_reflect_inner",
    "valid_from_minus_5": "valid_12x40",
    "windows_swapped": "valid_10x40",
    "mask_one_input": "c1_x1_reflect",
    "mask_at_frame_shift": "luma_x2_valid",
    "luma_rb": "luma_x2_reflect",
    "win_4_as_5": "auto_4_tall",
    "cov_norm_1": "auto_3_tall",
}


# ============================================================================================ the kernel's geometry
def area(case: Case, f: int):
    """ssim_area: dict(y0, x0, lh, lw, pad, mh, mw, degenerate) of frame f."""
    y0, y1, x0, x1 = clipped_rect(case, f)
    lh, lw = y1 - y0, x1 - x0
    deg = lh <= 0 or lw <= 0
    pad = case.pad
    if pad is None:
        rule = _auto(lh, lw)
        deg = deg or rule is None
        pad = 3 if rule is None else rule[0]
    sh = lh - 10 if case.border == "valid" and lh >= 11 else lh
    sw = lw - 10 if case.border == "valid" and lw >= 11 else lw
    mh, mw = sh - 2 * pad, sw - 2 * pad
    return dict(y0=y0, x0=x0, lh=lh, lw=lw, pad=pad, mh=mh, mw=mw, degenerate=deg or mh <= 0 or mw <= 0)


def aligned(case: Case) -> bool:
    used = case.offs[:2] + ((case.offs[2],) if case.mask is not None else ())
    return not any(o % 4 for o in used)


def staging(case: Case):
    """Every staged row of every wide tile, for the frames (`a`, bpp = c) and the mask (`m`, bpp = 1):
    (tensor, shift of the row in its first 4-byte word, whether the row's last word crosses the tensor's end).
    Also the number of tiles that take the per-pixel path.  From the case's numbers alone."""
    n, h, w, c = case.shape
    rows, narrow = [], 0
    toff = -5 if case.border == "reflect" else 0
    for f in range(n):
        g = area(case, f)
        if g["degenerate"]:
            continue
        for oy0 in range(0, g["mh"], TH):
            for ox0 in range(0, g["mw"], TW):
                iy0, ix0 = g["pad"] + oy0 + toff, g["pad"] + ox0 + toff
                if not (aligned(case) and ix0 >= 0 and ix0 + COLS <= g["lw"]):
                    narrow += 1
                    continue
                for r in range(ROWS):
                    gy = g["y0"] + int(Q.reflect_index(iy0 + r, g["lh"]))
                    for name, bpp, off in (("a", c, case.offs[0]),) + ((("m", 1, case.offs[2]),) if case.mask else ()):
                        p = off + ((f * h + gy) * w + g["x0"] + ix0) * bpp          # relative to a 16-byte boundary
                        sh = p & 3
                        last = p - sh + ((sh + COLS * bpp - 1) // 4) * 4           # the last word that holds a staged byte
                        rows.append((name, sh, last + 4 > off + n * h * w * bpp))
    return rows, narrow
