"""The device JPEG writer's contract (elvis_amd/jpeg_write.py, csrc/jpeg_write.hip, csrc/jpeg_encode.h)
stated in numpy and Python ints: libjpeg's forward path.  Importable without a GPU.

The statement: jccolor.c's 16-bit fixed-point RGB -> YCbCr; the edge replication and the h2v1 / h2v2 downsampling of
jcprepct.c and jcsample.c in their order (columns widened, the odd bottom row of 4:2:0 repeated, the downsample, then the
rows lengthened); jfdctint.c on samples less 128; the quantiser with the tables of `jpeg_set_quality(q, TRUE)`; the dummy
blocks of jccoefct.c; the Huffman coding of jchuff.c with the Annex K tables in one interleaved scan; the headers.
Against a libjpeg-turbo PIL at the same quality and sampling with `optimize=False`, the DQT tables, the SOF0 and SOS
contents and the entropy-coded segment are equal byte for byte (tests/test_jpeg_write_host.py); equality of whole files is
not claimed (the JFIF header's density fields are PIL's own).  `mutant=` switches on one named deviation.

    python tests/_jpeg_write_ref.py dump FILE      writes every case of the corpus for tools/jpeg_encode_check.cpp
"""
from __future__ import annotations

import struct
import sys
from dataclasses import dataclass
from functools import lru_cache
from typing import List, Optional, Tuple

import numpy as np

if __name__ == "__main__":          # run as a script: the package lies beside tests/
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import _jpeg_ref as R

MUTANTS = ("h2v2_bias_swapped", "bottom_rows_before_downsample", "dummy_dc_zero", "quantise_round_down",
           "dc_prediction_shared", "stuffing_off", "final_fill_zero")
SUBSAMPLINGS = ("444", "422", "420")
_FACTORS = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}
# Annex K.1 / K.2 in natural order: what PIL writes at quality 50, where the scaling is the identity
_BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
              80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72,
              92, 95, 98, 112, 100, 103, 99)
_BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99) + (99,) * 36


def quant_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
    """jpeg_set_quality(quality, force_baseline=TRUE): (luma, chroma), int64 [64] in natural order."""
    q = min(100, max(1, int(quality)))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.asarray(base, np.int64) * scale + 50) // 100, 1, 255) for base in (_BASE_LUMA, _BASE_CHROMA))


def _fix(x: float) -> int:
    return int(x * 65536 + 0.5)


def ycc(rgb: np.ndarray) -> List[np.ndarray]:
    r, g, b = (rgb[:, :, k].astype(np.int64) for k in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.168735892) * r - _fix(.331264108) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.418687589) * g - _fix(.081312411) * b + (128 << 16) + 32767) >> 16
    return [y, cb, cr]


def _widen(p: np.ndarray, cols: int) -> np.ndarray:
    return p if p.shape[1] >= cols else np.concatenate([p, np.repeat(p[:, -1:], cols - p.shape[1], axis=1)], axis=1)


def _lengthen(p: np.ndarray, rows: int) -> np.ndarray:
    return p if p.shape[0] >= rows else np.concatenate([p, np.repeat(p[-1:], rows - p.shape[0], axis=0)], axis=0)


def component_plane(p: np.ndarray, hf: int, vf: int, wib: int, hib: int, mutant: Optional[str] = None) -> np.ndarray:
    """A full-resolution plane to the component's hib * 8 x wib * 8 samples; hf, vf: the downsampling factors."""
    p = _widen(p.astype(np.int64), wib * 8 * hf)
    if vf == 2:
        p = _lengthen(p, hib * 16) if mutant == "bottom_rows_before_downsample" else _lengthen(p, p.shape[0] + (p.shape[0] & 1))
    if (hf, vf) == (2, 2):
        bias = np.tile([2, 1] if mutant == "h2v2_bias_swapped" else [1, 2], p.shape[1] // 4 + 1)[:p.shape[1] // 2]
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias[None, :]) >> 2
    elif (hf, vf) == (2, 1):
        bias = np.tile([0, 1], p.shape[1] // 4 + 1)[:p.shape[1] // 2]
        p = (p[:, 0::2] + p[:, 1::2] + bias[None, :]) >> 1
    return _lengthen(p, hib * 8)[:hib * 8, :wib * 8]


def _fdct_pass(v: np.ndarray, first: bool) -> np.ndarray:
    """One 8-point pass of jfdctint.c over the last axis (CONST_BITS 13, PASS1_BITS 2); descales round half up."""
    d = [v[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    s = 11 if first else 15

    def descale(x, n):
        return (x + (1 << (n - 1))) >> n

    o = [None] * 8
    o[0], o[4] = ((t10 + t11) << 2, (t10 - t11) << 2) if first else (descale(t10 + t11, 2), descale(t10 - t11, 2))
    z1 = (t12 + t13) * 4433
    o[2], o[6] = descale(z1 + t13 * 6270, s), descale(z1 - t12 * 15137, s)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = descale(t4 + z1 + z3, s), descale(t5 + z2 + z4, s), descale(t6 + z2 + z3, s), descale(t7 + z1 + z4, s)
    return np.stack(o, axis=-1)


def fdct_blocks(samples: np.ndarray) -> np.ndarray:
    """int [n, 8, 8] samples -> int64 [n, 8, 8] coefficients scaled by 8: rows first, then columns."""
    x = _fdct_pass(samples.astype(np.int64) - 128, True)
    return _fdct_pass(x.transpose(0, 2, 1), False).transpose(0, 2, 1)


def quantise(coef: np.ndarray, table: np.ndarray, mutant: Optional[str] = None) -> np.ndarray:
    q8 = table.reshape(8, 8).astype(np.int64) << 3
    half = 0 if mutant == "quantise_round_down" else q8 >> 1
    return np.sign(coef) * ((np.abs(coef) + half) // q8)


@dataclass
class Encoded:
    data: bytes                 # the whole file
    scan: bytes                 # the entropy-coded segment, stuffed and filled, without EOI
    blocks: np.ndarray          # int16 [blocks, 64], zigzag, MCU scan order, dummy blocks filled in
    dummy: np.ndarray           # bool [blocks]
    qt: Tuple[np.ndarray, ...]  # the tables in use, natural order
    unstuffed: bytes            # the scan before FF 00, final fill included
    zrl: int                    # ZRL symbols in the scan
    last63: int                 # blocks whose coefficient 63 is not zero
    block_bits: np.ndarray = None   # int64 [blocks]: the bits every block adds to the scan, before the final fill


def _planes(frame: np.ndarray, order: str) -> List[np.ndarray]:
    a = np.asarray(frame)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.shape[2] == 1:
        return [a[:, :, 0].astype(np.int64)]
    return ycc(a[:, :, ::-1] if order == "bgr" else a)


def quantised_blocks(frame: np.ndarray, quality: int, subsampling: str, order: str = "rgb", mutant: Optional[str] = None):
    """(blocks int64 [blocks, 64] in zigzag and MCU scan order, dummy flags, component of every block, the tables)."""
    planes = _planes(frame, order)
    h, w = planes[0].shape
    tables = quant_tables(quality)
    if len(planes) == 1:
        wib, hib = -(-w // 8), -(-h // 8)
        p = component_plane(planes[0], 1, 1, wib, hib)
        blk = p.reshape(hib, 8, wib, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        q = quantise(fdct_blocks(blk), tables[0], mutant).reshape(-1, 64)[:, list(R.ZIGZAG)]
        return q, np.zeros(len(q), bool), np.zeros(len(q), np.int64), tables[:1]
    hmax, vmax = _FACTORS[subsampling]
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    grids = []
    for c, p in enumerate(planes):
        hs, vs = (hmax, vmax) if c == 0 else (1, 1)
        cw, ch = -(-w * hs // hmax), -(-h * vs // vmax)
        wib, hib = -(-cw // 8), -(-ch // 8)
        plane = component_plane(p, hmax // hs, vmax // vs, wib, hib, mutant)
        blk = plane.reshape(hib, 8, wib, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        q = quantise(fdct_blocks(blk), tables[min(c, 1)], mutant).reshape(hib, wib, 64)[:, :, list(R.ZIGZAG)]
        grids.append((q, hs, vs, wib, hib))
    out, dummy, comp = [], [], []
    for my in range(mcuy):
        for mx in range(mcux):
            for c, (q, hs, vs, wib, hib) in enumerate(grids):
                for vy in range(vs):
                    for hx in range(hs):
                        by, bx = my * vs + vy, mx * hs + hx
                        if by < hib and bx < wib:
                            out.append(q[by, bx])
                            dummy.append(False)
                        else:
                            z = np.zeros(64, np.int64)
                            if mutant != "dummy_dc_zero":
                                z[0] = out[-1][0]          # the block before it in the MCU's own order
                            out.append(z)
                            dummy.append(True)
                        comp.append(c)
    return np.asarray(out), np.asarray(dummy), np.asarray(comp), tables


def _magnitude(v: int) -> Tuple[int, int]:
    t = abs(v).bit_length()
    return t, (v if v >= 0 else v + (1 << t) - 1)


@lru_cache(maxsize=None)
def _codes():
    """(code as a bit string by symbol) for DC 0, DC 1, AC 0, AC 1 of Annex K."""
    _, dc, ac = R.std_tables()
    inv = lambda tab: {s: k for k, s in R.code_strings(*tab).items()}
    return [inv(dc[0]), inv(dc[1])], [inv(ac[0]), inv(ac[1])]


def entropy(blocks: np.ndarray, comp: np.ndarray, mutant: Optional[str] = None, block_bits: Optional[List[int]] = None):
    """(the stuffed and filled scan, the same before stuffing, ZRL count, blocks with a non-zero coefficient 63).
    `block_bits`, when given, receives the number of bits of every block."""
    dcs, acs = _codes()
    bits: List[str] = []
    pred = [0, 0, 0]
    zrl = last63 = 0
    for blk, c in zip(blocks.tolist(), comp.tolist()):
        before = len(bits)
        t = min(c, 1)
        k = 0 if mutant == "dc_prediction_shared" else c
        cat, extra = _magnitude(blk[0] - pred[k])
        pred[k] = blk[0]
        bits.append(dcs[t][cat])
        if cat:
            bits.append(format(extra, f"0{cat}b"))
        run = 0
        for v in blk[1:]:
            if v == 0:
                run += 1
                continue
            while run > 15:
                bits.append(acs[t][0xF0])
                zrl += 1
                run -= 16
            cat, extra = _magnitude(v)
            bits.append(acs[t][run << 4 | cat] + format(extra, f"0{cat}b"))
            run = 0
        if run:
            bits.append(acs[t][0x00])
        last63 += blk[63] != 0
        if block_bits is not None:
            block_bits.append(sum(map(len, bits[before:])))
    s = "".join(bits)
    s += ("0" if mutant == "final_fill_zero" else "1") * (-len(s) % 8)
    raw = int(s, 2).to_bytes(len(s) // 8, "big") if s else b""
    return (raw if mutant == "stuffing_off" else raw.replace(b"\xff", b"\xff\x00")), raw, zrl, last63


def header(width: int, height: int, channels: int, subsampling: str, tables) -> bytes:
    """SOI, JFIF APP0, one DQT per table, SOF0, the DHT segments (DC 0, AC 0, then DC 1, AC 1 for colour), SOS."""
    _, dc, ac = R.std_tables()
    hmax, vmax = _FACTORS[subsampling] if channels == 3 else (1, 1)
    comps = [(1, hmax, vmax, 0)] + ([(2, 1, 1, 1), (3, 1, 1, 1)] if channels == 3 else [])
    out = bytearray(b"\xff\xd8") + R.JFIF
    for t, table in enumerate(tables):
        out += R.dqt(t, table)
    out += R._segment(0xC0, bytes([8]) + struct.pack(">HH", height, width) + bytes([len(comps)])
                      + b"".join(bytes([cid, h << 4 | v, tq]) for cid, h, v, tq in comps))
    for t in range(len(tables)):
        out += R.dht(0, t, *dc[t]) + R.dht(1, t, *ac[t])
    out += R._segment(0xDA, bytes([len(comps)]) + b"".join(bytes([c[0], min(i, 1) * 0x11]) for i, c in enumerate(comps)) + bytes([0, 63, 0]))
    return bytes(out)


def encode(frame: np.ndarray, quality: int = 95, subsampling: str = "420", order: str = "rgb", mutant: Optional[str] = None) -> Encoded:
    """One uint8 frame (H,W), (H,W,1) or (H,W,3) as a baseline JPEG file."""
    a = np.asarray(frame)
    channels = 1 if a.ndim == 2 else a.shape[2]
    blocks, dummy, comp, tables = quantised_blocks(a, quality, subsampling, order, mutant)
    lengths: List[int] = []
    scan, raw, zrl, last63 = entropy(blocks, comp, mutant, lengths)
    data = header(a.shape[1], a.shape[0], channels, subsampling, tables) + scan + b"\xff\xd9"
    return Encoded(data, scan, blocks.astype(np.int16), dummy, tables, raw, zrl, last63, np.asarray(lengths, np.int64))


# ----------------------------------------------------------------------------- the corpus
EXTRA_SIZES = ((8, 24), (24, 8), (7, 72), (40, 8))          # (w, h)
EXTREMES = ("white", "checker255")                          # at quality 100: the largest magnitude categories


def make_frame(kind: str, h: int, w: int, c: int, seed: int) -> np.ndarray:
    if kind == "white":
        return np.full((h, w, c), 255, np.uint8)
    if kind == "checker255":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], c, axis=2)
    return R.make_content(kind, h, w, c, seed)


@dataclass(frozen=True)
class Case:
    name: str
    w: int
    h: int
    sampling: str              # "gray" | "444" | "422" | "420"
    quality: int
    kind: str
    seed: int

    @property
    def channels(self) -> int:
        return 1 if self.sampling == "gray" else 3

    def frame(self) -> np.ndarray:
        """uint8 [h, w, channels], RGB."""
        return make_frame(self.kind, self.h, self.w, self.channels, self.seed)

    @property
    def subsampling(self) -> str:
        return "420" if self.sampling == "gray" else self.sampling


@lru_cache(maxsize=None)
def cases() -> Tuple[Case, ...]:
    """Every size with the other axes cycling, every sampling x quality x content at the odd size and at the sizes whose
    padding order matters, and the two extremes at quality 100 for every sampling."""
    out, k = [], 0

    def add(w, h, s, q, kind):
        nonlocal k
        out.append(Case(f"w{w}-h{h}-{s}-q{q}-{kind}", w, h, s, q, kind, 300 + k))
        k += 1

    sizes = [(w, h) for w in R.WIDTHS for h in R.HEIGHTS] + list(EXTRA_SIZES)
    for w, h in sizes:
        for _ in range(4):
            i = k
            add(w, h, R.SAMPLINGS[i % 4], R.QUALITIES[(i // 4 + i) % 4], R.CONTENTS[(i // 3) % 4])
    for w, h in ((53, 37),) + EXTRA_SIZES:
        for s in R.SAMPLINGS:
            for q in R.QUALITIES:
                for kind in R.CONTENTS:
                    if not any(c.name == f"w{w}-h{h}-{s}-q{q}-{kind}" for c in out):
                        add(w, h, s, q, kind)
    for s in R.SAMPLINGS:
        for kind in EXTREMES:
            add(33, 17, s, 100, kind)
            add(16, 16, s, 100, kind)
    return tuple(out)


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


@lru_cache(maxsize=None)
def encoded(name: str, order: str = "rgb") -> Encoded:
    """The statement's file for a case by name, computed once."""
    c = case(name)
    frame = c.frame()
    return encode(frame[:, :, ::-1] if order == "bgr" and c.channels == 3 else frame, c.quality, c.subsampling, order)


def pil_encode(frame: np.ndarray, quality: int, subsampling: str) -> bytes:
    """PIL's file of an RGB or gray frame with `optimize=False`."""
    import io
    from PIL import Image
    a = np.asarray(frame)
    gray = a.ndim == 2 or a.shape[2] == 1
    img = Image.fromarray(a.reshape(a.shape[0], a.shape[1]) if gray else a)
    buf = io.BytesIO()
    kw = {} if gray else {"subsampling": R._PIL_SUB[subsampling]}
    img.save(buf, "JPEG", quality=quality, optimize=False, **kw)
    return buf.getvalue()


# ----------------------------------------------------------------------------- the corpus for the host check
def dump(path: str) -> None:
    """Every case as tools/jpeg_encode_check.cpp reads it: the shape and the settings, the pixels (the channel orders
    alternate), the kernels' code table, and what the statement says of them - the quantised blocks and the scan with
    EOI."""
    from elvis_amd import jpeg_write
    table = jpeg_write.encode_tables().tobytes()
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases())))
        for k, c in enumerate(cases()):
            order = "bgr" if k % 2 and c.channels == 3 else "rgb"
            frame = c.frame()
            pixels = np.ascontiguousarray(frame[:, :, ::-1] if order == "bgr" else frame)
            e = encoded(c.name, order)
            fh.write(struct.pack("<I", len(c.name)) + c.name.encode())
            fh.write(struct.pack("<6I", c.h, c.w, c.channels, int(order == "bgr"), c.quality, SUBSAMPLINGS.index(c.subsampling)))
            for blob in (pixels.tobytes(), table, e.blocks.astype("<i2").tobytes(), e.scan + b"\xff\xd9"):
                fh.write(struct.pack("<I", len(blob)) + blob)
    print(f"{len(cases())} cases -> {path}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(__doc__)
