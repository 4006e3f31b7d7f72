"""Restart intervals of the device JPEG writer (elvis_amd/jpeg_write.py `restart_rows=` / `restart_mcus=`,
csrc/jpeg_write.hip, csrc/jpeg_encode.h) stated on top of tests/_jpeg_write_ref.py, whose block coder codes an interval
as it codes a frame.  Importable without a GPU.

The rule (libjpeg jchuff.c `encode_mcu_huff` / `emit_restart`, jcmarker.c `write_scan_header`, jcmaster.c): with an
interval of Ri > 0 MCUs and M MCUs in the scan, interval s holds MCUs [s * Ri, min((s + 1) * Ri, M)); every interval
starts with the DC predictor of every component at 0 and ends with 1 bits to the byte boundary, a byte that is stuffed
like any other; in front of every interval s >= 1 stands FF D0+((s - 1) & 7), not stuffed, and nothing but EOI stands
behind the last; Ri >= M gives no marker at all.  The header gets FF DD 00 04 <Ri> behind the last DHT, in front of SOS.
`restart_rows=r` is libjpeg's `restart_in_rows`: Ri = min(r * MCUs per row, 65535); `restart_mcus=k` is
`restart_interval = k`.  A dummy block still repeats the DC of the block before it in its own MCU.  Against a
libjpeg-turbo PIL with `restart_marker_rows=` / `restart_marker_blocks=` and `optimize=False` the DRI segment's place and
content and everything from SOS to EOI are equal byte for byte (tests/test_jpeg_restart_host.py).  `mutant=` switches on
one named deviation.

    python tests/_jpeg_restart_ref.py dump FILE      writes every case of the corpus for tools/jpeg_restart_check.cpp
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
import _jpeg_write_ref as W

MUTANTS = ("predictor_not_reset", "marker_index_not_wrapped", "marker_after_last", "pad_zero", "pad_ff_not_stuffed", "marker_stuffed",
           "rows_not_capped")
WIDTHS = (1, 8, 9, 17, 33, 53)
HEIGHTS = (1, 8, 16, 17, 37)
QUALITIES = (30, 75, 95, 100)
CONTENTS = ("flat200", "noise", "ramp", "white", "checker255")
# (restart_rows, restart_mcus); restart_mcus -1 stands for the frame's MCU count plus 3: an interval that holds the whole scan
SETTINGS = ((1, 0), (2, 0), (0, 1), (0, 2), (0, 3), (0, 5), (0, 7), (0, -1))


def mcu_grid(w: int, h: int, channels: int, subsampling: str) -> Tuple[int, int, int]:
    """(MCUs per row, MCU rows, blocks per MCU)."""
    hmax, vmax = W._FACTORS[subsampling] if channels == 3 else (1, 1)
    return -(-w // (8 * hmax)), -(-h // (8 * vmax)), (hmax * vmax + 2 if channels == 3 else 1)


def restart_interval(w: int, h: int, channels: int, subsampling: str, restart_rows: int = 0, restart_mcus: int = 0,
                     mutant: Optional[str] = None) -> int:
    """The interval in MCUs, 0 for none (jcmaster.c: restart_in_rows wins where it is set, capped at 65535)."""
    if restart_rows:
        nominal = restart_rows * mcu_grid(w, h, channels, subsampling)[0]
        return nominal if mutant == "rows_not_capped" else min(nominal, 65535)
    return restart_mcus


def _bits_of(raw: bytes, count: int) -> str:
    return format(int.from_bytes(raw, "big"), f"0{8 * len(raw)}b")[:count] if raw else ""


def _interval(blocks, comp, lo: int, hi: int, bpm: int, mutant: Optional[str]) -> Tuple[bytes, bytes]:
    """(the stuffed bytes, the bytes before stuffing) of blocks [lo, hi) coded as an interval of their own."""
    inner = "final_fill_zero" if mutant == "pad_zero" else None
    if mutant == "predictor_not_reset" and lo > 0:
        # the MCU in front sets every predictor: code it too, then cut its bits off the front
        lengths: List[int] = []
        _, raw, _, _ = W.entropy(blocks[lo - bpm:hi], comp[lo - bpm:hi], None, lengths)
        s = _bits_of(raw, sum(lengths))[sum(lengths[:bpm]):]
        s += "1" * (-len(s) % 8)
        raw = int(s, 2).to_bytes(len(s) // 8, "big") if s else b""
        return raw.replace(b"\xff", b"\xff\x00"), raw
    scan, raw, _, _ = W.entropy(blocks[lo:hi], comp[lo:hi], inner)
    if mutant == "pad_ff_not_stuffed" and raw.endswith(b"\xff"):
        scan = scan[:-1]
    return scan, raw


@dataclass
class Encoded:
    data: bytes                       # the whole file
    scan: bytes                       # everything between SOS and EOI: the intervals, stuffed and filled, and the markers
    ri: int                           # the interval in MCUs
    mcus: int                         # MCUs of the scan
    bpm: int
    intervals: List[Tuple[bytes, bytes]]    # per interval (stuffed bytes, bytes before stuffing), markers not included
    blocks: np.ndarray                # int16 [blocks, 64] as the statement without an interval has them
    dummy: np.ndarray
    comp: np.ndarray


def header(width: int, height: int, channels: int, subsampling: str, tables, ri: int) -> bytes:
    """The header of the statement without an interval, with DRI in front of SOS (jcmarker.c write_scan_header: the DHT
    segments, then DRI, then SOS)."""
    head = W.header(width, height, channels, subsampling, tables)
    if not ri:
        return head
    sos = 2 + 2 + 1 + 2 * channels + 3
    assert head[-sos:-sos + 2] == b"\xff\xda"
    return head[:-sos] + b"\xff\xdd\x00\x04" + struct.pack(">H", ri) + head[-sos:]


def encode(frame: np.ndarray, quality: int = 95, subsampling: str = "420", order: str = "rgb", restart_rows: int = 0, restart_mcus: int = 0,
           mutant: Optional[str] = None) -> Encoded:
    """One uint8 frame (H,W), (H,W,1) or (H,W,3) as a baseline JPEG file with restart intervals."""
    a = np.asarray(frame)
    channels = 1 if a.ndim == 2 else a.shape[2]
    h, w = a.shape[:2]
    blocks, dummy, comp, tables = W.quantised_blocks(a, quality, subsampling, order)
    mcux, mcuy, bpm = mcu_grid(w, h, channels, subsampling)
    mcus = mcux * mcuy
    assert len(blocks) == mcus * bpm
    ri = restart_interval(w, h, channels, subsampling, restart_rows, restart_mcus, mutant)
    step = ri if ri else mcus
    intervals = [_interval(blocks, comp, m * bpm, min(m + step, mcus) * bpm, bpm, mutant) for m in range(0, mcus, step)]
    scan = bytearray()
    for s, (stuffed, _) in enumerate(intervals):
        if s:
            index = s - 1 if mutant == "marker_index_not_wrapped" else (s - 1) & 7
            scan += b"\xff\x00" if mutant == "marker_stuffed" else b"\xff"
            scan.append(0xD0 + index)
        scan += stuffed
    if mutant == "marker_after_last" and ri:
        scan += bytes([0xFF, 0xD0 + ((len(intervals) - 1) & 7)])
    data = header(w, h, channels, subsampling, tables, ri) + bytes(scan) + b"\xff\xd9"
    return Encoded(data, bytes(scan), ri, mcus, bpm, intervals, blocks.astype(np.int16), dummy, comp)


def entropy_part(data: bytes) -> Tuple[List[int], bytes]:
    """(the markers of a file's segments in front of the entropy-coded bytes, in their order; everything behind SOS)."""
    at, seen = 2, []
    while True:
        assert data[at] == 0xFF
        m = data[at + 1]
        (ln,) = struct.unpack(">H", data[at + 2:at + 4])
        seen.append(m)
        at += 2 + ln
        if m == 0xDA:
            return seen, data[at:]


def markers(scan: bytes) -> List[int]:
    """The RSTm markers of the entropy-coded bytes in their order (an FF that no 00 follows)."""
    return [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]


# ----------------------------------------------------------------------------- the corpus
@dataclass(frozen=True)
class Case:
    name: str
    w: int
    h: int
    sampling: str              # "gray" | "444" | "422" | "420"
    quality: int
    kind: str
    seed: int
    restart_rows: int
    restart_mcus: int

    @property
    def channels(self) -> int:
        return 1 if self.sampling == "gray" else 3

    @property
    def subsampling(self) -> str:
        return "420" if self.sampling == "gray" else self.sampling

    def frame(self) -> np.ndarray:
        """uint8 [h, w, channels], RGB."""
        if self.kind in ("flat200", "flat128"):
            return np.full((self.h, self.w, self.channels), int(self.kind[4:]), np.uint8)
        return W.make_frame(self.kind, self.h, self.w, self.channels, self.seed)

    @property
    def restart(self) -> dict:
        return {"restart_rows": self.restart_rows} if self.restart_rows else {"restart_mcus": self.restart_mcus}

    @property
    def pil_restart(self) -> dict:
        return {"restart_marker_rows": self.restart_rows} if self.restart_rows else {"restart_marker_blocks": self.restart_mcus}


@lru_cache(maxsize=None)
def cases() -> Tuple[Case, ...]:
    """Every size x sampling with the setting, the quality and the content cycling; every setting x sampling at 53x37, at
    17x17 (odd block counts: dummy blocks on both edges in 4:2:0) and at 33x16 with the content cycling on; 128x128 gray,
    whose 256 blocks are one step of the prefix sum, with every setting and with intervals of 255, 256 and 257 blocks; a
    mid-gray frame, whose intervals of one MCU are one byte long."""
    out, k = [], 0

    def add(w, h, s, setting):
        nonlocal k
        rows, mcus = setting
        if mcus < 0:
            mx, my, _ = mcu_grid(w, h, 1 if s == "gray" else 3, "420" if s == "gray" else s)
            mcus = mx * my + 3
        q, kind = QUALITIES[(k + k // 4) % 4], CONTENTS[k % 5]
        name = f"w{w}-h{h}-{s}-q{q}-{kind}-" + (f"rows{rows}" if rows else f"mcus{mcus}")
        if not any(c.name == name for c in out):
            out.append(Case(name, w, h, s, q, kind, 700 + k, rows, mcus))
        k += 1

    for w in WIDTHS:
        for h in HEIGHTS:
            for s in R.SAMPLINGS:
                add(w, h, s, SETTINGS[k % len(SETTINGS)])
    for w, h in ((53, 37), (17, 17), (33, 16)):
        for s in R.SAMPLINGS:
            for setting in SETTINGS:
                add(w, h, s, setting)
            k += 1
    for setting in SETTINGS + ((0, 255), (0, 256), (0, 257)):
        add(128, 128, "gray", setting)
    # mid-gray: DC 0 and no AC, 6 bits a block, so that an interval of one MCU is one byte
    out.append(Case("w33-h16-gray-q75-flat128-mcus1", 33, 16, "gray", 75, "flat128", 0, 0, 1))
    out.append(Case("w33-h16-gray-q75-flat128-mcus3", 33, 16, "gray", 75, "flat128", 0, 0, 3))
    return tuple(out)


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


@lru_cache(maxsize=None)
def encoded(name: str, order: str = "rgb") -> Encoded:
    """The statement's file for a case by name, computed once."""
    c = case(name)
    frame = c.frame()
    return encode(frame[:, :, ::-1] if order == "bgr" and c.channels == 3 else frame, c.quality, c.subsampling, order, **c.restart)


@lru_cache(maxsize=None)
def plain(name: str) -> bytes:
    """The same case written without an interval."""
    c = case(name)
    return W.encode(c.frame(), c.quality, c.subsampling).data


def pil_encode(c: Case) -> bytes:
    """PIL's file of the case with `optimize=False` and its restart setting."""
    import io
    from PIL import Image
    a = c.frame()
    img = Image.fromarray(a[:, :, 0] if c.channels == 1 else a)
    buf = io.BytesIO()
    kw = {} if c.channels == 1 else {"subsampling": R._PIL_SUB[c.subsampling]}
    img.save(buf, "JPEG", quality=c.quality, optimize=False, **kw, **c.pil_restart)
    return buf.getvalue()


# ----------------------------------------------------------------------------- the corpus for the host check
def dump(path: str) -> None:
    """Every case as tools/jpeg_restart_check.cpp reads it: the shape and the settings with the interval in MCUs, the
    pixels (the channel orders alternate), the kernels' code table, and what the statement says of them - the quantised
    blocks and everything between SOS and the end of the file."""
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
            fh.write(struct.pack("<7I", c.h, c.w, c.channels, int(order == "bgr"), c.quality, W.SUBSAMPLINGS.index(c.subsampling), e.ri))
            for blob in (pixels.tobytes(), table, e.blocks.astype("<i2").tobytes(), e.scan + b"\xff\xd9"):
                fh.write(struct.pack("<I", len(blob)) + blob)
    print(f"{len(cases())} cases -> {path}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(__doc__)
