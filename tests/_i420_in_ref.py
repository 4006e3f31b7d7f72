"""numpy restatement of the decoder hand-off (elvis_amd/handoff.py, csrc/i420_in.hip) - what the device output and the Y4M
parser are pinned against, bit for bit.  Written from the contract, not from the code under test; no model, no cv2.

  * `i420_to_rgb`: cv2.cvtColor(planes, COLOR_YUV2RGB_I420 / COLOR_YUV2BGR_I420), restated from OpenCV 4.x
    YUV420p2RGB8Invoker in int64: with u = U[y/2, x/2] - 128, v = V[y/2, x/2] - 128, yy = max(0, Y[y, x] - 16) * 1220542,
        R = sat8((yy + (1 << 19) + 1673527 v) >> 20)
        G = sat8((yy + (1 << 19) - 852492 v - 409993 u) >> 20)
        B = sat8((yy + (1 << 19) + 2116026 u) >> 20)
    `>>` floors, sat8 clamps to [0, 255], chroma is replicated over its 2x2 quad.
  * `MUTANTS`: five statements that each change one clause; tests/test_i420_in_host.py shows the exhaustive frame tells
    four of them from the statement by their bytes.  The fifth, truncation toward zero in place of the floor shift,
    differs from the statement only where a sum is negative, by one, and sat8 sends both results to 0: it changes the
    value before sat8 and can change no byte, which the same test shows both ways.
  * `every_yuv_frame`: one 4096 x 4096 frame holding all 2^24 (Y, U, V) triples.
  * `y4m_walk`: a small statement of the Y4M container walk over bytes in memory.
"""
from __future__ import annotations

import numpy as np

SHIFT = 20
CY, CRV, CGV, CGU, CBU = 1220542, 1673527, -852492, -409993, 2116026


def _planes(planes: np.ndarray):
    """[n, H*3//2, W] u8 -> Y [n,H,W], U [n,H/2,W/2], V [n,H/2,W/2] as int64."""
    assert planes.ndim == 3 and planes.dtype == np.uint8 and planes.shape[1] % 3 == 0 and planes.shape[2] % 2 == 0
    n, rows, w = planes.shape
    h = rows // 3 * 2
    flat = planes.reshape(n, -1).astype(np.int64)
    y = flat[:, :h * w].reshape(n, h, w)
    u = flat[:, h * w:h * w + h * w // 4].reshape(n, h // 2, w // 2)
    v = flat[:, h * w + h * w // 4:].reshape(n, h // 2, w // 2)
    return y, u, v


def _floor_shift(x: np.ndarray) -> np.ndarray:
    return x >> SHIFT                                   # int64 >> floors


def _trunc_shift(x: np.ndarray) -> np.ndarray:
    return np.sign(x) * (np.abs(x) >> SHIFT)            # toward zero


def rgb_of(y, u, v, *, clamp_luma=True, rounding=1 << (SHIFT - 1), shift=_floor_shift, saturate=True):
    """(R, G, B) as int64 of the (Y, U, V) bytes given element by element - the arithmetic of the contract, no layout.
    `saturate=False` gives the values before sat8."""
    y, u, v = (np.asarray(p).astype(np.int64) for p in (y, u, v))
    uu, vv = u - 128, v - 128
    luma = y - 16
    if clamp_luma:
        luma = np.maximum(luma, 0)
    yy = luma * CY + rounding
    rgb = [shift(yy + CRV * vv), shift(yy + CGV * vv + CGU * uu), shift(yy + CBU * uu)]
    return [np.clip(c, 0, 255) for c in rgb] if saturate else rgb


def i420_to_rgb(planes: np.ndarray, order: str = "rgb", *, swap_uv=False, chroma_shift=0, **clauses) -> np.ndarray:
    """[n, H*3//2, W] u8 -> [n,H,W,3] u8.  The keywords are the clauses the mutants change; the defaults are the contract."""
    assert order in ("rgb", "bgr")
    y, u, v = _planes(planes)
    if swap_uv:
        u, v = v, u
    n, h, w = y.shape
    ys, xs = np.arange(h) // 2, np.minimum((np.arange(w) + chroma_shift) // 2, w // 2 - 1)
    rgb = rgb_of(y, u[:, ys][:, :, xs], v[:, ys][:, :, xs], **clauses)
    return np.stack(rgb if order == "rgb" else rgb[::-1], axis=-1).astype(np.uint8)


MUTANTS = {
    "luma_not_clamped": dict(clamp_luma=False),
    "rounding_dropped": dict(rounding=0),
    "u_v_swapped": dict(swap_uv=True),
    "chroma_from_the_next_column": dict(chroma_shift=1),            # quad (y/2, (x+1)/2)
    "truncation_toward_zero": dict(shift=_trunc_shift),
}


def every_yuv_frame(side: int = 4096) -> np.ndarray:
    """[1, side*3//2, side] u8: quad q of 2^22 has u = q >> 14 & 255, v = q >> 6 & 255 and the four lumas
    4 * (q & 63) + {0, 1, 2, 3} (row-major within the quad), so every (Y, U, V) occurs exactly once at side = 4096."""
    half = side // 2
    q = np.arange(half * half, dtype=np.int64).reshape(half, half)
    base = 4 * (q & 63)
    y = np.empty((side, side), np.int64)
    y[0::2, 0::2], y[0::2, 1::2], y[1::2, 0::2], y[1::2, 1::2] = base, base + 1, base + 2, base + 3
    u, v = (q >> 14) & 255, (q >> 6) & 255
    flat = np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).astype(np.uint8)
    return flat.reshape(1, side * 3 // 2, side)


def extreme_sums():
    """(largest, smallest) sum any channel forms before the shift, over all inputs."""
    top = (255 - 16) * CY + (1 << (SHIFT - 1))
    return top + CBU * 127, (1 << (SHIFT - 1)) + (CGV + CGU) * 127


# ----------------------------------------------------------------------------- the Y4M walk
def y4m_walk(data: bytes):
    """(width, height, offsets) of a YUV4MPEG2 byte string: the header line's W and H tokens, then FRAME lines each
    followed by width * height * 3 // 2 payload bytes; offsets are the payloads'."""
    end = data.index(b"\n")
    tokens = data[:end].split(b" ")
    assert tokens[0] == b"YUV4MPEG2"
    width = next(int(t[1:]) for t in tokens[1:] if t[:1] == b"W")
    height = next(int(t[1:]) for t in tokens[1:] if t[:1] == b"H")
    size = width * height * 3 // 2
    offsets, pos = [], end + 1
    while pos < len(data):
        assert data[pos:pos + 5] == b"FRAME"
        pos = data.index(b"\n", pos) + 1
        offsets.append(pos)
        pos += size
    assert pos == len(data)
    return width, height, offsets
