"""numpy restatement of the encoder hand-off (elvis_amd/handoff.py, csrc/handoff.hip) - what the device output and the
host rules are pinned against, bit for bit.  Written from the rules, not from the code under test: the colour
conversion is three int64 matrix rows over whole clips, the float area resize walks the table output by output.

  * `yuv_of` / `rgb_to_i420`: cv2.cvtColor(frame, COLOR_RGB2YUV_I420 / COLOR_BGR2YUV_I420), restated from OpenCV 4.x
    RGB8toYUV420pInvoker (20-bit fixed point; U and V from the even-row, even-column pixel of each 2x2 quad);
  * `yuv420p_bytes`, `y4m_bytes`: the byte streams of convert_frames_to_yuv420p (presley.py:217-223) and write_y4m
    (utils.py:453-462);
  * `calculate_importance_scores` (utils.py:665-688), `kvazaar_roi_bytes` (utils.py:1026-1053), `svtav1_roi_text`
    (utils.py:1056-1092) with `resize_area_f32` for its one cv2.resize call; `CvStub` is what
    tools/make_handoff_golden.py hands the reference in place of cv2.
"""
from __future__ import annotations

from typing import List

import numpy as np

from _presley_degrade_ref import area_entries

SHIFT = 20
Y_ROW = (269484, 528482, 102760)          # R, G, B
U_ROW = (-155188, -305135, 460324)
V_ROW = (460324, -385875, -74448)
Y_BIAS, C_BIAS = 16, 128
INTER_AREA = 3                            # cv2's flag values
COLOR_RGB2YUV_I420, COLOR_BGR2YUV_I420 = 127, 128


def _row(rgb: np.ndarray, coef, bias: int) -> np.ndarray:
    x = rgb.astype(np.int64)
    return (coef[0] * x[..., 0] + coef[1] * x[..., 1] + coef[2] * x[..., 2] + (1 << (SHIFT - 1)) + (bias << SHIFT)) >> SHIFT


def yuv_of(rgb: np.ndarray):
    """(Y, U, V) as int64 of every R,G,B triple in `rgb` [..., 3], unclipped (the range test is about that)."""
    return _row(rgb, Y_ROW, Y_BIAS), _row(rgb, U_ROW, C_BIAS), _row(rgb, V_ROW, C_BIAS)


def rgb_to_i420(frames: np.ndarray, order: str = "rgb") -> np.ndarray:
    """[n,H,W,3] u8 -> [n, H*3//2, W] u8: Y, then U, then V, each plane dense."""
    assert frames.ndim == 4 and frames.shape[3] == 3 and frames.dtype == np.uint8 and order in ("rgb", "bgr")
    n, h, w, _ = frames.shape
    assert h % 2 == 0 and w % 2 == 0
    rgb = frames if order == "rgb" else frames[..., ::-1]
    y, _, _ = yuv_of(rgb)
    _, u, v = yuv_of(rgb[:, ::2, ::2])
    for plane in (y, u, v):
        assert plane.size == 0 or (plane.min() >= 0 and plane.max() <= 255)
    out = np.concatenate([y.reshape(n, -1), u.reshape(n, -1), v.reshape(n, -1)], axis=1).astype(np.uint8)
    return out.reshape(n, h * 3 // 2, w)


def yuv420p_bytes(frames: List[np.ndarray]) -> bytes:
    return b"".join(rgb_to_i420(f[None]).tobytes() for f in frames)


def y4m_header(width: int, height: int, framerate: float) -> bytes:
    return b"YUV4MPEG2 W%d H%d F%d:1000 Ip A1:1 C420\n" % (width, height, int(round(framerate * 1000)))


def y4m_bytes(frames: List[np.ndarray], framerate: float) -> bytes:
    h, w = frames[0].shape[:2]
    return y4m_header(w, h, framerate) + b"".join(b"FRAME\n" + rgb_to_i420(f[None]).tobytes() for f in frames)


# ----------------------------------------------------------------------------- the block-grid rules
def calculate_importance_scores(alpha, beta, sc: np.ndarray, tc: np.ndarray, masks: np.ndarray) -> np.ndarray:
    """[F,By,Bx] scores, frame by frame in the arrays' dtype: mix with the next frame's TC, smooth with the previous
    frame, flip the sign where the mask is under 0.5 (and scale by it elsewhere), min-max with + 1e-8."""
    count = sc.shape[0]
    mixed = [alpha * sc[f] + (1 - alpha) * tc[f + 1] if f + 1 < count else sc[f].copy() for f in range(count)]
    out = []
    for f in range(count):
        value = mixed[f] if f == 0 else beta * mixed[f] + (1 - beta) * mixed[f - 1]
        value = (value * np.where(masks[f] < 0.5, masks.dtype.type(-1.0), masks[f])).astype(sc.dtype)
        low, high = value.min(keepdims=True), value.max(keepdims=True)          # arrays: the 1e-8 joins in their dtype
        out.append((value - low) / (high - low + 1e-8))
    return np.stack(out).astype(sc.dtype)


def kvazaar_delta_qp(importance: np.ndarray, base_qp: int, qp_range: int = 15) -> np.ndarray:
    delta = (1.0 - importance) * 2 * qp_range - qp_range
    delta = np.minimum(np.maximum(delta, -14), 14)
    delta = np.minimum(np.maximum(delta, 0 - base_qp), 51 - base_qp)
    return np.trunc(delta).astype(np.int8)                      # astype(int8) of a float cuts toward zero


def kvazaar_roi_bytes(importance_scores, base_qp: int, qp_range: int = 15) -> bytes:
    out = b""
    for imp in importance_scores:
        out += np.asarray([imp.shape[1], imp.shape[0]], "<i4").tobytes() + kvazaar_delta_qp(imp, base_qp, qp_range).tobytes()
    return out


def resize_area_f32(grid: np.ndarray, cols: int, rows: int) -> np.ndarray:
    """cv2.resize(float32, (cols, rows), INTER_AREA) onto a smaller grid.  Whole ratio in both axes (ResizeAreaFast):
    float32 sum over the cell in raster order, times 1.f / area.  Otherwise (ResizeArea): per source row
    buf[dx] += S[sx] * alpha over the x table, per destination row sum[dx] (+)= beta * buf[dx] over the y table."""
    grid = grid.astype(np.float32)
    sr, sc = grid.shape
    assert sr > rows and sc > cols
    out = np.zeros((rows, cols), np.float32)
    if sr % rows == 0 and sc % cols == 0:
        fy, fx = sr // rows, sc // cols
        inv = np.float32(1.0 / (fy * fx))
        for r in range(rows):
            for c in range(cols):
                total = np.float32(0)
                for v in grid[r * fy:(r + 1) * fy, c * fx:(c + 1) * fx].reshape(-1):
                    total = np.float32(total + v)
                out[r, c] = total * inv
        return out
    buf = np.zeros((sr, cols), np.float32)
    for dx, sx, a in area_entries(sc, cols):
        buf[:, dx] = buf[:, dx] + grid[:, sx] * a
    seen = set()
    for dy, sy, b in area_entries(sr, rows):
        out[dy] = b * buf[sy] if dy not in seen else out[dy] + b * buf[sy]
        seen.add(dy)
    return out


def svtav1_levels_margin(importance: np.ndarray, width: int, height: int) -> float:
    """How far 8 * resized is from a whole number, at its closest: what the unpinned float resize has to stay inside."""
    v = resize_area_f32(importance, (width + 63) // 64, (height + 63) // 64).astype(np.float64) * 8
    return float(np.abs(v - np.rint(v)).min())


def svtav1_delta_qp(importance: np.ndarray, base_crf: int, qp_range: int, width: int, height: int) -> np.ndarray:
    resized = resize_area_f32(importance, (width + 63) // 64, (height + 63) // 64)
    levels = np.clip(np.floor(resized.astype(np.float64) * 8).astype(np.int64), 0, 7)      # resized >= 0: floor is the int cast
    assert resized.min() >= 0
    delta = qp_range - (levels * 2 * qp_range) // 7
    return np.clip(delta, 0 - base_crf, 63 - base_crf)


def svtav1_roi_text(importance_scores, base_crf: int, qp_range: int, width: int, height: int) -> str:
    lines = []
    for i, imp in enumerate(importance_scores):
        lines.append(" ".join([str(i)] + [str(int(v)) for v in svtav1_delta_qp(imp, base_crf, qp_range, width, height).reshape(-1)]))
    return "".join(line + "\n" for line in lines)


class CvStub:
    """The three cv2 names the reference's hand-off functions touch, for tools/make_handoff_golden.py: `resize` is the
    restatement, `cvtColor` the restatement's planes (and a record of the codes it was asked for)."""
    INTER_AREA = INTER_AREA
    COLOR_RGB2YUV_I420, COLOR_BGR2YUV_I420 = COLOR_RGB2YUV_I420, COLOR_BGR2YUV_I420

    def __init__(self):
        self.codes = []

    def resize(self, img, dsize, interpolation=1):
        assert interpolation == INTER_AREA and img.dtype == np.float32 and img.ndim == 2
        return resize_area_f32(img, dsize[0], dsize[1])

    def cvtColor(self, frame, code):
        self.codes.append(int(code))
        assert code in (COLOR_RGB2YUV_I420, COLOR_BGR2YUV_I420)
        return rgb_to_i420(frame[None], "rgb" if code == COLOR_RGB2YUV_I420 else "bgr")[0]
