"""ELVIS v1 block removal on the device: shrink (the server removes the least important blocks of every frame)
and stretch (the client puts the kept blocks back and gets the hole mask the inpainter needs).

The reference's call surface, numpy in and numpy out, with a trailing `device`:

  apply_selective_removal / stretch_frame                         elvis.py:1387-1455   (top-k per block row)
  shrink_frame_row_only / stretch_frame_row_only                  utils.py:692-759     (row passes)
  shrink_frame_position_map / stretch_frame_position_map          utils.py:763-858     (row and column passes)
  shrink_frame_removal_indices / stretch_frame_removal_indices    utils.py:862-1018    (the same passes, index lists)
  shrink_video_frames / stretch_video_frames                      presley.py:761-827   (clip wrappers)

and the clip forms on resident tensors (`shrink_topk_device`, `shrink_passes_device`, `stretch_device`,
`block_gather_device`): `[n,H,W,C]` uint8 frames and `[n,By,Bx]` scores or masks, a whole clip per launch.  Every
shrink and every stretch is one block gather (csrc/shrink.hip) driven by an int32 index map that the selection
kernels build on the device; only `stretch_frame_position_map` / `stretch_frame_removal_indices` build their map
on the host, from side data that is host data by construction.

Contract: scores are compared as float64 (float32 is up-cast exactly, nothing is down-cast); ties of
the pass rule go to the first index as np.argmin does; ties of the top-k rule remove the LOWER column first (the
reference's np.argsort(-row) is not a stable sort, so its ties are not defined); a partial last pass is reproduced as
it is (the row-only form drops the last column without a mask entry, the row-and-column forms keep stale duplicates).
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib, ptr
from .ops import _chk_u8, _s
from .recompose import frames_to_device

MODE_ROWS, MODE_ROWS_COLS = 0, 1        # ELVIS_SHRINK_ROWS, ELVIS_SHRINK_ROWS_COLS
RANK_FLAT, RANK_ROWS = 0, 1             # ELVIS_STRETCH_FLAT, ELVIS_STRETCH_ROWS
_MODES = {"rows": MODE_ROWS, "rows_cols": MODE_ROWS_COLS}
_RANKS = {"flat": RANK_FLAT, "rows": RANK_ROWS}


# ----------------------------------------------------------------------------- host arithmetic (no device)
def topk_count(shrink_amount: float, blocks_x: int) -> int:
    """Blocks removed per row by apply_selective_removal (elvis.py:1392-1396): int(amount * Bx) below 1.0, else
    int(amount), capped at Bx."""
    if not shrink_amount >= 0:
        raise ValueError("shrink_amount must be >= 0")
    k = int(shrink_amount * blocks_x) if shrink_amount < 1.0 else int(shrink_amount)
    return min(k, blocks_x)


def passes_target(blocks_y: int, blocks_x: int, shrink_amount: float) -> int:
    """Blocks removed by the pass rule: int(By * Bx * amount) (utils.py:711)."""
    if not 0 <= shrink_amount <= 1:
        raise ValueError("shrink_amount must be in [0, 1]")
    return int(blocks_y * blocks_x * shrink_amount)


def passes_plan(blocks_y: int, blocks_x: int, target: int, mode: str) -> Tuple[int, int, List[int]]:
    """(shrunk By, shrunk Bx, removals of every pass) of the pass rule - a function of the grid, the target and the
    mode alone, never of the scores (computed by the library on the host)."""
    sby, sbx = C.c_int(0), C.c_int(0)
    cap = blocks_y + blocks_x + 2
    counts = (C.c_int * cap)()
    rc = lib().elvis_shrink_passes_plan(blocks_y, blocks_x, target, _mode(mode), C.addressof(sby), C.addressof(sbx),
                                        C.addressof(counts), cap)
    if rc < 0:
        check(rc)
    return sby.value, sbx.value, [int(v) for v in counts[:rc]]


def _mode(mode) -> int:
    if mode not in _MODES:
        raise ValueError(f"mode must be one of {sorted(_MODES)}")
    return _MODES[mode]


def _grid(h: int, w: int, block_size: int) -> Tuple[int, int]:
    if int(block_size) != block_size or block_size < 1:
        raise ValueError("block_size must be an integer >= 1")
    return h // block_size, w // block_size


# ----------------------------------------------------------------------------- device-resident forms
def _chk_frames(frames_d: torch.Tensor):
    _chk_u8(frames_d)
    if frames_d.dim() != 4 or frames_d.shape[0] < 1 or frames_d.shape[3] not in (1, 3):
        raise ValueError("frames must be a [n,H,W,C] uint8 tensor with n >= 1 and C in {1, 3}")


def _scores_f64(scores_d: torch.Tensor, n: int, by: int, bx: int) -> torch.Tensor:
    if not scores_d.is_cuda or scores_d.dtype not in (torch.float32, torch.float64):
        raise ValueError("scores must be a CUDA float32 or float64 tensor")
    if tuple(scores_d.shape) != (n, by, bx):
        raise ValueError(f"scores {tuple(scores_d.shape)} do not match the block grid {(n, by, bx)}")
    return scores_d.to(torch.float64).contiguous()      # float32 -> float64 is exact


def block_gather_device(frames_d: torch.Tensor, src_of_d: torch.Tensor, block_size: int,
                        src_grid: Optional[Tuple[int, int]] = None, out: Optional[torch.Tensor] = None,
                        fullres_mask: bool = False):
    """out[n, y, x] = block src_of[n, y, x] of frames[n] (a flat index into the source grid), a zero block where
    src_of < 0.  frames [n,hs,ws,C] u8; src_of int32 [n,dBy,dBx]; out [n,dBy*b,dBx*b,C].  `src_grid` defaults to the
    whole blocks of the frames.  With `fullres_mask` the [n,dBy*b,dBx*b] u8 hole mask (255 on zero blocks) is written
    in the same launch and (out, mask) is returned."""
    _chk_frames(frames_d)
    n, hs, ws, c = frames_d.shape
    b = int(block_size)
    sby, sbx = _grid(hs, ws, b) if src_grid is None else (int(src_grid[0]), int(src_grid[1]))
    if src_of_d.dtype != torch.int32 or src_of_d.dim() != 3 or src_of_d.shape[0] != n or not src_of_d.is_cuda:
        raise ValueError("src_of must be a CUDA int32 tensor [n, by, bx]")
    src_of_d = src_of_d.contiguous()
    dby, dbx = int(src_of_d.shape[1]), int(src_of_d.shape[2])
    shape = (n, dby * b, dbx * b, c)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=frames_d.device)
    else:
        _chk_u8(out)
        if tuple(out.shape) != shape:
            raise ValueError(f"out must have the shape {shape}")
    mask = torch.empty(shape[:3], dtype=torch.uint8, device=frames_d.device) if fullres_mask else None
    if dby and dbx:
        check(lib().elvis_block_gather_u8(ptr(frames_d), ptr(src_of_d), ptr(out), ptr(mask), n, hs, ws, c, b, sby, sbx,
                                          dby, dbx, _s(frames_d)), frames_d.device)
    return (out, mask) if fullres_mask else out


def shrink_topk_device(frames_d: torch.Tensor, scores_d: torch.Tensor, block_size: int, shrink_amount: float,
                       out: Optional[torch.Tensor] = None):
    """apply_selective_removal over a resident clip, one selection launch and one gather: per block row the k
    highest scores are removed (the lower column first among equal scores).  Returns (shrunk [n,H,(Bx-k)*b,C] u8,
    mask int8 [n,By,Bx] with 1 = removed, src_of int32 [n,By,Bx-k])."""
    _chk_frames(frames_d)
    n, h, w, c = frames_d.shape
    by, bx = _grid(h, w, block_size)
    if h % block_size or w % block_size:
        raise ValueError("Image dimensions must be divisible by block_size.")      # split_image_into_blocks, elvis.py:1376
    sc = _scores_f64(scores_d, n, by, bx)
    k = topk_count(shrink_amount, bx)
    dev = frames_d.device
    mask = torch.empty((n, by, bx), dtype=torch.int8, device=dev)
    src_of = torch.empty((n, by, bx - k), dtype=torch.int32, device=dev)
    check(lib().elvis_shrink_select_topk(ptr(sc), ptr(mask), ptr(src_of) if k < bx else 0, n, by, bx, k, _s(frames_d)), dev)
    return block_gather_device(frames_d, src_of, block_size, (by, bx), out), mask, src_of


def shrink_passes_device(frames_d: torch.Tensor, scores_d: torch.Tensor, block_size: int, shrink_amount: float,
                         mode: str = "rows", out: Optional[torch.Tensor] = None):
    """The pass rule of utils.py over a resident clip, one selection launch and one gather.  mode "rows" =
    shrink_frame_row_only, "rows_cols" = shrink_frame_position_map / shrink_frame_removal_indices.  Returns
    (shrunk [n,sBy*b,sBx*b,C] u8, mask bool [n,By,Bx], src_of int32 [n,sBy,sBx] - the position map as flat indices
    y * Bx + x -, removal_idx int32 [n,target] in removal order, pass_counts - how to split removal_idx per pass)."""
    _chk_frames(frames_d)
    n, h, w, c = frames_d.shape
    by, bx = _grid(h, w, block_size)
    if by < 1 or bx < 1:
        raise ValueError("the frame is smaller than one block")
    sc = _scores_f64(scores_d, n, by, bx)
    target = passes_target(by, bx, shrink_amount)
    sby, sbx, counts = passes_plan(by, bx, target, mode)
    dev = frames_d.device
    mask = torch.empty((n, by, bx), dtype=torch.uint8, device=dev)
    src_of = torch.empty((n, sby, sbx), dtype=torch.int32, device=dev)
    ridx = torch.empty((n, target), dtype=torch.int32, device=dev)
    ws_scores = torch.empty((n, by, bx), dtype=torch.float64, device=dev)
    ws_pos = torch.empty((n, by, bx), dtype=torch.int32, device=dev)
    check(lib().elvis_shrink_select_passes(ptr(sc), ptr(mask), ptr(src_of) if sby * sbx else 0, ptr(ridx) if target else 0,
                                           ptr(ws_scores), ptr(ws_pos), n, by, bx, target, _mode(mode), sby, sbx,
                                           _s(frames_d)), dev)
    # a rows-only shrink can stop before the target (one column always stays): only the removals made are indices
    ridx = ridx[:, :sum(counts)]
    return block_gather_device(frames_d, src_of, block_size, (by, bx), out), mask.view(torch.bool), src_of, ridx, counts


def stretch_index_device(masks_d: torch.Tensor, shrunk_grid: Tuple[int, int], mode: str = "flat") -> torch.Tensor:
    """The index map of a stretch from its removal masks ([n,By,Bx] bool / int8 / uint8 on the device, non-zero =
    removed): the rank of every kept block among the kept blocks of its frame ("flat") or of its row ("rows"), -1 for
    removed blocks and for ranks outside the shrunk grid."""
    if mode not in _RANKS:
        raise ValueError(f"mode must be one of {sorted(_RANKS)}")
    if not masks_d.is_cuda or masks_d.dim() != 3 or masks_d.dtype not in (torch.bool, torch.int8, torch.uint8):
        raise ValueError("masks must be a CUDA bool, int8 or uint8 tensor [n, by, bx]")
    m = masks_d.contiguous().view(torch.uint8)
    n, by, bx = m.shape
    src_of = torch.empty((n, by, bx), dtype=torch.int32, device=m.device)
    if n and by and bx:
        check(lib().elvis_stretch_index(ptr(m), ptr(src_of), n, by, bx, int(shrunk_grid[0]), int(shrunk_grid[1]),
                                        _RANKS[mode], _s(m)), m.device)
    return src_of


def stretch_device(shrunk_d: torch.Tensor, masks_d: torch.Tensor, block_size: int, mode: str = "flat",
                   out: Optional[torch.Tensor] = None, fullres_mask: bool = False):
    """Stretch a resident clip: the kept blocks of shrunk [n,hs,ws,C] go back to the positions masks [n,By,Bx] keep
    (zero = kept), removed blocks are zero.  mode "flat" = stretch_frame / stretch_video_frames (blocks in flat
    row-major order), "rows" = stretch_frame_row_only.  PRECONDITION of stretch_frame: the kept count equals the
    number of shrunk blocks (not checked here - no synchronisation; surplus blocks are zero, as in
    stretch_video_frames).  With `fullres_mask` returns (frames, [n,By*b,Bx*b] u8 mask, 255 = removed)."""
    _chk_frames(shrunk_d)
    n, hs, ws, c = shrunk_d.shape
    if hs % block_size or ws % block_size:
        raise ValueError("Image dimensions must be divisible by block_size.")
    if masks_d.dim() != 3 or masks_d.shape[0] != n:
        raise ValueError(f"masks must be [n, by, bx] for {n} frame(s)")
    grid = _grid(hs, ws, block_size)
    if mode == "rows" and grid[0] < masks_d.shape[1]:
        raise ValueError("stretch_frame_row_only: the shrunk frame has fewer block rows than the mask")
    src_of = stretch_index_device(masks_d, grid, mode)
    return block_gather_device(shrunk_d, src_of, block_size, grid, out, fullres_mask)


# ----------------------------------------------------------------------------- the reference's call surface
def _frame(frame, what: str) -> np.ndarray:
    f = np.asarray(frame)
    if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] not in (1, 3):
        raise ValueError(f"{what}: frames are uint8 (H,W,C) arrays with C in {{1, 3}}")
    return f


def _scores(scores, grid: Tuple[int, int], what: str) -> np.ndarray:
    s = np.asarray(scores)
    if s.ndim != 2 or s.dtype.kind not in "fiub" or tuple(s.shape) != tuple(grid):
        raise ValueError(f"{what}: scores {s.shape} do not match the block grid {tuple(grid)}")
    s = s.astype(np.float64)
    if np.isnan(s).any():
        raise ValueError(f"{what}: NaN scores")
    return s


def _mask(mask, what: str) -> np.ndarray:
    m = np.asarray(mask)
    if m.ndim != 2 or m.dtype.kind not in "biu":
        raise ValueError(f"{what}: the mask is a 2-D bool or integer array")
    return np.ascontiguousarray(m != 0).view(np.uint8)


def _up(a: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _gather_host_map(frame: np.ndarray, src_of: np.ndarray, block_size: int, grid, dev) -> np.ndarray:
    with torch.cuda.device(dev):
        return block_gather_device(_up(frame[None], dev), _up(src_of.astype(np.int32)[None], dev), block_size, grid)[0].cpu().numpy()


def apply_selective_removal(image: np.ndarray, frame_scores: np.ndarray, block_size: int, shrink_amount: float,
                            device="cuda:0") -> Tuple[np.ndarray, np.ndarray, List[List[int]]]:
    """elvis.py:1387-1427 on the device: per block row the k = int(amount * Bx) (int(amount) from 1.0 on, capped at
    Bx) highest scores are removed and the row closes up.  Returns (new image, int8 mask with 1 = removed, the removed
    columns of every row in ascending order).  Equal scores: the lower column is removed first (module docstring)."""
    img = _frame(image, "apply_selective_removal")
    h, w, c = img.shape
    if h % block_size or w % block_size:
        raise ValueError("Image dimensions must be divisible by block_size.")
    sc = _scores(frame_scores, _grid(h, w, block_size), "apply_selective_removal")
    if sc.size == 0:
        raise ValueError("apply_selective_removal: the frame is smaller than one block")
    topk_count(shrink_amount, sc.shape[1])
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        out, mask, _ = shrink_topk_device(_up(img[None], dev), _up(sc[None], dev), block_size, shrink_amount)
        mask_h = mask[0].cpu().numpy()
        return out[0].cpu().numpy(), mask_h, [np.nonzero(r)[0].tolist() for r in mask_h]


def stretch_frame(shrunk_frame: np.ndarray, binary_mask: np.ndarray, block_size: int, device="cuda:0") -> np.ndarray:
    """elvis.py:1436-1455 on the device: the blocks of the shrunk frame, in flat row-major order, go to the positions
    where the mask is 0; the others are zero.  ValueError (numpy's, in the reference) when the number of kept
    positions differs from the number of shrunk blocks."""
    f = _frame(shrunk_frame, "stretch_frame")
    m = _mask(binary_mask, "stretch_frame")
    h, w, _ = f.shape
    if h % block_size or w % block_size:
        raise ValueError("Image dimensions must be divisible by block_size.")
    sby, sbx = _grid(h, w, block_size)
    kept = int(m.size - m.sum())
    if kept != sby * sbx:
        raise ValueError(f"stretch_frame: cannot assign {sby * sbx} shrunk blocks to the {kept} positions the mask keeps")
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        return stretch_device(_up(f[None], dev), _up(m[None], dev), block_size, "flat")[0].cpu().numpy()


def _shrink_passes(frame, importance, block_size, shrink_amount, mode, device, what):
    f = _frame(frame, what)
    by, bx = _grid(f.shape[0], f.shape[1], block_size)
    if by < 1 or bx < 1:
        raise ValueError(f"{what}: the frame is smaller than one block")
    sc = _scores(importance, (by, bx), what)
    passes_target(by, bx, shrink_amount)
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        out, mask, src_of, ridx, counts = shrink_passes_device(_up(f[None], dev), _up(sc[None], dev), block_size,
                                                               shrink_amount, mode)
        return out[0].cpu().numpy(), mask[0].cpu().numpy(), src_of[0].cpu().numpy(), ridx[0].cpu().numpy(), counts, bx


def shrink_frame_row_only(frame: np.ndarray, importance: np.ndarray, block_size: int, shrink_amount: float,
                          device="cuda:0") -> Tuple[np.ndarray, np.ndarray]:
    """utils.py:692-736 on the device: row passes remove every row's least important remaining block until
    int(By * Bx * amount) are gone (one column always stays).  Returns (shrunk frame, bool mask).  A partial last pass
    still drops the last column: rows it did not reach lose their last block without a mask entry."""
    out, mask, _, _, _, _ = _shrink_passes(frame, importance, block_size, shrink_amount, "rows", device, "shrink_frame_row_only")
    return out, mask


def shrink_frame_position_map(frame: np.ndarray, importance: np.ndarray, block_size: int, shrink_amount: float,
                              device="cuda:0") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """utils.py:763-836 on the device: alternating row and column passes.  Returns (shrunk frame, bool mask, int64
    position map [sBy,sBx,2]: shrunk block -> (orig_y, orig_x)).  A partial last pass does not shrink the grid: the
    lines it shifted end with a stale duplicate."""
    out, mask, src_of, _, _, bx = _shrink_passes(frame, importance, block_size, shrink_amount, "rows_cols", device,
                                                 "shrink_frame_position_map")
    return out, mask, np.stack([src_of // bx, src_of % bx], axis=-1).astype(np.int64)


def shrink_frame_removal_indices(frame: np.ndarray, importance: np.ndarray, block_size: int, shrink_amount: float,
                                 device="cuda:0") -> Tuple[np.ndarray, np.ndarray, list]:
    """utils.py:862-948 on the device: the removal sequence of `shrink_frame_position_map`; the side data is the list
    of int32 arrays of removed indices, one per pass (row pass, column pass, ...)."""
    out, mask, _, ridx, counts, _ = _shrink_passes(frame, importance, block_size, shrink_amount, "rows_cols", device,
                                                   "shrink_frame_removal_indices")
    cuts = np.cumsum([0] + counts)
    return out, mask, [ridx[cuts[i]:cuts[i + 1]].astype(np.int32) for i in range(len(counts))]


def stretch_frame_row_only(shrunk_frame: np.ndarray, removal_mask: np.ndarray, block_size: int,
                           device="cuda:0") -> np.ndarray:
    """utils.py:739-759 on the device: per row, the shrunk blocks go to the kept columns in order; kept columns
    beyond the shrunk width stay zero."""
    f = _frame(shrunk_frame, "stretch_frame_row_only")
    m = _mask(removal_mask, "stretch_frame_row_only")
    if f.shape[0] % block_size or f.shape[1] % block_size:
        raise ValueError("Image dimensions must be divisible by block_size.")
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        return stretch_device(_up(f[None], dev), _up(m[None], dev), block_size, "rows")[0].cpu().numpy()


def position_map_to_src_of(position_map: np.ndarray, orig_grid: Tuple[int, int]) -> np.ndarray:
    """int32 [By,Bx]: for every original block the flat index of the shrunk block the position map sends there, -1
    where none does.  Shrunk blocks are placed in row-major order, so the last one wins a contested position."""
    pm = np.asarray(position_map)
    by, bx = orig_grid
    if pm.ndim != 3 or pm.shape[2] != 2 or pm.dtype.kind not in "iu":
        raise ValueError("position_map must be an integer array [sBy, sBx, 2]")
    pm = pm.astype(np.int64)
    if pm.size and (pm.min() < 0 or pm[..., 0].max() >= by or pm[..., 1].max() >= bx):
        raise ValueError("position_map points outside the original block grid")
    src_of = np.full(by * bx, -1, np.int64)
    np.maximum.at(src_of, (pm[..., 0] * bx + pm[..., 1]).ravel(), np.arange(pm.shape[0] * pm.shape[1]))
    return src_of.reshape(by, bx).astype(np.int32)


def stretch_frame_position_map(shrunk_frame: np.ndarray, removal_mask: np.ndarray, position_map: np.ndarray,
                               block_size: int, device="cuda:0") -> np.ndarray:
    """utils.py:839-858 on the device: every shrunk block goes to the position its map entry names (row-major order,
    so a later duplicate overwrites an earlier one); everything else is zero.  The mask only gives the grid."""
    f = _frame(shrunk_frame, "stretch_frame_position_map")
    grid = tuple(np.asarray(removal_mask).shape)
    if len(grid) != 2 or f.shape[0] % block_size or f.shape[1] % block_size:
        raise ValueError("stretch_frame_position_map: bad mask or frame shape")
    sgrid = _grid(f.shape[0], f.shape[1], block_size)
    if tuple(np.asarray(position_map).shape[:2]) != sgrid:
        raise ValueError(f"position_map {np.asarray(position_map).shape} does not match the shrunk grid {sgrid}")
    if grid[0] < 1 or grid[1] < 1:
        return np.zeros((grid[0] * block_size, grid[1] * block_size, f.shape[2]), np.uint8)
    return _gather_host_map(f, position_map_to_src_of(position_map, grid), block_size, sgrid, L.resolve_device(device))


def _open_gap(g: np.ndarray, where) -> np.ndarray:
    """One more column on the right of the index grid `g`; row r's entries from column where[r] on move right by one
    and leave a hole (-1).  Rows beyond len(where) keep their place."""
    rows, cols = g.shape
    at = np.full(rows, cols, np.int64)
    k = min(len(where), rows)
    at[:k] = np.minimum(np.asarray(where[:k], np.int64), cols)
    out = np.full((rows, cols + 1), -1, np.int64)
    c = np.arange(cols)[None, :]
    out[np.arange(rows)[:, None], c + (c >= at[:, None])] = g
    return out


def removal_indices_to_src_of(removal_indices: Sequence[np.ndarray], shrunk_grid: Tuple[int, int]) -> np.ndarray:
    """The index grid `stretch_frame_removal_indices` rebuilds (before its final crop): the passes are undone last
    to first, even entries as row passes (a hole opens in every listed row), odd ones as column passes."""
    sby, sbx = shrunk_grid
    g = np.arange(sby * sbx, dtype=np.int64).reshape(sby, sbx)
    for p in range(len(removal_indices) - 1, -1, -1):
        idx = np.asarray(removal_indices[p])
        if idx.ndim != 1 or (idx.size and (idx.dtype.kind not in "iu" or idx.min() < 0)):
            raise ValueError("removal_indices must be 1-D arrays of non-negative integers")
        g = _open_gap(g, idx) if p % 2 == 0 else _open_gap(g.T, idx).T
    return g.astype(np.int32)


def stretch_frame_removal_indices(shrunk_frame: np.ndarray, removal_indices: list, orig_blocks_y: int, orig_blocks_x: int,
                                  block_size: int, device="cuda:0") -> np.ndarray:
    """utils.py:951-1018 on the device: the passes are undone in reverse with zero blocks inserted at the recorded
    indices, and the result is cropped to the original grid.  The index math runs on the host (the list is host data);
    the pixels move once."""
    f = _frame(shrunk_frame, "stretch_frame_removal_indices")
    if f.shape[0] % block_size or f.shape[1] % block_size:
        raise ValueError("Image dimensions must be divisible by block_size.")
    sgrid = _grid(f.shape[0], f.shape[1], block_size)
    src_of = removal_indices_to_src_of(removal_indices, sgrid)[:orig_blocks_y, :orig_blocks_x]
    if src_of.size == 0:
        return np.zeros((src_of.shape[0] * block_size, src_of.shape[1] * block_size, f.shape[2]), np.uint8)
    return _gather_host_map(f, src_of, block_size, sgrid, L.resolve_device(device))


def _uniform(arrays) -> bool:
    return len({np.asarray(a).shape for a in arrays}) == 1


def shrink_video_frames(frames: List[np.ndarray], importance_scores: List[np.ndarray], block_size: int,
                        shrink_amount: float, method: Callable = None, device="cuda:0") -> Tuple[List[np.ndarray], List[Any]]:
    """presley.py:761-784: (shrunk frames, removal masks) of a clip.  `method` is a shrink function returning
    (frame, mask) - `shrink_frame_row_only` (the default), for which a clip of equally sized frames is one selection
    launch and one gather; any other callable is applied frame by frame as in the reference."""
    method = shrink_frame_row_only if method is None else method
    pairs = list(zip(frames, importance_scores))
    if not pairs:
        return [], []
    if method is not shrink_frame_row_only or not (_uniform(f for f, _ in pairs) and _uniform(s for _, s in pairs)):
        kw = {"device": device} if getattr(method, "__module__", None) == __name__ else {}
        outs, masks = [], []
        for f, s in pairs:
            shrunken, removal_mask = method(f, s, block_size, shrink_amount, **kw)
            outs.append(shrunken)
            masks.append(removal_mask)
        return outs, masks
    fs = [_frame(f, "shrink_video_frames") for f, _ in pairs]
    by, bx = _grid(fs[0].shape[0], fs[0].shape[1], block_size)
    if by < 1 or bx < 1:
        raise ValueError("shrink_video_frames: the frame is smaller than one block")
    sc = np.stack([_scores(s, (by, bx), "shrink_video_frames") for _, s in pairs])
    passes_target(by, bx, shrink_amount)
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        out, mask, _, _, _ = shrink_passes_device(frames_to_device(fs, dev), _up(sc, dev), block_size, shrink_amount, "rows")
        out_h, mask_h = out.cpu().numpy(), mask.cpu().numpy()
    return [out_h[i] for i in range(len(fs))], [mask_h[i] for i in range(len(fs))]


def stretch_video_frames(shrunken_frames: List[np.ndarray], removal_masks: List[np.ndarray], block_size: int,
                         device="cuda:0") -> List[np.ndarray]:
    """presley.py:787-827 on the device: per frame, the kept positions of the mask in row-major order take the shrunk
    blocks in flat order; positions beyond the shrunk grid stay zero (bounds-checked, never an error).  A clip of
    equally sized frames and masks is one launch pair."""
    if not shrunken_frames:
        return []
    fs = [_frame(f, "stretch_video_frames") for f in shrunken_frames]
    ms = [_mask(removal_masks[i], "stretch_video_frames") for i in range(len(fs))]
    for f in fs:
        if f.shape[0] % block_size or f.shape[1] % block_size:
            raise ValueError("Image dimensions must be divisible by block_size.")
    dev = L.resolve_device(device)
    groups = [range(len(fs))] if _uniform(fs) and _uniform(ms) else [[i] for i in range(len(fs))]
    out: List[np.ndarray] = []
    with torch.cuda.device(dev):
        for g in groups:
            m = np.stack([ms[i] for i in g])
            if m.shape[1] == 0 or m.shape[2] == 0:
                out.extend(np.zeros((m.shape[1] * block_size, m.shape[2] * block_size, fs[0].shape[2]), np.uint8) for _ in g)
                continue
            res = stretch_device(frames_to_device([fs[i] for i in g], dev), _up(m, dev), block_size, "flat").cpu().numpy()
            out.extend(res[j] for j in range(len(g)))
    return out
