"""Numpy restatement of the ELVIS v1 shrink / stretch rules, in this project's own words: every function is "build an
index grid, then move whole blocks once".  Pinned bit for bit against the reference's own outputs
(tests/golden/shrink.npz, tests/test_shrink_host.py); the device code is compared against it on shapes the goldens
are too small for (tests/test_gpu_shrink.py)."""
import numpy as np


# ----------------------------------------------------------------------------- test frames
def make_frame(h, w, block, c=3, salt=0):
    """A frame whose blocks can be told apart and whose block interior has an orientation, yet compresses well:
    channels 0 and 2 = the block's number (low / high byte), channel 1 labels the block's top row with the column
    and its left column with the row (one channel: the three folded together); pixels beyond the block grid get
    their own values."""
    y, x = np.mgrid[0:h, 0:w]
    bid = (y // block) * (w // block + 1) + x // block + 1 + salt
    iy, ix = y % block, x % block
    planes = [bid % 256, np.where(iy == 0, ix + 1, 0) + np.where(ix == 0, iy + 1, 0), bid // 256]
    f = np.stack(planes, axis=-1).astype(np.uint8)
    if c == 1:
        f = (f[..., :1] * 3) ^ (f[..., 1:2] * 16) ^ f[..., 2:]
    f[(h // block) * block:] = 250
    f[:, (w // block) * block:] = 251
    return f


# ----------------------------------------------------------------------------- whole blocks
def to_blocks(frame, block, grid=None):
    by, bx = (frame.shape[0] // block, frame.shape[1] // block) if grid is None else grid
    c = frame.shape[2]
    return frame[:by * block, :bx * block].reshape(by, block, bx, block, c).transpose(0, 2, 1, 3, 4)


def from_blocks(blocks):
    by, bx, b, _, c = blocks.shape
    return blocks.transpose(0, 2, 1, 3, 4).reshape(by * b, bx * b, c)


def gather_blocks(frame, src_of, block, src_grid=None):
    """out block (y, x) = source block number src_of[y, x] (flat, row-major in the source grid); zero where the index
    is negative or beyond the source grid."""
    src = to_blocks(frame, block, src_grid)
    flat = src.reshape((-1,) + src.shape[2:])
    src_of = np.asarray(src_of)
    out = np.zeros(src_of.shape + src.shape[2:], np.uint8)
    ok = (src_of >= 0) & (src_of < flat.shape[0])
    out[ok] = flat[src_of[ok]]
    return from_blocks(out)


def fullres_mask(src_of, block):
    holes = np.where(np.asarray(src_of) < 0, 255, 0).astype(np.uint8)
    return np.repeat(np.repeat(holes, block, axis=0), block, axis=1)


# ----------------------------------------------------------------------------- selection: top-k per row
def topk_count(amount, bx):
    return min(int(amount * bx) if amount < 1.0 else int(amount), bx)


def topk_select(scores, k):
    """(int8 mask, src_of of the shrunk frame): per row the k highest scores go, the lower column first among equals."""
    scores = np.asarray(scores, np.float64)
    by, bx = scores.shape
    mask = np.zeros((by, bx), np.int8)
    for r in range(by):
        order = sorted(range(bx), key=lambda i: (-scores[r, i], i))
        mask[r, order[:k]] = 1
    keep = np.stack([np.flatnonzero(mask[r] == 0) for r in range(by)]) if by else np.zeros((0, bx - k), np.int64)
    return mask, (keep + np.arange(by)[:, None] * bx).astype(np.int32)


# ----------------------------------------------------------------------------- selection: passes
def passes_select(scores, target, rows_only):
    """Alternating passes over the lines of a (score, origin) table.  A pass visits the lines in order and stops when
    the target is reached; a visited line loses its first minimum and closes up towards its start.  Row passes shorten
    the rows (always in the rows-only form, else only when every row was visited), column passes shorten the columns
    when every column was visited.  Returns (bool mask, final origin table as flat indices, per-pass index lists)."""
    sc = np.array(scores, np.float64)
    by, bx = sc.shape
    origin = np.arange(by * bx).reshape(by, bx)
    mask = np.zeros(by * bx, bool)
    live = [by, bx]                                   # current number of rows, columns
    removed, passes, axis = 0, [], 0                  # axis 0: the lines are rows

    def sweep(s, o, n_lines, length):
        nonlocal removed
        hit = []
        for line in range(min(n_lines, target - removed)):
            i = int(np.argmin(s[line, :length]))
            mask[o[line, i]] = True
            s[line, i:length - 1] = s[line, i + 1:length].copy()
            o[line, i:length - 1] = o[line, i + 1:length].copy()
            hit.append(i)
        removed += len(hit)
        return hit

    while removed < target and live[0] > 0 and live[1] > 0 and not (rows_only and live[1] <= 1):
        if axis == 0:
            hit = sweep(sc, origin, live[0], live[1])
            if rows_only or len(hit) == live[0]:
                live[1] -= 1
        else:
            hit = sweep(sc.T, origin.T, live[1], live[0])
            if len(hit) == live[1]:
                live[0] -= 1
        passes.append(np.array(hit, np.int32))
        if not rows_only:
            axis ^= 1
    return mask.reshape(by, bx), origin[:live[0], :live[1]].astype(np.int32), passes


# ----------------------------------------------------------------------------- index grids of the stretches
def flat_rank_src_of(mask, shrunk_grid):
    kept = np.asarray(mask) == 0
    rank = np.cumsum(kept.ravel()) - 1
    ok = kept.ravel() & (rank < shrunk_grid[0] * shrunk_grid[1])
    return np.where(ok, rank, -1).reshape(kept.shape).astype(np.int32)


def row_rank_src_of(mask, shrunk_grid):
    kept = np.asarray(mask) == 0
    rank = np.cumsum(kept, axis=1) - 1
    rows = np.arange(kept.shape[0])[:, None]
    ok = kept & (rank < shrunk_grid[1]) & (rows < shrunk_grid[0])
    return np.where(ok, rows * shrunk_grid[1] + rank, -1).astype(np.int32)


def position_map_src_of(position_map, grid):
    src_of = np.full(grid, -1, np.int32)
    sby, sbx = position_map.shape[:2]
    for i in range(sby * sbx):                        # later shrunk blocks overwrite earlier ones
        oy, ox = position_map[i // sbx, i % sbx]
        src_of[oy, ox] = i
    return src_of


def _widen(g, idx):
    """Every row of the index grid gets one more entry: a hole (-1) at idx[r], or at the end for rows idx does not list."""
    rows, cols = g.shape
    out = np.full((rows, cols + 1), -1, np.int64)
    for r in range(rows):
        line = list(g[r])
        line.insert(min(int(idx[r]), cols) if r < len(idx) else cols, -1)
        out[r] = line
    return out


def removal_indices_src_of(passes, shrunk_grid):
    """Undo the passes last to first: even list entries were row passes, odd ones column passes."""
    sby, sbx = shrunk_grid
    g = np.arange(sby * sbx, dtype=np.int64).reshape(sby, sbx)
    for p in range(len(passes) - 1, -1, -1):
        g = _widen(g, passes[p]) if p % 2 == 0 else _widen(g.T, passes[p]).T
    return g.astype(np.int32)


# ----------------------------------------------------------------------------- the reference's names
def apply_selective_removal(image, frame_scores, block_size, shrink_amount):
    if image.shape[0] % block_size or image.shape[1] % block_size:
        raise ValueError("Image dimensions must be divisible by block_size.")
    by, bx = frame_scores.shape
    mask, src_of = topk_select(frame_scores, topk_count(shrink_amount, bx))
    return gather_blocks(image, src_of, block_size), mask, [np.flatnonzero(r).tolist() for r in mask]


def stretch_frame(shrunk_frame, binary_mask, block_size):
    grid = (shrunk_frame.shape[0] // block_size, shrunk_frame.shape[1] // block_size)
    kept = int((np.asarray(binary_mask) == 0).sum())
    if kept != grid[0] * grid[1]:
        raise ValueError(f"cannot assign {grid[0] * grid[1]} blocks to {kept} kept positions")
    return gather_blocks(shrunk_frame, flat_rank_src_of(binary_mask, grid), block_size)


def _passes(frame, importance, block_size, shrink_amount, rows_only):
    by, bx = frame.shape[0] // block_size, frame.shape[1] // block_size
    mask, origin, passes = passes_select(importance, int(by * bx * shrink_amount), rows_only)
    return gather_blocks(frame, origin, block_size, (by, bx)), mask, origin, passes, bx


def shrink_frame_row_only(frame, importance, block_size, shrink_amount):
    out, mask, _, _, _ = _passes(frame, importance, block_size, shrink_amount, True)
    return out, mask


def shrink_frame_position_map(frame, importance, block_size, shrink_amount):
    out, mask, origin, _, bx = _passes(frame, importance, block_size, shrink_amount, False)
    return out, mask, np.stack([origin // bx, origin % bx], axis=-1).astype(np.int64)


def shrink_frame_removal_indices(frame, importance, block_size, shrink_amount):
    out, mask, _, passes, _ = _passes(frame, importance, block_size, shrink_amount, False)
    return out, mask, passes


def _shrunk_grid(frame, block_size):
    return frame.shape[0] // block_size, frame.shape[1] // block_size


def stretch_frame_row_only(shrunk_frame, removal_mask, block_size):
    return gather_blocks(shrunk_frame, row_rank_src_of(removal_mask, _shrunk_grid(shrunk_frame, block_size)), block_size)


def stretch_frame_position_map(shrunk_frame, removal_mask, position_map, block_size):
    return gather_blocks(shrunk_frame, position_map_src_of(position_map, removal_mask.shape), block_size)


def stretch_frame_removal_indices(shrunk_frame, removal_indices, orig_blocks_y, orig_blocks_x, block_size):
    src_of = removal_indices_src_of(removal_indices, _shrunk_grid(shrunk_frame, block_size))
    return gather_blocks(shrunk_frame, src_of[:orig_blocks_y, :orig_blocks_x], block_size)


def stretch_video_frames(shrunken_frames, removal_masks, block_size):
    return [gather_blocks(f, flat_rank_src_of(removal_masks[i], _shrunk_grid(f, block_size)), block_size)
            for i, f in enumerate(shrunken_frames)]


# ----------------------------------------------------------------------------- golden file access
FAMILIES = ("elvis", "row_only", "position_map")


def golden_cases(npz):
    """[(index, dict of that case's arrays)] of tests/golden/shrink.npz; removal index lists are rebuilt from the
    flat array and the per-pass counts."""
    cases = []
    for i in range(int(npz["n_cases"])):
        pre = f"c{i}_"
        d = {k[len(pre):]: npz[k] for k in npz.files if k.startswith(pre)}
        d["family"] = str(d["family"])
        d["block"] = int(d["block"])
        d["amount"] = float(d["amount"])
        if "ridx_flat" in d:
            cuts = np.cumsum(np.concatenate([[0], d["ridx_counts"]])).astype(int)
            d["ridx"] = [d["ridx_flat"][cuts[j]:cuts[j + 1]] for j in range(len(cuts) - 1)]
        if "coords_flat" in d:
            cuts = np.cumsum(np.concatenate([[0], d["coords_counts"]])).astype(int)
            d["coords"] = [d["coords_flat"][cuts[j]:cuts[j + 1]].tolist() for j in range(len(cuts) - 1)]
        cases.append((i, d))
    return cases
