"""csrc/vq_index.hip restated on the CPU - the index build and the shell search, float32 with one rounding per operation -
with mutants, and the cases tests/test_gpu_vq_indexed.py and tests/test_vq_grid_host.py share.

`search` follows the kernel's visiting order (own cell, then Chebyshev shells; rows i, j ascending; on rows inside the
shell's hull the two end cells, elsewhere the row's cells k0 .. k1) and its stop rule, and returns per pixel

    idx     the code it settles on (SENTINEL where it saw none),
    shells  how many shells it walked (r = 0 counts as one),
    late    whether the winner was visited AFTER a rival at the same rounded distance - the only situation the clause
            `id < best_i` of the kernel exists for.

Mutants, by what they can change.  Three change the index on their named case:
    tie_keeps_first_seen    drops `id < best_i`: among equal distances the code visited first stays
    stop_after_first_hit    stops after the first shell that gave any code
    interior_rows_one_end   scans only the upper end cell (kb) of a row inside the hull
One changes the index only for pixels outside the codebook's box:
    pixel_cell_by_division  floor((p - lo) / width) instead of counting edges: not clamped to the grid, so a pixel beyond
                            the box searches cells that do not exist and finds nothing
And one cannot change the index at all, only the cost:
    bound_ignores_shell     the gap to the faces of the pixel's own cell at every r.  That gap is never larger than the
                            gap to the searched cube's faces, so the search only stops later: the named case pins the
                            shells walked.  (A pixel's cell being off the mark is harmless in the same way: gaps are
                            clamped at 0, so a face the pixel lies beyond keeps the search going.)
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple

import numpy as np

F32 = np.float32
VQG_MAX = 16
SENTINEL = 0x7FFFFFFF
BIG = F32(3.0e38)
SLACK = F32(0.99999)
MUTANTS = ("tie_keeps_first_seen", "stop_after_first_hit", "interior_rows_one_end", "pixel_cell_by_division", "bound_ignores_shell")

# literal text of csrc/vq_index.hip that this module restates
SOURCE_TEXT = (
    "constexpr int VQG_MAX = 16;",
    "int g = (int)lround(cbrt((double)n_embed / 2.0));",
    "for (int j = 1; j < g; ++j) i += x >= e[j] ? 1 : 0;",
    "float v = i >= G ? hi : (float)((double)lo + ((double)hi - (double)lo) * i / G);",
    "if (d < best || (d == best && id < best_i && best_i != VQG_SENTINEL)) {",
    "if (abs(i - ci[0]) < r && abs(j - ci[1]) < r) {",
    "if (ka >= 0) scan(start[row + ka], start[row + ka + 1]);",
    "if (kb < G) scan(start[row + kb], start[row + kb + 1]);",
    "scan(start[row + k0], start[row + k1 + 1]);",
    "const int a = ci[d] - r, b = ci[d] + r + 1;",
    "if (!open || __fmul_rn(lb, 0.99999f) > best) break;",
    "float best = 3.0e38f;",
    "if (idx_out) idx_out[px] = best_i;",
    "for (int k = 3; k < pitch_out; ++k) o[k] = from_f<T>(0.f);",
)


# ============================================================================================ the index
def grid_cells(n_embed: int) -> int:
    g = int(math.floor(float(np.cbrt(n_embed / 2.0)) + 0.5))          # lround of a positive value
    return max(1, min(VQG_MAX, g))


def axis_cell(e: np.ndarray, g: int, x) -> int:
    return int(np.count_nonzero(F32(x) >= e[1:g]))


@dataclass
class Index:
    G: int
    edges: np.ndarray        # float32 [3, 17]
    start: np.ndarray        # int64 [G^3 + 1]
    ent: np.ndarray          # float32 [K, 3] in CSR order
    ids: np.ndarray          # int64 [K]


def build(cb: np.ndarray) -> Index:
    cb = np.asarray(cb, F32)
    k = cb.shape[0]
    g = grid_cells(k)
    edges = np.zeros((3, VQG_MAX + 1), F32)
    for d in range(3):
        lo, hi = cb[:, d].min(), cb[:, d].max()
        e = edges[d]
        for i in range(VQG_MAX + 1):
            v = hi if i >= g else F32(float(lo) + (float(hi) - float(lo)) * i / g)
            if i > 0 and v < e[i - 1]:
                v = e[i - 1]
            e[i] = min(v, hi)
        e[0] = lo
    cell = np.zeros(k, np.int64)
    for d in range(3):
        cell = cell * g + (cb[:, d][:, None] >= edges[d][None, 1:g]).sum(1)
    order = np.argsort(cell, kind="stable")                            # ascending id inside a cell
    start = np.zeros(g ** 3 + 1, np.int64)
    np.add.at(start, cell + 1, 1)
    return Index(g, edges, np.cumsum(start), cb[order], order.astype(np.int64))


# ============================================================================================ the search
def _pixel_cells(ix: Index, p: np.ndarray, mutant: Optional[str]):
    if mutant != "pixel_cell_by_division":
        return [axis_cell(ix.edges[d], ix.G, p[d]) for d in range(3)]
    out = []
    with np.errstate(all="ignore"):
        for d in range(3):
            lo, hi = ix.edges[d][0], ix.edges[d][ix.G]
            q = np.floor(F32(F32(p[d] - lo) / F32(F32(hi - lo) / F32(ix.G))))
            out.append(0 if np.isnan(q) else int(np.clip(q, -(1 << 20), 1 << 20)))
    return out


def search_pixel(ix: Index, p: np.ndarray, mutant: Optional[str] = None) -> Tuple[int, int, bool]:
    G, edges, start = ix.G, ix.edges, ix.start
    p = np.asarray(p, F32)
    ci = _pixel_cells(ix, p, mutant)
    best, best_i, best_pos, late = BIG, SENTINEL, -1, False
    pos = 0
    shells = 0

    def scan(e0: int, e1: int):
        nonlocal best, best_i, best_pos, late, pos
        if e1 <= e0:
            return
        q = ix.ent[e0:e1]
        dx, dy, dz = p[0] - q[:, 0], p[1] - q[:, 1], p[2] - q[:, 2]
        d = (dx * dx + dy * dy) + dz * dz                               # float32 arrays: one rounding per operation
        ids = ix.ids[e0:e1]
        ok = d < BIG
        if ok.any():
            dm = d[ok].min()
            at = np.flatnonzero(ok & (d == dm))                         # in visiting order
            w = at[0] if mutant == "tie_keeps_first_seen" else at[np.argmin(ids[at])]
            if dm < best:
                best, best_i, best_pos, late = dm, int(ids[w]), pos + int(w), bool(w != at[0])
            elif dm == best and best_i != SENTINEL and mutant != "tie_keeps_first_seen" and int(ids[w]) < best_i:
                best_i, best_pos, late = int(ids[w]), pos + int(w), True
        pos += e1 - e0

    for r in range(G):
        shells = r + 1
        i0, i1 = max(ci[0] - r, 0), min(ci[0] + r, G - 1)
        j0, j1 = max(ci[1] - r, 0), min(ci[1] + r, G - 1)
        k0, k1 = max(ci[2] - r, 0), min(ci[2] + r, G - 1)
        for i in range(i0, i1 + 1):
            for j in range(j0, j1 + 1):
                row = (i * G + j) * G
                if abs(i - ci[0]) < r and abs(j - ci[1]) < r:
                    ka, kb = ci[2] - r, ci[2] + r
                    if 0 <= ka < G and mutant != "interior_rows_one_end":
                        scan(start[row + ka], start[row + ka + 1])
                    if 0 <= kb < G:
                        scan(start[row + kb], start[row + kb + 1])
                elif k0 <= k1:
                    scan(start[row + k0], start[row + k1 + 1])
        if mutant == "stop_after_first_hit" and best_i != SENTINEL:
            break
        lb, is_open = F32(np.inf), False
        for d in range(3):
            a, b = (ci[d], ci[d] + 1) if mutant == "bound_ignores_shell" else (ci[d] - r, ci[d] + r + 1)
            if a >= 1:
                g = max(F32(p[d] - edges[d][min(a, VQG_MAX)]), F32(0))
                lb, is_open = min(lb, F32(g * g)), True
            if b <= G - 1:
                g = max(F32(edges[d][max(b, 0)] - p[d]), F32(0))
                lb, is_open = min(lb, F32(g * g)), True
        if not is_open or F32(lb * SLACK) > best:
            break
    return best_i, shells, late


def search(cb: np.ndarray, z: np.ndarray, mutant: Optional[str] = None, index: Optional[Index] = None):
    """(idx int64 [P], shells int64 [P], late bool [P]) for pixels z [P, 3] float32."""
    assert mutant is None or mutant in MUTANTS, mutant
    ix = build(cb) if index is None else index
    z = np.asarray(z, F32)
    out = [search_pixel(ix, z[i], mutant) for i in range(z.shape[0])]
    return (np.array([o[0] for o in out], np.int64), np.array([o[1] for o in out], np.int64), np.array([o[2] for o in out], bool))


# ============================================================================================ the cases
@dataclass(frozen=True)
class Case:
    id: str
    make: Callable[[np.random.Generator], Tuple[np.ndarray, np.ndarray]]      # -> (codebook [K, 3], pixels [P, 3]) float32

    def arrays(self) -> Tuple[np.ndarray, np.ndarray]:
        if self.id not in _ARRAYS:
            cb, z = self.make(np.random.default_rng([len(self.id)] + [ord(ch) for ch in self.id]))
            # values both storage types hold exactly: the f16 run then works on the very same numbers
            cb, z = np.ascontiguousarray(cb, F32), np.ascontiguousarray(z, F32).astype(np.float16).astype(F32)
            cb.setflags(write=False)
            z.setflags(write=False)
            _ARRAYS[self.id] = (cb, z)
        return _ARRAYS[self.id]


_ARRAYS: Dict[str, Tuple[np.ndarray, np.ndarray]] = {}


def _random(k, p, spread=1.2):
    return lambda rng: (rng.standard_normal((k, 3)), rng.standard_normal((p, 3)) * spread)


def _constant(axes, k=300, p=257, value=0.375):
    """A codebook constant on `axes`; pixels below, on and above the constant on those axes, anything elsewhere."""
    def make(rng):
        cb = rng.standard_normal((k, 3))
        cb[:, list(axes)] = value
        z = rng.standard_normal((p, 3)) * 1.5
        for a in axes:
            z[:, a] = rng.choice([value - 1.0, value - 2.0 ** -10, value, value + 2.0 ** -10, value + 1.0], p)
        return cb, z
    return make


def _mirrored_winner_seen_later(rng):
    """Pairs (b, a, t), (a, b, t) with b > a: the FIRST of a pair, which must win every tie on the diagonal, lies in the
    cell row with the larger i and is visited after its rival (rows are walked with i ascending).  The set of codes is
    symmetric in x and y, so both axes have the same edges and a pair's two cells lie in the same shell of a diagonal
    pixel."""
    ab = rng.standard_normal((64, 3)).astype(np.float16).astype(F32)
    hi, lo = np.maximum(ab[:, 0], ab[:, 1]), np.minimum(ab[:, 0], ab[:, 1])
    pairs = np.empty((128, 3), F32)
    pairs[0::2] = np.stack([hi, lo, ab[:, 2]], 1)
    pairs[1::2] = np.stack([lo, hi, ab[:, 2]], 1)
    s = rng.standard_normal((300, 2))
    return pairs, np.stack([s[:, 0], s[:, 0], s[:, 1]], 1)


def _cluster_and_corners(rng):
    """Two corner codes span the grid and a tight cluster fills one cell: most pixels stand in an empty cell and walk
    several shells."""
    cb = np.concatenate([[[-4.0, -4.0, -4.0]], 0.3 + rng.standard_normal((254, 3)) * 1e-3, [[4.0, 4.0, 4.0]]])
    return cb, np.concatenate([rng.standard_normal((150, 3)) * 3, 0.3 + rng.standard_normal((107, 3)) * 2e-3])


def _far_outside(rng):
    cb = rng.standard_normal((2000, 3))
    z = rng.standard_normal((257, 3)) * 1.0e3
    z[200:, 0] = rng.standard_normal(57)                                # outside on two axes only
    return cb, z


CASES = (
    Case("k6_one_cell", _random(6, 257)), Case("k7_two_cells", _random(7, 257)),
    Case("k16384_grid_capped", _random(16384, 1025)), Case("k20000_grid_capped", _random(20000, 600)),
    Case("constant_z", _constant((2,))), Case("constant_yz", _constant((1, 2))), Case("all_identical", _constant((0, 1, 2))),
    Case("p255", _random(257, 255)), Case("p256", _random(257, 256)), Case("p257", _random(257, 257)),
    Case("random_2000", _random(2000, 600, 1.5)), Case("mirrored_winner_seen_later", _mirrored_winner_seen_later),
    Case("cluster_and_corners", _cluster_and_corners), Case("far_outside", _far_outside),
)
BY_ID = {c.id: c for c in CASES}
MAX_CODES, MAX_PIXELS = 20000, 1100

# mutant -> (case, what it changes there)
MUTANT_CASES = {"tie_keeps_first_seen": ("mirrored_winner_seen_later", "idx"), "stop_after_first_hit": ("random_2000", "idx"),
                "interior_rows_one_end": ("random_2000", "idx"), "pixel_cell_by_division": ("far_outside", "idx"),
                "bound_ignores_shell": ("random_2000", "shells")}
