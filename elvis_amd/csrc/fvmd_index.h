// Index arithmetic of the FVMD kernels (fvmd.hip), host and device: the mirror of the pyramid filter, the level sizes,
// the segment count, the grid-slot -> keypoint map, the window offsets and the round-robin pairing of the Jacobi sweeps.
// tools/fvmd_index_check.cpp walks every one of them on the host over the shapes the entry points admit.
#pragma once

#if defined(__HIPCC__)
#define FVMD_HD __host__ __device__ __forceinline__
#else
#define FVMD_HD static inline
#endif

#define FVMD_MIN_SIDE 64
#define FVMD_GRID 20                 // keypoints per side
#define FVMD_POINTS 400
#define FVMD_LEVELS 3
#define FVMD_RADIUS 7
#define FVMD_WIN 15
#define FVMD_WIN_PIXELS 225
#define FVMD_CELLS 4                 // histogram cells per side, 5 x 5 keypoints each
#define FVMD_CELL_SIDE 5
#define FVMD_BINS 8
#define FVMD_FIELD_VALUES 128        // 16 cells x 8 bins
#define FVMD_MIN_SEQ 10
#define FVMD_MAX_SEQ 16
#define FVMD_MAX_ROWS 1024           // the most feature rows (segments) of one clip a Frechet distance takes
#define FVMD_LDS_DOUBLES 16384       // k * len up to which the Jacobi sweeps run in one workgroup's LDS (128 KB)

// mirror without repeating the edge, one fold at each end: valid for -n < i < 2n - 1
FVMD_HD int fvmd_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * n - 2 - i : i;
}

// side of pyramid level l (level l + 1 keeps the even indices of level l)
FVMD_HD int fvmd_level_size(int n, int level) {
    for (int l = 0; l < level; ++l) n = (n + 1) / 2;
    return n;
}

// sliding segments of seq_len frames starting every step frames; 0 when the clip is shorter than one segment
FVMD_HD int fvmd_segments(int frames, int seq_len, int step) { return frames < seq_len ? 0 : (frames - seq_len) / step + 1; }

// grid slot q (neighbouring waves) -> keypoint index i * 20 + j: the 25 points of a histogram cell are 25 neighbouring slots
FVMD_HD int fvmd_point_of_slot(int q) {
    const int cell = q / (FVMD_CELL_SIDE * FVMD_CELL_SIDE), in = q % (FVMD_CELL_SIDE * FVMD_CELL_SIDE);
    const int i = (cell / FVMD_CELLS) * FVMD_CELL_SIDE + in / FVMD_CELL_SIDE, j = (cell % FVMD_CELLS) * FVMD_CELL_SIDE + in % FVMD_CELL_SIDE;
    return i * FVMD_GRID + j;
}

// keypoint a (0..24) of histogram cell c (0..15), in the order the cell is summed
FVMD_HD int fvmd_cell_point(int c, int a) {
    return ((c / FVMD_CELLS) * FVMD_CELL_SIDE + a / FVMD_CELL_SIDE) * FVMD_GRID + (c % FVMD_CELLS) * FVMD_CELL_SIDE + a % FVMD_CELL_SIDE;
}

// round-robin pairing of K (even) vectors: round r in [0, K - 1), pair p in [0, K / 2); every vector is in one pair of a
// round and every two vectors meet once per sweep.  With an odd count the caller rounds K up and skips index K - 1.
FVMD_HD void fvmd_pair(int r, int p, int K, int* i, int* j) {
    const int m = K - 1;
    if (p == 0) {
        *i = m;
        *j = r;
    } else {
        *i = (r + p) % m;
        *j = (r - p + m) % m;
    }
}
