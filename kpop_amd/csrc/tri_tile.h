// tri_tile.h -- the tiles of a self-join as plain integer arithmetic: the two tile shapes, and which tile of the folded upper triangle
// a block owns.  Nothing of HIP is included: a host compiler alone builds and tests this file (tools/probes/src/tri_tile_check.cpp);
// self_tile.h puts the kernels' pieces on top of it.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define KPOP_TRI_FN __host__ __device__ inline
#else
#define KPOP_TRI_FN inline
#endif

namespace kpop {

// A tile is w columns (rows i of the set) x TJ = TY n_rg rows (rows j), TJ = kf w; a thread 4 columns x TY rows, n_cg threads a row and
// n_rg row groups: n_cg n_rg = 256, every thread of a workgroup holds pairs.  32 x 256 with a thread 4 x 8 for a long set, so that it is
// read from HBM once per 256 rows; 64 x 64 with a thread 4 x 4 below.  (The choice moves no bit: a pair's chain is one thread's either way.)
struct SelfShape {
  uint32_t w, n_cg, n_rg, TY, TJ, kf;
};

KPOP_TRI_FN SelfShape self_shape(uint32_t r1) {
  SelfShape s;
  s.TY = r1 >= 65536 ? 8 : 4;
  s.w = s.TY == 8 ? 32 : 64;
  s.n_cg = s.w / 4;
  s.n_rg = 256 / s.n_cg;
  s.TJ = s.TY * s.n_rg;
  s.kf = s.TJ / s.w;
  return s;
}

// Row tile `by` of n_rt needs the column tiles 0 .. (by + 1) kf - 1 (those with a column below its last row).  The n_act row tiles
// from by_first on are folded, the y-th with the y-th from the end, so that every line of the grid holds the same number of tiles and
// no block is launched for the lower triangle: `lines` lines of gx blocks.
struct TriGrid {
  uint32_t gx, lines;
};

KPOP_TRI_FN TriGrid tri_grid(uint32_t n_rt, uint32_t by_first, uint32_t kf) {
  const uint32_t n_act = n_rt - by_first;
  return TriGrid{(2 * by_first + n_act + 1) * kf, (n_act + 1) / 2};  // gx: the tiles of a row tile and of its partner from the end
}

// Column tile bx of row tile by: columns i0 .. i1, rows j0 .. j1 of the set's r1.  live: the block has pairs to compute.  It has none
// in the second half of the middle line of an odd number of row tiles (the line's own row tile is computed once: bx stays beyond the
// row tile's (by + 1) kf column tiles, the bounds are empty), and none where the ragged last row tile leaves no column below its last row
struct TriTile {
  uint32_t bx, by, i0, i1, j0, j1;
  bool live;
};

KPOP_TRI_FN TriTile tri_tile(uint32_t bx, uint32_t y, uint32_t w, uint32_t TJ, uint32_t kf, uint32_t by_first, uint32_t n_act, uint32_t r1) {
  TriTile t{bx, by_first + y, 0, 0, 0, 0, false};
  const uint32_t by_hi = by_first + n_act - 1 - y, n_lo = (t.by + 1) * kf;
  if (bx >= n_lo) {
    if (by_hi == t.by) return t;
    t.bx = bx - n_lo;
    t.by = by_hi;
  }
  t.i0 = t.bx * w;
  t.j0 = t.by * TJ;
  t.j1 = t.j0 + TJ < r1 ? t.j0 + TJ : r1;
  t.i1 = t.i0 + w < r1 ? t.i0 + w : r1;
  t.live = t.i0 + 1 < t.j1;
  return t;
}

}  // namespace kpop
