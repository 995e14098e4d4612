// tri_tile_check.cpp -- the folded upper triangle of a self-join (kpop_amd/csrc/tri_tile.h) on its own, with a host compiler alone:
//   c++ -std=c++17 -O1 -o tri_tile_check tools/probes/src/tri_tile_check.cpp && ./tri_tile_check
// For n_rt = 1 .. 12 row tiles, both tile shapes and every by_first, every block (bx, y) of tri_grid is asked for its tile: each tile
// (bx, by) with by >= by_first and bx < (by + 1) kf must be owned by exactly one block and no block may own anything else; with the
// last row tile ragged or full, `live` must be false exactly for the owned tiles with i0 + 1 >= j1 (and for the blocks that own none).
// Prints one line a shape, "... bad 0" when all is well; the exit status is the number of bad findings (capped).
#include <stdio.h>

#include <vector>

#include "../../../kpop_amd/csrc/tri_tile.h"

using namespace kpop;

int main() {
  long total_bad = 0;
  for (uint32_t r1_shape : {1000u, 70000u}) {  // 64 x 64 (kf = 1) and 32 x 256 (kf = 8)
    const SelfShape s = self_shape(r1_shape);
    long bad = 0, blocks = 0, tiles = 0;
    if (s.TJ != s.TY * s.n_rg || s.kf * s.w != s.TJ || s.n_cg * s.n_rg != 256 || s.n_cg * 4 != s.w) ++bad;
    for (uint32_t n_rt = 1; n_rt <= 12; ++n_rt)
      for (uint32_t by_first = 0; by_first < n_rt; ++by_first)
        for (uint32_t r1 : {n_rt * s.TJ - s.TJ + 1, n_rt * s.TJ}) {
          const uint32_t n_act = n_rt - by_first;
          const TriGrid g = tri_grid(n_rt, by_first, s.kf);
          std::vector<int> owners((size_t)n_rt * n_rt * s.kf, 0);  // [by][bx]
          for (uint32_t y = 0; y < g.lines; ++y)
            for (uint32_t bx = 0; bx < g.gx; ++bx) {
              const TriTile t = tri_tile(bx, y, s.w, s.TJ, s.kf, by_first, n_act, r1);
              ++blocks;
              if (t.bx >= (t.by + 1) * s.kf) {  // the block owns no tile: only the second half of the middle line of an odd count
                if (t.live || !(n_act % 2 == 1 && y == n_act / 2 && bx >= (by_first + y + 1) * s.kf)) ++bad;
                continue;
              }
              if (t.by < by_first || t.by >= n_rt) {
                ++bad;
                continue;
              }
              ++owners[(size_t)t.by * n_rt * s.kf + t.bx];
              const uint32_t j1 = (t.by + 1) * s.TJ < r1 ? (t.by + 1) * s.TJ : r1, i1 = (t.bx + 1) * s.w < r1 ? (t.bx + 1) * s.w : r1;
              if (t.i0 != t.bx * s.w || t.j0 != t.by * s.TJ || t.j1 != j1 || t.i1 != i1) ++bad;
              if (t.live != !(t.i0 + 1 >= t.j1)) ++bad;
            }
          for (uint32_t by = 0; by < n_rt; ++by)
            for (uint32_t bx = 0; bx < n_rt * s.kf; ++bx) {
              const int want = (by >= by_first && bx < (by + 1) * s.kf) ? 1 : 0;
              tiles += want;
              if (owners[(size_t)by * n_rt * s.kf + bx] != want) ++bad;
            }
        }
    printf("shape %u x %u (kf %u): %ld blocks, %ld tiles, bad %ld\n", s.w, s.TJ, s.kf, blocks, tiles, bad);
    total_bad += bad;
  }
  return total_bad > 100 ? 100 : (int)total_bad;
}
