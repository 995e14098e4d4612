// forest.hip -- the single-linkage tree of a resident set: its minimum spanning forest.
//
//   The graph of clusters.hip: the set's r1 rows, i < j joined iff d(j, i) <= max_distance, d the reference chain's distance
//   (lib/Space.ml:182-205 with the adaptors of lib/Matrix.ml:243-250), symmetric bit for bit, a NaN no edge; no kpop_tune setting is
//   read.  Edges are ordered by (d with -0 taken as +0, i, j) ascending: a STRICT total order, under which the minimum spanning
//   forest is unique -- the result is defined without reference to an algorithm and is the same bits on every run.
//
// Boruvka rounds over the implicit complete graph; neither a matrix nor a neighbour list is formed.  A round:
//   forest_tile_labels_kernel  per tile of w rows: the label its rows share, or "mixed" -- a tile of the pass below whose rows and
//                              columns all carry one label holds no foreign pair and is skipped (the late rounds are mostly that)
//   forest_nearest_kernel      per row, the least allowed edge to a row of ANOTHER component.  The self-join's tile shapes
//                              (tri_tile.h) and the loop of pair_tile.h: a pair's bits are the chain's.  A
//                              workgroup owns a strip of TJ rows and walks the column tiles of its segment of the set, columns
//                              ascending; every thread keeps the best (key, column) of its TY rows in registers, the lanes of a
//                              row reduce with shuffles (self_tile.h), one store a row and segment.  For a fixed row r
//                              the order of the edges {r, c} is (d, c): whichever side of r the columns lie on, (min, max) ascends
//                              with c.  Each pair is computed twice (once from either end); the key is 96 bits, which no atomic of
//                              gfx950 holds, and this shape needs none
//   forest_row_min_kernel      the least of a row's segments; atomicMin of its key onto the row's component (a distance's key: its
//                              bits mapped so that doubles order as unsigned integers, negative ones included)
//   forest_comp_edge_kernel    among the rows that hold their component's least key: atomicMin of (i << 32 | j), i < j
//   forest_link_kernel         a component emits its edge unless the component at the other end chose the SAME edge and has the
//                              smaller label (the edge is then emitted once, by that one), and unites with the other end: the
//                              lock-free union of union_find.h, the larger root hooked under the smaller with one compare-and-swap
//   forest_flatten_kernel      labels[i] = the root of i, the smallest index of its component: section 6d's labels when the rounds end
// No cycle can form: under a strict total order the least edge that leaves a component belongs to THE minimum spanning forest (the
// cut property, without ties to break), so every edge emitted in any round is an edge of that one forest, and a subset of a forest
// holds no cycle; the only edge two components can both choose is the same edge, which is emitted once.
// Components that can still merge at least halve a round, so ceil(log2 r1) rounds always suffice.  The device form enqueues that
// many; every kernel of a round returns at once when the word of the round before says that it added no edge -- nothing is read
// back.  The host form reads the word and stops.  Edges arrive in any order; they are sorted on the device by (d, i, j): two stable
// radix sorts (radix_sort.h), the pair first, the distance's key second.
// The tile loop is pair_tile.h's, the shapes and the lanes' reduction self_tile.h's, the union union_find.h's, the distance's key
// space_ops.h's.
//
// The rounds under another weight.  forest_nearest_kernel takes what an edge weighs as a policy: ForestDistanceWeight, the distance
// (an empty struct that compiles away: the kernel above), or ForestReachWeight, max(d, core_i, core_j) over per-row core distances --
// the mutual-reachability forest of reachability.hip, which calls forest_dev through forest_rounds.h.  Nothing else of a round knows
// what a key stands for, and the two claims the rounds rest on hold for any symmetric weight wt(r, c) that is a function of the
// unordered pair alone (both checked again for the second policy):
//   * for a fixed row r the edges {r, c} order by (wt, c): the order is (wt, min, max), and (min(r, c), max(r, c)) ascends with c
//     whichever side of r the columns lie on (every c < r gives (c, r), below every (r, c') with c' > r) -- no property of wt is used;
//   * a tile whose rows and columns all carry one label is skipped because it holds no pair of two components, whatever a pair weighs.
// Weights tie far more often there (every edge out of row i within core_i weighs at least core_i); the strict order makes that harmless.
#include <algorithm>

#include "common.h"
#include "distance_routes.h"
#include "forest_rounds.h"
#include "radix_sort.h"
#include "refset_call.h"
#include "self_tile.h"

namespace kpop {

constexpr int kFMaxW = 64, kFMaxTJ = 256, kFMaxSeg = 8, kFMaxRounds = 32;
constexpr uint32_t kFMixed = 0xFFFFFFFFu;  // (no label: labels are row indices, below r1 <= 2^32 - 1)
constexpr uint64_t kFNone = ~0ull;         // (no key: distance_key maps only a NaN's bits there, and a NaN is never a key)

#define FOREST_GATE() \
  if (gate && *gate == 0) return  // the round before added no edge: the forest is complete

__global__ __launch_bounds__(256) void forest_init_kernel(uint32_t *__restrict__ lab, uint32_t *__restrict__ par, uint64_t *__restrict__ comp_k,
                                                          uint64_t *__restrict__ comp_e, uint64_t *__restrict__ out_k, uint64_t *__restrict__ out_e, uint32_t r1,
                                                          uint32_t m) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) {
    lab[i] = (uint32_t)i;
    par[i] = (uint32_t)i;
    comp_k[i] = kFNone;
    comp_e[i] = kFNone;
    if (i < m) {
      out_k[i] = kFNone;  // (a slot no edge takes sorts behind every edge)
      out_e[i] = kFNone;
    }
  }
}

__global__ __launch_bounds__(256) void forest_tile_labels_kernel(const uint32_t *__restrict__ lab, uint32_t r1, uint32_t w, uint32_t n_ct,
                                                                 uint32_t *__restrict__ tile_lab, const uint32_t *gate) {
  FOREST_GATE();
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < n_ct; t += (uint64_t)gridDim.x * 256) {
    const uint64_t i0 = t * w, i1 = (i0 + w < r1) ? i0 + w : (uint64_t)r1;
    uint32_t l = lab[i0];
    for (uint64_t i = i0 + 1; i < i1; ++i)
      if (lab[i] != l) {
        l = kFMixed;
        break;
      }
    tile_lab[t] = l;
  }
}

// What an edge weighs.  The single-linkage tree: the distance -- every call folds away.  The mutual-reachability forest
// (reachability.hip): max(d, core_i, core_j), core the rows' core distances; a thread holds its rows' for the launch and the tile's
// four columns' for the tile.  weight(yy, x, d): the weight of the pair of the thread's yy-th row and x-th column, a NaN when it is
// no edge -- tested value by value, because fmax drops a NaN operand instead of handing it on
struct ForestDistanceWeight {
  __device__ __forceinline__ void rows(const double *, uint32_t, uint32_t) {}
  __device__ __forceinline__ void columns(const double *, uint32_t, uint32_t) {}
  __device__ __forceinline__ double weight(int, int, double d) const { return d; }
};
template <int TY>
struct ForestReachWeight {
  double own[TY], col[4];
  __device__ __forceinline__ void rows(const double *core, uint32_t jfirst, uint32_t j1) {
#pragma unroll
    for (int yy = 0; yy < TY; ++yy) own[yy] = jfirst + yy < j1 ? core[jfirst + yy] : 0.0;
  }
  __device__ __forceinline__ void columns(const double *core, uint32_t ifirst, uint32_t i1) {
#pragma unroll
    for (int x = 0; x < 4; ++x) col[x] = ifirst + x < i1 ? core[ifirst + x] : 0.0;
  }
  __device__ __forceinline__ double weight(int yy, int x, double d) const {
    if (d != d || own[yy] != own[yy] || col[x] != col[x]) return __longlong_as_double(0x7FF8000000000000ll);
    return fmax(fmax(d, col[x]), own[yy]);
  }
};

// a: the set's rows as the chain reads them (divided by their norms when the set normalises), both operands.  Strip blockIdx.x:
// rows j0 .. j0 + TJ, TJ = TY n_rg = kf w; segment blockIdx.y: the column tiles (w rows of the set each) t_begin .. t_end.  A thread
// 4 columns x TY rows, the dimensions ascending in one thread, 16 at a time through LDS (pair_tile.h).  The next step's
// operands -- the tile's next 16 dimensions, or the first of the next tile that is not skipped -- are loaded under the arithmetic.
// core: the rows' core distances, read by ForestReachWeight alone
template <int KIND, int TY, class Weight>
__global__ __launch_bounds__(256, 1) void forest_nearest_kernel(const double *__restrict__ a, uint32_t w, uint32_t r1, uint32_t n_dims,
                                                                const double *__restrict__ metric, double p, double max_distance, uint32_t n_cg,
                                                                uint32_t n_rg, uint32_t kf, uint32_t n_ct, uint32_t tiles_per_seg,
                                                                const uint32_t *__restrict__ lab, const uint32_t *__restrict__ tile_lab,
                                                                uint64_t *__restrict__ part_k, uint32_t *__restrict__ part_c, const uint32_t *gate,
                                                                const double *__restrict__ core) {
  FOREST_GATE();
  __shared__ __attribute__((aligned(16))) double As[kPairDC][kFMaxW + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][kFMaxTJ + 2];
  __shared__ double s_metric[kPairDC];
  const uint32_t TJ = TY * n_rg;
  const uint32_t strip = blockIdx.x, seg = blockIdx.y;
  const uint32_t j0 = strip * TJ, j1 = min(r1, j0 + TJ);  // (the grid has div_up(r1, TJ) strips: j0 < r1)
  const uint32_t t_begin = min(n_ct, seg * tiles_per_seg), t_end = min(n_ct, t_begin + tiles_per_seg);
  // the label all rows of the strip share, if they do
  uint32_t strip_lab = tile_lab[strip * kf];
  for (uint32_t q = 1; q < kf; ++q)
    if (strip * kf + q < n_ct && tile_lab[strip * kf + q] != strip_lab) strip_lab = kFMixed;
  struct Tile : PairTile {
    uint32_t t;
  };
  auto tile_from = [&](uint32_t t) {  // the first tile from t on that holds a foreign pair (the same for every thread); empty at t_end
    while (t < t_end && strip_lab != kFMixed && tile_lab[t] == strip_lab) ++t;
    return Tile{{t * w, t < t_end ? min(r1, t * w + w) : 0u}, t};
  };
  const uint32_t cg = threadIdx.x % n_cg, rg = threadIdx.x / n_cg;
  const bool worker = rg < n_rg;
  const uint32_t ti = cg * 4, tj = (worker ? rg : 0) * TY;
  uint32_t lj[TY], best_c[TY];
  uint64_t best_k[TY];
#pragma unroll
  for (int yy = 0; yy < TY; ++yy) {
    lj[yy] = (j0 + tj + yy < j1) ? lab[j0 + tj + yy] : 0u;
    best_k[yy] = kFNone;
    best_c[yy] = 0u;
  }
  Weight wt;
  wt.rows(core, j0 + tj, j1);
  const PairRows rows{a, r1};
  PairStage<kFMaxW, kFMaxTJ> stage;
  Tile cur = tile_from(t_begin), nxt;
  for (pair_sweep_open(stage, rows, cur, rows, j0, j1, n_dims); cur.i0 < cur.i1; cur = nxt) {
    nxt = tile_from(cur.t + 1);
    const uint32_t i0 = cur.i0, i1 = cur.i1;
    uint32_t li[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) li[x] = (i0 + ti + x < i1) ? lab[i0 + ti + x] : 0u;
    wt.columns(core, i0 + ti, i1);
    double acc[TY][4];
    pair_sweep_tile<KIND>(stage, acc, As, Bs, s_metric, rows, cur, nxt, rows, j0, j1, n_dims, metric, p, ti, tj, worker);
    // the epilogue: the pair's weight against the bound (a NaN compares false: no edge), a row of another component only
    // (which the row itself never is); columns ascend within the tile and from tile to tile, so that `below` alone keeps, among
    // equal keys, the least column
    if (worker) {
#pragma unroll
      for (int yy = 0; yy < TY; ++yy)
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const double d = wt.weight(yy, x, scale_distance<KIND>(acc[yy][x], p));
          const uint32_t i = i0 + ti + x, j = j0 + tj + yy;
          if (j < j1 && i < i1 && li[x] != lj[yy] && d <= max_distance) {
            const uint64_t key = distance_key(d);
            if (key < best_k[yy]) {
              best_k[yy] = key;
              best_c[yy] = i;
            }
          }
        }
    }
  }
  // the least (key, column) over a row's lanes
#pragma unroll
  for (int yy = 0; yy < TY; ++yy) {
    const KeyAt best = reduce_row_lanes(KeyAt{best_k[yy], best_c[yy]}, n_cg, key_at_min);
    const uint32_t j = j0 + tj + yy;
    if (worker && cg == 0 && j < j1) {
      part_k[(uint64_t)seg * r1 + j] = best.k;
      part_c[(uint64_t)seg * r1 + j] = best.c;
    }
  }
}

// the segments hold ascending columns: among equal keys the first segment's
__global__ __launch_bounds__(256) void forest_row_min_kernel(uint64_t *__restrict__ part_k, uint32_t *__restrict__ part_c, uint32_t n_seg, uint32_t r1,
                                                             const uint32_t *__restrict__ lab, uint64_t *comp_k, const uint32_t *gate) {
  FOREST_GATE();
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < r1; r += (uint64_t)gridDim.x * 256) {
    uint64_t k = part_k[r];
    uint32_t c = part_c[r];
    for (uint32_t s = 1; s < n_seg; ++s) {
      const uint64_t kk = part_k[(uint64_t)s * r1 + r];
      if (kk < k) {
        k = kk;
        c = part_c[(uint64_t)s * r1 + r];
      }
    }
    part_k[r] = k;
    part_c[r] = c;
    if (k != kFNone) atomicMin((unsigned long long *)(comp_k + lab[r]), (unsigned long long)k);
  }
}

__global__ __launch_bounds__(256) void forest_comp_edge_kernel(const uint64_t *__restrict__ part_k, const uint32_t *__restrict__ part_c, uint32_t r1,
                                                               const uint32_t *__restrict__ lab, const uint64_t *__restrict__ comp_k, uint64_t *comp_e,
                                                               const uint32_t *gate) {
  FOREST_GATE();
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < r1; r += (uint64_t)gridDim.x * 256) {
    const uint64_t k = part_k[r];
    if (k == kFNone || k != comp_k[lab[r]]) continue;
    const uint32_t c = part_c[r], lo = min((uint32_t)r, c), hi = max((uint32_t)r, c);
    atomicMin((unsigned long long *)(comp_e + lab[r]), ((unsigned long long)lo << 32) | hi);
  }
}

// lab, comp_k, comp_e: the round's, read only here; the unions go into par
__global__ __launch_bounds__(256) void forest_link_kernel(const uint32_t *__restrict__ lab, const uint64_t *__restrict__ comp_k,
                                                          const uint64_t *__restrict__ comp_e, uint32_t r1, uint32_t m, uint32_t *par, uint32_t *n_edges,
                                                          uint64_t *__restrict__ out_k, uint64_t *__restrict__ out_e, uint32_t *added, const uint32_t *gate) {
  FOREST_GATE();
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < r1; r += (uint64_t)gridDim.x * 256) {
    const uint32_t R = (uint32_t)r;
    if (lab[R] != R) continue;
    const uint64_t k = comp_k[R];
    if (k == kFNone) continue;  // nothing within max_distance leaves this component: it is final
    const uint64_t e = comp_e[R];
    const uint32_t i = (uint32_t)(e >> 32), j = (uint32_t)e;
    const uint32_t li = lab[i], other = (li == R) ? lab[j] : li;
    if (comp_k[other] == k && comp_e[other] == e && other < R) continue;  // the same edge from its other end: emitted and united there
    const uint32_t pos = atomicAdd(n_edges, 1u);
    if (pos < m) {  // (a forest on r1 rows has at most m = r1 - 1 edges)
      out_k[pos] = k;
      out_e[pos] = e;
    }
    atomicAdd(added, 1u);
    uf_unite<__HIP_MEMORY_SCOPE_AGENT>(par, R, other);
  }
}

// every row's root into par (uf_settle) and lab, the components' words cleared for the next round
__global__ __launch_bounds__(256) void forest_flatten_kernel(uint32_t *par, uint32_t *__restrict__ lab, uint64_t *__restrict__ comp_k,
                                                             uint64_t *__restrict__ comp_e, uint32_t r1, const uint32_t *gate) {
  FOREST_GATE();
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) {
    lab[i] = uf_settle<__HIP_MEMORY_SCOPE_AGENT>(par, (uint32_t)i);
    comp_k[i] = kFNone;
    comp_e[i] = kFNone;
  }
}

// the first sort's key: the pair in 2 jb bits (i, j < 2^jb); the value that travels is the edge's slot
__global__ __launch_bounds__(256) void forest_pair_keys_kernel(const uint64_t *__restrict__ out_e, uint32_t m, uint32_t jb, uint64_t *__restrict__ keys,
                                                               uint32_t *__restrict__ vals) {
  for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < m; q += (uint64_t)gridDim.x * 256) {
    const uint64_t e = out_e[q];
    keys[q] = ((e >> 32) << jb) | (e & 0xFFFFFFFFull);  // (an empty slot: any key, its distance's key puts it last)
    vals[q] = (uint32_t)q;
  }
}

// the second sort's key: the distance's, in the order the first sort left
__global__ __launch_bounds__(256) void forest_distance_keys_kernel(const uint64_t *__restrict__ out_k, const uint32_t *__restrict__ slot, uint32_t m,
                                                               uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < m; q += (uint64_t)gridDim.x * 256) {
    keys[q] = out_k[slot[q]];
    vals[q] = slot[q];
  }
}

__global__ __launch_bounds__(256) void forest_write_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ slot,
                                                           const uint64_t *__restrict__ out_e, const uint32_t *__restrict__ n_edges, uint32_t m,
                                                           uint32_t *__restrict__ edge_i, uint32_t *__restrict__ edge_j, double *__restrict__ edge_dist) {
  const uint32_t n = min(*n_edges, m);
  for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (uint64_t)gridDim.x * 256) {
    const uint64_t e = out_e[slot[q]];
    edge_i[q] = (uint32_t)(e >> 32);
    edge_j[q] = (uint32_t)e;
    edge_dist[q] = key_f64(keys[q]);
  }
}

// the workspace, carved: sized for the set's r1 alone
struct ForestWork {
  uint32_t *words, *lab, *par, *tile_lab, *part_c, *va, *vb, *v2a, *v2b;
  uint64_t *comp_k, *comp_e, *part_k, *out_k, *out_e, *ka, *kb, *k2a, *k2b;
  void *radix;
  uint64_t bytes;
};

static ForestWork forest_carve(void *base, uint32_t r1) {
  const uint64_t n = std::max(r1, 1u), m = std::max(r1, 2u) - 1;
  Carver c(base);
  ForestWork f;
  f.words = c.take<uint32_t>(4 * (kFMaxRounds + 1));  // what each round added
  f.lab = c.take<uint32_t>(n * 4);
  f.par = c.take<uint32_t>(n * 4);
  f.tile_lab = c.take<uint32_t>(n * 4);
  f.comp_k = c.take<uint64_t>(n * 8);
  f.comp_e = c.take<uint64_t>(n * 8);
  f.part_k = c.take<uint64_t>(n * 8 * kFMaxSeg);
  f.part_c = c.take<uint32_t>(n * 4 * kFMaxSeg);
  f.out_k = c.take<uint64_t>(m * 8);
  f.out_e = c.take<uint64_t>(m * 8);
  f.ka = c.take<uint64_t>(m * 8);
  f.kb = c.take<uint64_t>(m * 8);
  f.k2a = c.take<uint64_t>(m * 8);
  f.k2b = c.take<uint64_t>(m * 8);
  f.va = c.take<uint32_t>(m * 4);
  f.vb = c.take<uint32_t>(m * 4);
  f.v2a = c.take<uint32_t>(m * 4);
  f.v2b = c.take<uint32_t>(m * 4);
  f.radix = c.take<void>(radix_scratch_bytes(m));
  f.bytes = c.off;
  return f;
}

// core set: the mutual-reachability weight over those core distances; not set: the distance
template <int KIND>
static int forest_nearest(const double *a, uint32_t r1, uint32_t n_dims, const double *metric, double p, double max_distance, const double *core,
                          const ForestWork &f, uint32_t *lab, uint32_t *n_seg_out, const uint32_t *gate, hipStream_t st) {
  const SelfShape s = self_shape(r1);
  const uint32_t w = s.w, n_ct = div_up(r1, w), strips = div_up(r1, s.TJ);
  // the columns in a few segments when the strips alone do not fill the chip twice over
  const uint32_t want = div_up(2 * (uint64_t)std::max(ctx().n_cus, 1), strips);
  const uint32_t n_seg_max = std::max(1u, std::min({want, (uint32_t)kFMaxSeg, n_ct}));
  const uint32_t tiles_per_seg = div_up(n_ct, n_seg_max), n_seg = div_up(n_ct, tiles_per_seg);  // (no segment is empty)
  *n_seg_out = n_seg;
  forest_tile_labels_kernel<<<dim3(std::min(div_up(n_ct, 256), 4096u)), dim3(256), 0, st>>>(lab, r1, w, n_ct, f.tile_lab, gate);
  KPOP_LAUNCH_CHECK();
  if (strips > 0x7FFFFFFFu) KPOP_FAIL(KPOP_ERR_UNSUPPORTED, "kpop_dev_spanning_forest: %u rows", r1);
  const dim3 grid(strips, n_seg);
  by_shape_rows(s, [&](auto TY) {
    constexpr int ty = decltype(TY)::value;
    if (core)
      forest_nearest_kernel<KIND, ty, ForestReachWeight<ty>><<<grid, dim3(256), 0, st>>>(a, w, r1, n_dims, metric, p, max_distance, s.n_cg, s.n_rg, s.kf, n_ct,
                                                                                        tiles_per_seg, lab, f.tile_lab, f.part_k, f.part_c, gate, core);
    else
      forest_nearest_kernel<KIND, ty, ForestDistanceWeight><<<grid, dim3(256), 0, st>>>(a, w, r1, n_dims, metric, p, max_distance, s.n_cg, s.n_rg, s.kf, n_ct,
                                                                                       tiles_per_seg, lab, f.tile_lab, f.part_k, f.part_c, gate, nullptr);
  });
  KPOP_LAUNCH_CHECK();
  return 0;
}

static uint32_t forest_rounds(uint32_t r1) {  // ceil(log2 r1)
  uint32_t rounds = 0;
  while (rounds < 32 && (1ull << rounds) < r1) ++rounds;
  return rounds;
}

// the body of both entry points.  host_reads: after a round, wait for the word that says what it added and stop at zero;
// otherwise enqueues only.  d_core set: the edges weigh max(d, core_i, core_j) over those r1 core distances (forest_rounds.h: for
// reachability.hip)
int forest_dev(kpop_refset *rs, const double *d_core, double max_distance, void *d_work, uint32_t *d_n_edges, uint32_t *d_edge_i, uint32_t *d_edge_j,
                      double *d_edge_dist, uint32_t *d_labels, hipStream_t st, bool host_reads, const char *who) {
  if (max_distance != max_distance) KPOP_FAIL(KPOP_ERR_INVALID, "%s: the distance is not a number", who);
  if (!d_n_edges) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null count", who);
  KPOP_HIP(hipMemsetAsync(d_n_edges, 0, 4, st));
  const uint32_t r1 = rs->r1;
  if (r1 == 0) return KPOP_OK;
  if (r1 > 1 && (!d_edge_i || !d_edge_j || !d_edge_dist)) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null edge arrays", who);
  const ForestWork f = forest_carve(d_work, r1);
  uint32_t *lab = d_labels ? d_labels : f.lab;
  const uint32_t m = std::max(r1, 2u) - 1, rows_grid = std::min(div_up(r1, 256), 4096u);
  KPOP_HIP(hipMemsetAsync(f.words, 0, 4 * (kFMaxRounds + 1), st));
  forest_init_kernel<<<dim3(rows_grid), dim3(256), 0, st>>>(lab, f.par, f.comp_k, f.comp_e, f.out_k, f.out_e, r1, r1 > 1 ? m : 0);
  KPOP_LAUNCH_CHECK();
  if (r1 == 1 || !(max_distance >= 0.0)) return KPOP_OK;  // (no distance is negative: below zero every row stays alone)
  const double *a;
  KPOP_TRY(refset_chain_rows(rs, st, &a));
  const uint32_t rounds = forest_rounds(r1);
  for (uint32_t k = 0; k < rounds; ++k) {
    const uint32_t *gate = k ? f.words + (k - 1) : nullptr;
    uint32_t n_seg = 1;
    KPOP_TRY(by_kind(rs->kind, [&](auto K) { return forest_nearest<decltype(K)::value>(a, r1, rs->n_dims, rs->metric, rs->p, max_distance, d_core, f, lab, &n_seg, gate, st); }));
    forest_row_min_kernel<<<dim3(rows_grid), dim3(256), 0, st>>>(f.part_k, f.part_c, n_seg, r1, lab, f.comp_k, gate);
    KPOP_LAUNCH_CHECK();
    forest_comp_edge_kernel<<<dim3(rows_grid), dim3(256), 0, st>>>(f.part_k, f.part_c, r1, lab, f.comp_k, f.comp_e, gate);
    KPOP_LAUNCH_CHECK();
    forest_link_kernel<<<dim3(rows_grid), dim3(256), 0, st>>>(lab, f.comp_k, f.comp_e, r1, m, f.par, d_n_edges, f.out_k, f.out_e, f.words + k, gate);
    KPOP_LAUNCH_CHECK();
    forest_flatten_kernel<<<dim3(rows_grid), dim3(256), 0, st>>>(f.par, lab, f.comp_k, f.comp_e, r1, gate);
    KPOP_LAUNCH_CHECK();
    if (host_reads) {
      uint32_t added = 0;
      KPOP_HIP(hipMemcpyAsync(&added, f.words + k, 4, hipMemcpyDeviceToHost, st));
      KPOP_HIP(hipStreamSynchronize(st));
      if (added == 0) break;
    }
  }
  // the order: by the pair, then -- stably -- by the distance's key
  const uint32_t edges_grid = std::min(div_up(m, 256), 4096u);
  uint32_t jb = 1;
  while (jb < 32 && (1ull << jb) < r1) ++jb;
  forest_pair_keys_kernel<<<dim3(edges_grid), dim3(256), 0, st>>>(f.out_e, m, jb, f.ka, f.va);
  KPOP_LAUNCH_CHECK();
  uint64_t *ks = nullptr, *k2s = nullptr;
  uint32_t *vs = nullptr, *v2s = nullptr;
  KPOP_TRY(radix_sort_pairs_u64(f.ka, f.kb, f.va, f.vb, m, (int)(2 * jb), f.radix, st, &ks, &vs));
  forest_distance_keys_kernel<<<dim3(edges_grid), dim3(256), 0, st>>>(f.out_k, vs, m, f.k2a, f.v2a);
  KPOP_LAUNCH_CHECK();
  KPOP_TRY(radix_sort_pairs_u64(f.k2a, f.k2b, f.v2a, f.v2b, m, 64, f.radix, st, &k2s, &v2s));
  forest_write_kernel<<<dim3(edges_grid), dim3(256), 0, st>>>(k2s, v2s, f.out_e, d_n_edges, m, d_edge_i, d_edge_j, d_edge_dist);
  KPOP_LAUNCH_CHECK();
  return KPOP_OK;
}

uint64_t forest_workspace_bytes(uint32_t r1) { return forest_carve(nullptr, r1).bytes; }

}  // namespace kpop

using namespace kpop;

extern "C" uint64_t kpop_dev_spanning_forest_workspace_bytes(const kpop_refset *rs) {
  if (!rs) return 0;
  return forest_carve(nullptr, rs->r1).bytes;
}

extern "C" int kpop_dev_spanning_forest(kpop_refset *rs, double max_distance, void *d_work, uint32_t *d_n_edges, uint32_t *d_edge_i, uint32_t *d_edge_j,
                                        double *d_edge_dist, uint32_t *d_labels, void *stream) {
  const char *who = "kpop_dev_spanning_forest";
  KPOP_TRY(refset_check_handle(rs, who));
  if (!d_work) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null workspace", who);
  return forest_dev(rs, nullptr, max_distance, d_work, d_n_edges, d_edge_i, d_edge_j, d_edge_dist, d_labels, as_stream(stream), false, who);
}

extern "C" int kpop_spanning_forest(kpop_refset *rs, double max_distance, uint32_t *n_edges, uint32_t *edge_i, uint32_t *edge_j, double *edge_dist,
                                    uint32_t *labels) {
  const char *who = "kpop_spanning_forest";
  KPOP_TRY(refset_check_handle(rs, who));
  ArenaScope scratch;
  KPOP_TRY(check_distance_is_a_number(max_distance, who));
  const uint32_t r1 = rs->r1;
  if (!n_edges || (r1 > 1 && (!edge_i || !edge_j || !edge_dist))) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  *n_edges = 0;
  if (r1 == 0) return KPOP_OK;
  const uint64_t m = std::max(r1, 2u) - 1;
  HostCall h;
  void *work = h.work(forest_carve(nullptr, r1).bytes);
  uint32_t *dn = h.scalars<uint32_t>(), *di = h.counted(edge_i, m), *dj = h.counted(edge_j, m);
  double *dd = h.counted(edge_dist, m);
  uint32_t *dl = h.out(labels, r1);
  KPOP_TRY(h.upload());
  KPOP_TRY(forest_dev(rs, nullptr, max_distance, work, dn, di, dj, dd, dl, h.st, true, who));
  uint32_t n = 0;
  KPOP_TRY(h.read(&n, dn, 1));
  if (n > m) KPOP_FAIL(KPOP_ERR_HIP, "%s: %u edges on %u rows", who, n, r1);  // (cannot happen: a forest)
  KPOP_TRY(h.finish(n));
  *n_edges = n;
  return KPOP_OK;
}

extern "C" int kpop_distance_spanning_forest(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p, int normalize,
                                             double max_distance, uint32_t *n_edges, uint32_t *edge_i, uint32_t *edge_j, double *edge_dist,
                                             uint32_t *labels) {
  return with_temporary_refset(m, rows, n_dims, metric, kind, p, normalize,
                               [&](kpop_refset *rs) { return kpop_spanning_forest(rs, max_distance, n_edges, edge_i, edge_j, edge_dist, labels); });
}

// host arithmetic alone: the union-find of the labels, the larger root under the smaller, over the edges within T
extern "C" int kpop_forest_cut(uint32_t r1, uint32_t n_edges, const uint32_t *edge_i, const uint32_t *edge_j, const double *edge_dist, double T,
                               uint32_t *labels, uint32_t *n_clusters) {
  const char *who = "kpop_forest_cut";
  KPOP_TRY(check_distance_is_a_number(T, who));
  if (!n_clusters || (r1 && !labels) || (n_edges && (!edge_i || !edge_j || !edge_dist))) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  for (uint32_t e = 0; e < n_edges; ++e)
    if (!(edge_i[e] < edge_j[e] && edge_j[e] < r1))
      KPOP_FAIL(KPOP_ERR_INVALID, "%s: edge %u joins rows %u and %u of %u (i < j < r1)", who, e, edge_i[e], edge_j[e], r1);
  for (uint32_t i = 0; i < r1; ++i) labels[i] = i;
  auto find = [&](uint32_t x) {
    while (labels[x] != x) {
      labels[x] = labels[labels[x]];
      x = labels[x];
    }
    return x;
  };
  for (uint32_t e = 0; e < n_edges; ++e) {
    if (!(edge_dist[e] <= T)) continue;  // (a NaN joins nothing)
    const uint32_t a = find(edge_i[e]), b = find(edge_j[e]);
    if (a != b) labels[std::max(a, b)] = std::min(a, b);
  }
  uint32_t n = 0;
  for (uint32_t i = 0; i < r1; ++i) {
    labels[i] = find(i);
    n += labels[i] == i;
  }
  *n_clusters = n;
  return KPOP_OK;
}
