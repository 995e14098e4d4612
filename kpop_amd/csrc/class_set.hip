// class_set.hip -- rowwise distances of many rows to a small set of classes (Base.get_distance_rowwise, lib/Matrix.ml:191-266, with a
// first operand of fewer than 128 rows of at most 64 dimensions: KPopTwistDB -d against a class set, the headline step's second call).
//
//   class_set_prepare_kernel    the class side, once per call: norms (computed, supplied, or a resident set's), every divided row with a
//                               copy of the metric behind it, padded with +0.0 to DP dimensions, in the room of the workspace where the
//                               operands' divided copies would have gone
//   class_set_distance_kernel   a block owns 64 rows of the second operand, ONE ROW A LANE, held in registers; the four wavefronts split the
//                               classes.  The class values and the metric are wave-uniform: they are read through uniform addresses and
//                               reach the vector pipe as scalar operands.  The inner loop is the reference's chain and nothing else --
//                               sub, mul, mul, add a pair and dimension -- with no LDS traffic, no barrier and no padded column.
//
// Numerics are distance_rowwise_kernel's (distance.hip), operation for operation: a row's norm is row_norms_block's chain (row_norms.h),
// every element is divided by its row's norm once (lib/Matrix.ml:247-249), a pair's sum runs over the dimensions in ascending order in
// one lane, diff = a -. b with the class first, diff *. diff *. m left to right, nothing fused.  A padded dimension adds
// (0 - 0) * (0 - 0) * 0 = +0.0 to a sum that started at +0.0: the same bits.
//
// No state: no atomics, no counters, no memset, no allocation, no stream but the caller's.
#include <algorithm>

#include "common.h"
#include "space_ops.h"
#include "distance_routes.h"

namespace kpop {

constexpr int kClassRows = 64;    // rows of the second operand a block owns: one a lane
constexpr int kClassGroup = 8;    // dimensions a class hands over at a time: one 64-byte uniform load
constexpr int kClassFlight = 4;   // classes a wavefront carries at once (independent sums: no add waits for the one before it)
// the second operand's rows from which the default dispatch takes this path (class_set_applies).  Measured ahead of the tiled kernel at
// every eligible shape tried, 65 x r2 x 64 from 128 rows and 10 x r2 x 9 from 64 rows on (profiles/class_set_distance.md); shorter second
// operands seldom have the room to lend, and were not measured
constexpr uint32_t kClassSetMinRows = 128;

// One wavefront a class row, one dimension a lane (DP <= 64).  The norm is the sum of the lanes' components taken in ascending order,
// which is what row_norms_block's one thread a row does; the quotients are the divisions distance_rowwise_kernel does as it stages.
template <int KIND>
__global__ __launch_bounds__(256) void class_set_prepare_kernel(const double *__restrict__ m1, uint32_t r1, uint32_t n_dims, uint32_t dp,
                                                                const double *__restrict__ metric, double p, const double *__restrict__ norms1,
                                                                bool divide, double *__restrict__ n1_out, double *__restrict__ cls) {
  const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (i >= r1) return;  // (uniform in a wavefront)
  const bool in = lane < n_dims;
  const double el = in ? m1[(uint64_t)i * n_dims + lane] : 0.0, mc = in ? metric[lane] : 0.0;
  double nv = 1.0;  // normalize == 0: n = 1 and x /. 1. = x (lib/Matrix.ml:201-202)
  if (divide) {
    if (norms1) {
      nv = norms1[i];
    } else {
      // lib/Space.ml:169-178: acc +. (el *. el *. m_i), the dimensions in ascending order
      // (a lane past n_dims holds (0 * 0) * 0 = +0.0, and a sum that started at +0.0 is never -0.0: adding it changes no bit, so the
      // walk goes over all 64 lanes with constant lane numbers -- 64 lane reads, not 64 round trips through the LDS crossbar)
      const double t = component<KIND>(el, mc, p);
      double acc = 0.0;
#pragma unroll
      for (int c = 0; c < 64; ++c)
        acc = __dadd_rn(acc, __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(t), c), __builtin_amdgcn_readlane(__double2loint(t), c)));
      nv = scale_distance<KIND>(acc, p);
      nv = (nv == 0.0) ? 1.0 : nv;  // lib/Matrix.ml:67
      if (n1_out && lane == 0) n1_out[i] = nv;
    }
  }
  if (lane < dp) {
    cls[(uint64_t)i * 2u * dp + lane] = in ? (divide ? __ddiv_rn(el, nv) : el) : 0.0;
    cls[(uint64_t)i * 2u * dp + dp + lane] = mc;
  }
}

// NC classes from class i on against the lane's row x: NC sums, every one over the dimensions in ascending order
template <int KIND, int DP, int NC>
__device__ __forceinline__ void class_set_chain(const double (&x)[DP], const double *__restrict__ cls, uint32_t i, double p, double *stage) {
  double acc[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) acc[k] = 0.0;
  // (uniform: the loads below are scalar loads.  The metric is read from the copy behind class i, as it is wanted: 64 doubles read once
  // ahead of the loop over the classes do not fit the scalar registers and come back lane by lane out of a vector register)
  const double *__restrict__ a = cls + (uint64_t)i * (2 * DP);
  const double *__restrict__ metp = a + DP;
#pragma unroll
  for (int g = 0; g < DP; g += kClassGroup) {
#pragma unroll
    for (int d = 0; d < kClassGroup; ++d) {
      const double mc = metp[g + d];
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        // lib/Space.ml:192-200: diff = a -. b ; acc +. (diff *. diff *. m)
        const double diff = __dsub_rn(a[k * (2 * DP) + g + d], x[g + d]);
        acc[k] = __dadd_rn(acc[k], component<KIND>(diff, mc, p));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NC; ++k) stage[i + k] = scale_distance<KIND>(acc[k], p);  // data.(j).@(i), lib/Matrix.ml:253
}

// DP: the dimensions padded to a multiple of kClassGroup (cls: [r1][2][DP] -- a class's divided row, then the metric --, padding +0.0).  DIVIDE: normalize != 0.
// Dynamic LDS: 64 x max(DP + 1, r1 | 1) doubles -- the rows' tile, then the block's results.
template <int KIND, int DP, bool DIVIDE>
__global__ __launch_bounds__(256, DP == 64 ? 3 : 4) void class_set_distance_kernel(const double *__restrict__ cls,
                                                                                  uint32_t r1, const double *__restrict__ m2, uint32_t r2,
                                                                                  uint32_t n_dims, double p, double *__restrict__ n2,
                                                                                  double *__restrict__ out, uint32_t n_full, uint32_t tail_parts) {
  extern __shared__ __attribute__((aligned(16))) double class_lds[];
  constexpr int LD = DP + 1;  // (odd: a lane's row is read without bank conflicts; column DP holds the row's norm)
  constexpr int kPer = kClassRows * DP / 256;
  double *tile = class_lds;
  // The first n_full blocks take all the classes of their 64 rows.  The blocks behind them -- the round that would leave most of the
  // device idle while a few blocks walk every class at one wavefront's pace -- take the classes of their rows in tail_parts parts, a
  // block a part (launch_class_set_dp).  Which block computes a pair changes nothing about how it is computed.
  uint32_t rb = blockIdx.x, part = 0, parts = 1;
  if (blockIdx.x >= n_full) {
    const uint32_t t = blockIdx.x - n_full;
    rb = n_full + t / tail_parts;
    part = t % tail_parts;
    parts = tail_parts;
  }
  const uint32_t row0 = rb * (uint32_t)kClassRows;
  const uint32_t nrows = min((uint32_t)kClassRows, r2 - row0);
  // 1. the block's rows into LDS, coalesced; addresses clamped into the matrix, what lies outside stored as +0.0 (row_norms.h:36)
  {
    double pre[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const uint32_t e = threadIdx.x + 256u * u, i = e / DP, c = e % DP;
      pre[u] = m2[(uint64_t)min(row0 + i, r2 - 1u) * n_dims + min(c, n_dims - 1u)];
    }
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const uint32_t e = threadIdx.x + 256u * u, i = e / DP, c = e % DP;
      tile[i * LD + c] = (i < nrows && c < n_dims) ? pre[u] : 0.0;
    }
  }
  __syncthreads();
  if (DIVIDE) {
    // 2. norms: row_norms_block's operations, one lane a row
    if (threadIdx.x < (uint32_t)kClassRows) {
      const double *row = tile + threadIdx.x * LD;
      const double *__restrict__ metp = cls + DP;  // (the copy behind class 0)
      double acc = 0.0;
      // (all DP dimensions, unrolled, so that the reads run ahead of the chain of additions: a padded term is (0 * 0) * 0 = +0.0 and
      // a sum that started at +0.0 is never -0.0, so adding it changes no bit)
#pragma unroll
      for (int c = 0; c < DP; ++c) acc = __dadd_rn(acc, component<KIND>(row[c], metp[c], p));
      double nv = scale_distance<KIND>(acc, p);
      nv = (nv == 0.0) ? 1.0 : nv;  // lib/Matrix.ml:67
      tile[threadIdx.x * LD + DP] = nv;
      if (threadIdx.x < nrows && part == 0) n2[row0 + threadIdx.x] = nv;
    }
    __syncthreads();
    // 3. every element divided once (lib/Matrix.ml:248); the padding stays +0.0
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const uint32_t e = threadIdx.x + 256u * u, i = e / DP, c = e % DP;
      if (c < n_dims) tile[i * LD + c] = __ddiv_rn(tile[i * LD + c], tile[i * LD + DP]);
    }
    __syncthreads();
  }
  // 4. a lane's row into its registers (all four wavefronts hold the same 64 rows)
  const uint32_t lane = threadIdx.x & 63u;
  double x[DP];
#pragma unroll
  for (int c = 0; c < DP; ++c) x[c] = tile[lane * LD + c];
  __syncthreads();  // the tile's space is the results' from here
  // 5. the chains: the block's classes in four slices, a wavefront a slice, kClassFlight classes at a time, the remainder one at a time
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t slices = 4u * parts, u = 4u * part + wv;
  const uint32_t c_hi = (u + 1u) * r1 / slices;
  const uint32_t RS = r1 | 1u;
  double *stage = class_lds + lane * RS;
  uint32_t i = u * r1 / slices;
  for (; i + kClassFlight <= c_hi; i += kClassFlight) class_set_chain<KIND, DP, kClassFlight>(x, cls, i, p, stage);
  for (; i < c_hi; ++i) class_set_chain<KIND, DP, 1>(x, cls, i, p, stage);
  __syncthreads();
  // 6. a block with all the classes holds nrows x r1 results that are one contiguous stretch of `out`: full-width stores (a part of
  // the classes: bw consecutive results a row)
  const uint32_t b_lo = part * r1 / parts, bw = (part + 1u) * r1 / parts - b_lo;
  if (bw == 0) return;
  const uint32_t total = nrows * bw, dj = 256u / bw, di = 256u % bw;
  double *__restrict__ dst = out + (uint64_t)row0 * r1 + b_lo;
  const double *src = class_lds + b_lo;
  uint32_t j = threadIdx.x / bw, ii = threadIdx.x % bw;
  for (uint32_t e = threadIdx.x; e < total; e += 256u) {
    dst[(uint64_t)j * r1 + ii] = src[j * RS + ii];
    j += dj;
    ii += di;
    if (ii >= bw) {
      ii -= bw;
      ++j;
    }
  }
}

static uint32_t class_set_padded_dims(uint32_t n_dims) { return n_dims <= 8 ? 8u : n_dims <= 16 ? 16u : n_dims <= 32 ? 32u : 64u; }

// kpop_tune("class_set", v): 0 never, 1 (default) eligible shapes from kClassSetMinRows rows on, 2 every eligible shape.
// room_doubles: what the workspace holds where the operands' copies would go (DistWork::a and ::b; ::b alone with a resident set), 0
// without a workspace.
bool class_set_applies(int kind, uint32_t r1, uint32_t r2, uint32_t n_dims, uint64_t room_doubles) {
  const int mode = ctx().tune_class_set;
  if (mode == 0 || (kind != KPOP_EUCLIDEAN && kind != KPOP_COSINE)) return false;
  if (n_dims == 0 || n_dims > 64 || r1 < 1 || r1 >= 128 || r2 < 1 || r2 >= (1u << 30)) return false;
  const uint64_t dp = class_set_padded_dims(n_dims);
  if (2u * (uint64_t)r1 * dp > room_doubles) return false;  // the padded classes and metric must fit the room they borrow
  return mode == 2 || r2 >= kClassSetMinRows;
}

template <int KIND, int DP>
static int launch_class_set_dp(const double *cls, uint32_t r1, const double *m2, uint32_t r2, uint32_t n_dims, double p,
                               bool divide, double *n2, double *out, hipStream_t st) {
  // Blocks are handed out as slots free.  The last, partial round of them is cut finer when it is short: its row blocks take their classes
  // in 2, 4 or 8 parts, so that the device does not wait for a few blocks that walk all the classes with a SIMD to themselves (65 x
  // 100,000 x 64: 1,563 blocks over 768 slots are two rounds and 27 blocks).  A pure function of the shape and the device: no state.
  const uint32_t slots = (uint32_t)ctx().n_cus * (DP == 64 ? 3u : 4u), blocks = div_up(r2, kClassRows);
  const uint32_t tail = blocks % slots;
  uint32_t parts = 1;
  if (tail) parts = tail * 8u <= slots ? 8u : tail * 4u <= slots ? 4u : tail * 2u <= slots ? 2u : 1u;
  parts = std::max(1u, std::min(parts, r1 / 4u));  // (a wavefront keeps a class or more)
  const uint32_t n_full = parts > 1 ? blocks - tail : blocks;
  const dim3 grid(n_full + (blocks - n_full) * parts), block(256);
  const size_t lds = sizeof(double) * kClassRows * std::max<size_t>(DP + 1, r1 | 1u);
  if (divide) class_set_distance_kernel<KIND, DP, true><<<grid, block, lds, st>>>(cls, r1, m2, r2, n_dims, p, n2, out, n_full, parts);
  else class_set_distance_kernel<KIND, DP, false><<<grid, block, lds, st>>>(cls, r1, m2, r2, n_dims, p, n2, out, n_full, parts);
  KPOP_LAUNCH_CHECK();
  return 0;
}

// norms1: the first operand's norms when the caller (or a resident set) brings them, else they are computed and written to n1_out
// (n1_out may be null: a resident set's workspace has no room for them).  room: see class_set_applies.  n2: the workspace's norms of the rows.
template <int KIND>
static int launch_class_set_kind(const double *m1, uint32_t r1, const double *norms1, double *n1_out, const double *m2, uint32_t r2, double *n2,
                                 uint32_t n_dims, const double *metric, double p, bool divide, double *room, double *out, hipStream_t st) {
  const uint32_t dp = class_set_padded_dims(n_dims);
  double *cls = room;
  class_set_prepare_kernel<KIND><<<dim3(div_up(r1, 4)), dim3(256), 0, st>>>(m1, r1, n_dims, dp, metric, p, norms1, divide, n1_out, cls);
  KPOP_LAUNCH_CHECK();
  switch (dp) {
    case 8: return launch_class_set_dp<KIND, 8>(cls, r1, m2, r2, n_dims, p, divide, n2, out, st);
    case 16: return launch_class_set_dp<KIND, 16>(cls, r1, m2, r2, n_dims, p, divide, n2, out, st);
    case 32: return launch_class_set_dp<KIND, 32>(cls, r1, m2, r2, n_dims, p, divide, n2, out, st);
    default: return launch_class_set_dp<KIND, 64>(cls, r1, m2, r2, n_dims, p, divide, n2, out, st);
  }
}

int launch_class_set_distance(int kind, const double *m1, uint32_t r1, const double *norms1, double *n1_out, const double *m2, uint32_t r2, double *n2,
                              uint32_t n_dims, const double *metric, double p, bool divide, double *room, double *out, hipStream_t st) {
  if (kind == KPOP_EUCLIDEAN) return launch_class_set_kind<KPOP_EUCLIDEAN>(m1, r1, norms1, n1_out, m2, r2, n2, n_dims, metric, p, divide, room, out, st);
  return launch_class_set_kind<KPOP_COSINE>(m1, r1, norms1, n1_out, m2, r2, n2, n_dims, metric, p, divide, room, out, st);
}

}  // namespace kpop
