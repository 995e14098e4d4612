// distill.hip -- distill_kmers of KPopCountDB -d (lib/KMerDB.ml:812-976) on the GPU: for every k-mer, the absolute
// differences of the normalised counts of all S(S-1)/2 pairs of spectra, binned by the pair of classes they fall in,
// summarised per bin (mean, sample variance, coefficient of variation), then across the diagonal ("Inner") and the
// off-diagonal ("Outer") bins (mean and median), and a straight line Outer ~ Inner fitted over all k-mers whose residuals
// are the ranking.  The semantics are declared in INTEGRATION.md ("distill"); tests/distill_ref.py restates them.
//
// Everything is f64 on the vector pipe, lanes along k-mers (every read of a spectrum is a run of consecutive int32), no
// atomics and one fixed order of additions: the same bits on every run, whatever the band size.
//
//   cells    one thread per k-mer, one block row per class a.  The spectra arrive sorted by class (a permutation built on
//            the host), so the cell (a, b) is a rectangle of members, or a triangle when a == b.  A thread keeps the
//            normalised counts of up to M members of a and up to M of b in a column of LDS of its own ([member][thread]:
//            the thread is the fastest index, so ds_read_b64 / ds_write_b64 are conflict-free and no barrier is ever needed)
//            and walks the rectangle in 4 x 4 register tiles: 8 LDS reads serve 16 pairs of 3 operations each (subtract,
//            add |d|, fused multiply-add d*d) -- 6 vector operations an LDS read where the LDS could feed 2.  Classes of more
//            than M members go through in chunks of M.  Sum and sum of squares are kept in four partial accumulators a thread
//            (one per tile row) and folded in a fixed order.
//   reduce   one thread per k-mer: mean and median (sorted[n / 2]) of the C diagonal and of the C(C-1)/2 off-diagonal cell
//            values, for each of the three quantities.  Up to 296 values the thread sorts them by insertion in an LDS column of
//            its own as it reads them; up to 5,120 (101 classes) a wavefront takes the k-mer, holds the values in registers and
//            selects the rank with ballots (wave_select.h); beyond, a thread resolves the rank bit by bit over the band
//            workspace (any C, slow).
//   fit      per (quantity, Mean | Median): block-tree sums of x and y, the means, block-tree centred sums, slope and
//            intercept, and an elementwise pass for the residuals.
//
// The k-mers go through in bands, sized so that the cells of a band (n_cells x 3 doubles a k-mer) fit the workspace;
// kpop_tune("distill_band", n) makes the bands smaller (the tests run several bands where one would do).
#include <math.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "wave_select.h"

namespace kpop {

namespace {

constexpr int kCellThreads = 128;
constexpr uint32_t kReduceLdsValues = 296;  // x 64 threads x 8 bytes = 151,552 bytes of the CU's 160 KiB
constexpr uint32_t kFitBlocks = 1024;
constexpr uint64_t kBandBytes = 1ull << 30;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// poff[p] = offset of the p-th spectrum in class order, psum[p] = its linear column sum
__global__ void distill_prep_kernel(const uint32_t *__restrict__ perm, const double *__restrict__ col_stats, uint64_t ld, uint32_t n_cols,
                                    uint64_t *__restrict__ poff, double *__restrict__ psum) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_cols) return;
  poff[p] = (uint64_t)perm[p] * ld;
  psum[p] = col_stats[4 * (uint64_t)perm[p] + 2];
}

struct Acc {
  double s[4], q[4];
};

__device__ __forceinline__ void add_pair(double a, double b, double &s, double &q) {
  const double d = a - b;
  s += fabs(d);
  q = fma(d, d, q);
}

// four members in registers against x[j_lo .. j_hi)
template <int T>
__device__ __forceinline__ void rows4(const double (&a)[4], const double *x, uint32_t j_lo, uint32_t j_hi, Acc &acc) {
  uint32_t j = j_lo;
  for (; j + 4 <= j_hi; j += 4) {
    double b[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) b[v] = x[(j + v) * T];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) add_pair(a[u], b[v], acc.s[u], acc.q[u]);
  }
  for (; j < j_hi; ++j) {
    const double b = x[j * T];
#pragma unroll
    for (int u = 0; u < 4; ++u) add_pair(a[u], b, acc.s[u], acc.q[u]);
  }
}

// one member against x[j_lo .. j_hi)
template <int T>
__device__ __forceinline__ void row1(double a, const double *x, uint32_t j_lo, uint32_t j_hi, Acc &acc) {
  uint32_t j = j_lo;
  for (; j + 4 <= j_hi; j += 4) {
#pragma unroll
    for (int v = 0; v < 4; ++v) add_pair(a, x[(j + v) * T], acc.s[v], acc.q[v]);
  }
  for (; j < j_hi; ++j) add_pair(a, x[j * T], acc.s[0], acc.q[0]);
}

// every pair (i, j) of xa[0 .. na) x xb[0 .. nb)
template <int T>
__device__ __forceinline__ void rectangle(const double *xa, uint32_t na, const double *xb, uint32_t nb, Acc &acc) {
  uint32_t i = 0;
  for (; i + 4 <= na; i += 4) {
    double a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = xa[(i + u) * T];
    rows4<T>(a, xb, 0, nb, acc);
  }
  for (; i < na; ++i) row1<T>(xa[i * T], xb, 0, nb, acc);
}

// every pair i < j of x[0 .. n)
template <int T>
__device__ __forceinline__ void triangle(const double *x, uint32_t n, Acc &acc) {
  uint32_t i = 0;
  for (; i + 4 <= n; i += 4) {
    double a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = x[(i + u) * T];
    add_pair(a[0], a[1], acc.s[0], acc.q[0]);
    add_pair(a[0], a[2], acc.s[0], acc.q[0]);
    add_pair(a[0], a[3], acc.s[0], acc.q[0]);
    add_pair(a[1], a[2], acc.s[1], acc.q[1]);
    add_pair(a[1], a[3], acc.s[1], acc.q[1]);
    add_pair(a[2], a[3], acc.s[2], acc.q[2]);
    rows4<T>(a, x, i + 4, n, acc);
  }
  for (; i < n; ++i) row1<T>(x[i * T], x, i + 1, n, acc);
}

// x[m] = count / sum of the spectra p0 .. p0 + n of the class order: a true division (0 / 0 = NaN for an empty spectrum)
template <int T>
__device__ __forceinline__ void stage(double *x, const int32_t *__restrict__ storage, const uint64_t *__restrict__ poff,
                                      const double *__restrict__ psum, uint32_t p0, uint32_t n, uint64_t r) {
  uint32_t m = 0;
  for (; m + 4 <= n; m += 4) {
    int32_t c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) c[u] = storage[poff[p0 + m + u] + r];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[(m + u) * T] = __ddiv_rn((double)c[u], psum[p0 + m + u]);
  }
  for (; m < n; ++m) x[m * T] = __ddiv_rn((double)storage[poff[p0 + m] + r], psum[p0 + m]);
}

// the off-diagonal cell (a, b), a < b, in the order the reference visits them (lib/KMerDB.ml:876-889); the C diagonal
// cells come first in the workspace
__host__ __device__ __forceinline__ uint64_t off_cell(uint32_t a, uint32_t b, uint32_t n_classes) {
  return (uint64_t)n_classes + (uint64_t)a * (2ull * n_classes - a - 1) / 2 + (b - a - 1);
}

// cells[(cell * 3 + {mean, var, cov}) * band_ld + k-mer of the band]
template <int M>
__global__ __launch_bounds__(kCellThreads) void distill_cells_kernel(const int32_t *__restrict__ storage, uint64_t row0, uint32_t band_rows,
                                                                    uint64_t band_ld, const uint64_t *__restrict__ poff,
                                                                    const double *__restrict__ psum, const uint32_t *__restrict__ cls_off,
                                                                    uint32_t n_classes, double *__restrict__ cells) {
  constexpr int T = kCellThreads;
  extern __shared__ double distill_lds[];
  double *xa = distill_lds + threadIdx.x, *xb = xa + M * T;
  const uint32_t a = blockIdx.y;
  const uint32_t lr = blockIdx.x * T + threadIdx.x;
  const bool live = lr < band_rows;
  const uint64_t r = row0 + (live ? lr : 0);  // the threads past the end redo the band's first k-mer and store nothing
  const uint32_t a_lo = cls_off[a], a_hi = cls_off[a + 1], ma = a_hi - a_lo;
  bool a_staged = false;
  for (uint32_t b = a; b < n_classes; ++b) {
    const uint32_t b_lo = cls_off[b], b_hi = cls_off[b + 1], mb = b_hi - b_lo;
    Acc acc;
#pragma unroll
    for (int u = 0; u < 4; ++u) acc.s[u] = acc.q[u] = 0.;
    for (uint32_t i0 = a_lo; i0 < a_hi; i0 += M) {
      const uint32_t na = min((uint32_t)M, a_hi - i0);
      if (!(ma <= (uint32_t)M && a_staged)) {  // a class of one chunk stays where it is along its row of cells
        stage<T>(xa, storage, poff, psum, i0, na, r);
        a_staged = true;
      }
      for (uint32_t j0 = (b == a ? i0 : b_lo); j0 < b_hi; j0 += M) {
        const uint32_t nb = min((uint32_t)M, b_hi - j0);
        if (b == a && j0 == i0) {
          triangle<T>(xa, na, acc);
        } else {
          stage<T>(xb, storage, poff, psum, j0, nb, r);
          rectangle<T>(xa, na, xb, nb, acc);
        }
      }
    }
    const double n = b == a ? (double)ma * (double)(ma - 1) * 0.5 : (double)ma * (double)mb;
    const double s = (acc.s[0] + acc.s[1]) + (acc.s[2] + acc.s[3]), q = (acc.q[0] + acc.q[1]) + (acc.q[2] + acc.q[3]);
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const double mean = n >= 1. ? s / n : nan;
    double var = nan;
    if (n >= 2.) {
      var = (q - s * mean) / (n - 1.);
      if (var < 0.) var = 0.;  // (rounding; a NaN stays a NaN)
    }
    const double cov = sqrt(var) / mean;
    if (live) {
      double *o = cells + (b == a ? (uint64_t)a : off_cell(a, b, n_classes)) * 3 * band_ld + lr;
      o[0] = mean;
      o[band_ld] = var;
      o[2 * band_ld] = cov;
    }
  }
}

// out rows of quantity q: 6q + {0 InnerMean, 1 OuterMean, 2 ResidualMean, 3 InnerMedian, 4 OuterMedian, 5 ResidualMedian}
__global__ __launch_bounds__(64) void distill_reduce_lds_kernel(const double *__restrict__ cells, uint64_t band_ld, uint32_t band_rows,
                                                                uint64_t row0, uint64_t n_rows, uint32_t n_classes, uint32_t n_off,
                                                                double *__restrict__ out) {
  extern __shared__ double distill_lds[];
  double *col = distill_lds + threadIdx.x;
  const uint32_t lr = blockIdx.x * 64 + threadIdx.x;
  if (lr >= band_rows) return;
  const uint64_t r = row0 + lr;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  for (uint32_t q = 0; q < 3; ++q)
    for (uint32_t g = 0; g < 2; ++g) {
      const uint32_t first = g ? n_classes : 0, n = g ? n_off : n_classes;
      double sum = 0.;
      bool any_nan = false;
      for (uint32_t i = 0; i < n; ++i) {
        const double v = cells[((uint64_t)(first + i) * 3 + q) * band_ld + lr];
        any_nan |= v != v;
        sum += v;
        uint32_t j = i;
        while (j > 0) {
          const double w = col[(j - 1) * 64];
          if (!(w > v)) break;
          col[j * 64] = w;
          --j;
        }
        col[j * 64] = v;
      }
      out[(uint64_t)(6 * q + g) * n_rows + r] = any_nan ? nan : sum / (double)n;
      out[(uint64_t)(6 * q + 3 + g) * n_rows + r] = any_nan ? nan : col[(n / 2) * 64];
    }
}

// Up to 64 R off-diagonal cells (and up to 128 classes): one wavefront per k-mer, the cell values in registers (R a lane; which
// lane holds which cell does not matter to a sum in a fixed tree or to a rank), the median by wave_select_rank.  The eight
// wavefronts of a block take eight neighbouring k-mers: their strided loads share their 64-byte sectors.
template <int R>
__global__ __launch_bounds__(512) void distill_reduce_wave_kernel(const double *__restrict__ cells, uint64_t band_ld, uint32_t band_rows,
                                                                  uint64_t row0, uint64_t n_rows, uint32_t n_classes, uint32_t n_off,
                                                                  double *__restrict__ out) {
  const uint32_t lane = threadIdx.x & 63, lr = blockIdx.x * 8 + (threadIdx.x >> 6);
  if (lr >= band_rows) return;  // (a whole wavefront: no barrier in this kernel)
  const uint64_t r = row0 + lr;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  for (uint32_t q = 0; q < 3; ++q) {
    double mean[2], med[2];
    {  // Inner
      double v[2], sum = 0.;
      bool bad = false;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const uint32_t i = (uint32_t)k * 64 + lane;
        const bool in = i < n_classes;
        const double x = in ? cells[((uint64_t)i * 3 + q) * band_ld + lr] : 0.;
        bad |= x != x;
        sum += x;
        v[k] = in ? x : INFINITY;
      }
      const bool any_nan = __ballot(bad) != 0;
      mean[0] = any_nan ? nan : __shfl(wave_sum(sum), 0, 64) / (double)n_classes;  // (the tree's total is lane 0's)
      med[0] = any_nan ? nan : wave_select_rank<2>(v, n_classes >> 1);
    }
    {  // Outer
      double v[R], sum = 0.;
      bool bad = false;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const uint32_t i = (uint32_t)k * 64 + lane;
        const bool in = i < n_off;
        const double x = in ? cells[((uint64_t)(n_classes + i) * 3 + q) * band_ld + lr] : 0.;
        bad |= x != x;
        sum += x;
        v[k] = in ? x : INFINITY;
      }
      const bool any_nan = __ballot(bad) != 0;
      mean[1] = any_nan ? nan : __shfl(wave_sum(sum), 0, 64) / (double)n_off;
      med[1] = any_nan ? nan : wave_select_rank<R>(v, n_off >> 1);
    }
    if (lane < 4) out[(uint64_t)(6 * q + 3 * (lane >> 1) + (lane & 1)) * n_rows + r] = lane < 2 ? mean[lane & 1] : med[lane & 1];
  }
}

__device__ __forceinline__ uint64_t ordered_key(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  return b ^ ((uint64_t)((int64_t)b >> 63) | 0x8000000000000000ull);
}
__device__ __forceinline__ double ordered_value(uint64_t k) {
  const uint64_t b = (k & 0x8000000000000000ull) ? (k ^ 0x8000000000000000ull) : ~k;
  return __longlong_as_double((long long)b);
}

// any number of classes: the key of rank n / 2 resolved bit by bit, a sweep over the k-mer's cell values a bit
__global__ __launch_bounds__(256) void distill_reduce_bits_kernel(const double *__restrict__ cells, uint64_t band_ld, uint32_t band_rows,
                                                                  uint64_t row0, uint64_t n_rows, uint32_t n_classes, uint32_t n_off,
                                                                  double *__restrict__ out) {
  const uint32_t lr = blockIdx.x * 256 + threadIdx.x;
  if (lr >= band_rows) return;
  const uint64_t r = row0 + lr;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  for (uint32_t q = 0; q < 3; ++q)
    for (uint32_t g = 0; g < 2; ++g) {
      const uint32_t first = g ? n_classes : 0, n = g ? n_off : n_classes;
      const double *v = cells + ((uint64_t)first * 3 + q) * band_ld + lr;
      const uint64_t step = 3 * band_ld;
      double sum = 0.;
      bool any_nan = false;
      for (uint32_t i = 0; i < n; ++i) {
        const double x = v[i * step];
        any_nan |= x != x;
        sum += x;
      }
      double med = nan;
      if (!any_nan) {
        uint64_t prefix = 0ull, known = 0ull;
        uint32_t rank = n >> 1;
        for (int bit = 63; bit >= 0; --bit) {
          const uint64_t m = 1ull << bit;
          uint32_t zeros = 0;
          for (uint32_t i = 0; i < n; ++i) {
            const uint64_t key = ordered_key(v[i * step]);
            zeros += ((key & known) == prefix && !(key & m)) ? 1u : 0u;
          }
          if (rank >= zeros) {
            rank -= zeros;
            prefix |= m;
          }
          known |= m;
        }
        med = ordered_value(prefix);
      }
      out[(uint64_t)(6 * q + g) * n_rows + r] = any_nan ? nan : sum / (double)n;
      out[(uint64_t)(6 * q + 3 + g) * n_rows + r] = med;
    }
}

// fit f = 2 * quantity + {0 Mean, 1 Median}: x = row 6q + 3m, y = the row after it, residuals the row after that
__device__ __forceinline__ uint64_t fit_x_row(uint32_t f) { return 6 * (f >> 1) + 3 * (f & 1); }

// res[f] = {mean of x, mean of y, intercept, slope}.  centred == 0: partial sums of x and of y; 1: of (x - mx)(y - my) and
// (x - mx)^2.  Every block owns a fixed slice of the k-mers and adds it up in a fixed tree.
__global__ __launch_bounds__(256) void distill_fit_sums_kernel(const double *__restrict__ out, uint64_t n_rows, int centred,
                                                               const double *__restrict__ res, double *__restrict__ partial) {
  const uint32_t f = blockIdx.y;
  const double *x = out + fit_x_row(f) * n_rows, *y = x + n_rows;
  const uint64_t per = (n_rows + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * per, hi = min(n_rows, lo + per);
  const double mx = centred ? res[4 * f] : 0., my = centred ? res[4 * f + 1] : 0.;
  double s0 = 0., s1 = 0.;
  for (uint64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const double dx = x[i] - mx, dy = y[i] - my;
    s0 += centred ? dx * dy : dx;
    s1 += centred ? dx * dx : dy;
  }
  __shared__ double sh[2][4];
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = s0;
    sh[1][threadIdx.x >> 6] = s1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double *p = partial + 2 * ((uint64_t)f * gridDim.x + blockIdx.x);
    p[0] = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
    p[1] = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
  }
}

__global__ void distill_fit_finish_kernel(const double *__restrict__ partial, uint32_t n_blocks, uint64_t n_rows, int centred,
                                          double *__restrict__ res) {
  const uint32_t f = threadIdx.x;
  if (f >= 6) return;
  double s0 = 0., s1 = 0.;
  for (uint32_t b = 0; b < n_blocks; ++b) {
    s0 += partial[2 * ((uint64_t)f * n_blocks + b)];
    s1 += partial[2 * ((uint64_t)f * n_blocks + b) + 1];
  }
  if (!centred) {
    res[4 * f] = s0 / (double)n_rows;
    res[4 * f + 1] = s1 / (double)n_rows;
  } else {
    const double slope = s0 / s1;
    res[4 * f + 3] = slope;
    res[4 * f + 2] = res[4 * f + 1] - slope * res[4 * f];
  }
}

__global__ __launch_bounds__(256) void distill_residual_kernel(double *__restrict__ out, uint64_t n_rows, const double *__restrict__ res) {
  const uint32_t f = blockIdx.y;
  const double *x = out + fit_x_row(f) * n_rows, *y = x + n_rows;
  double *o = out + (fit_x_row(f) + 2) * n_rows;
  const double a = res[4 * f + 2], b = res[4 * f + 3];
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_rows; i += stride) o[i] = y[i] - (a + b * x[i]);
}

uint64_t up256(uint64_t n) { return (n + 255) / 256 * 256; }

struct DistillLayout {
  uint64_t stats_ws, col_stats, perm, cls_off, poff, psum, partial, res, cells, total;
  uint64_t band;  // k-mers a band, a multiple of the cell kernel's block
};

DistillLayout distill_layout(uint32_t n_cols, uint64_t n_rows, uint32_t n_classes) {
  DistillLayout L;
  const uint64_t n_cells = (uint64_t)n_classes * ((uint64_t)n_classes + 1) / 2;
  uint64_t at = 0;
  auto take = [&](uint64_t bytes) {
    const uint64_t here = at;
    at += up256(bytes);
    return here;
  };
  L.stats_ws = take(kpop_dev_counter_workspace_bytes(n_cols, n_rows));
  L.col_stats = take((uint64_t)n_cols * 32);
  L.perm = take((uint64_t)n_cols * 4);
  L.cls_off = take(((uint64_t)n_classes + 1) * 4);
  L.poff = take((uint64_t)n_cols * 8);
  L.psum = take((uint64_t)n_cols * 8);
  L.partial = take(6ull * kFitBlocks * 16);
  L.res = take(6 * 4 * 8);
  const uint64_t all = (n_rows + kCellThreads - 1) / kCellThreads * kCellThreads;
  const uint64_t fit = kBandBytes / std::max<uint64_t>(1, n_cells * 24) / kCellThreads * kCellThreads;
  L.band = std::max<uint64_t>(kCellThreads, std::min(all, fit));
  L.cells = take(L.band * n_cells * 24);
  L.total = at;
  return L;
}

int check_class_count(uint32_t n_cols, uint32_t n_classes, const char *who) {
  if (n_classes <= 1 || n_classes >= n_cols)  // lib/KMerDB.ml:822-823
    KPOP_FAIL(KPOP_ERR_INVALID, "%s: Invalid_number_of_classes(%u)", who, n_classes);
  if (n_classes > 65535) KPOP_FAIL(KPOP_ERR_UNSUPPORTED, "%s: more than 65,535 classes", who);
  return 0;
}

// `classes` is on the host here; everything else as kpop_dev_counter_distill
int distill_run(const int32_t *d_storage, uint64_t ld, uint32_t n_cols, uint64_t n_rows, const uint32_t *classes, uint32_t n_classes,
                void *d_workspace, double *d_out, double *fits_host, hipStream_t st, const char *who) {
  KPOP_TRY(check_class_count(n_cols, n_classes, who));
  std::vector<uint32_t> cls_off(n_classes + 1, 0), perm(n_cols);
  for (uint32_t c = 0; c < n_cols; ++c) {
    if (classes[c] >= n_classes) KPOP_FAIL(KPOP_ERR_INVALID, "%s: spectrum %u has class %u of %u", who, c, classes[c], n_classes);
    ++cls_off[classes[c] + 1];
  }
  uint32_t largest = 0;
  for (uint32_t k = 0; k < n_classes; ++k) {
    if (cls_off[k + 1] == 0) KPOP_FAIL(KPOP_ERR_INVALID, "%s: class %u is empty", who, k);
    largest = std::max(largest, cls_off[k + 1]);
    cls_off[k + 1] += cls_off[k];
  }
  {
    std::vector<uint32_t> next(cls_off.begin(), cls_off.end() - 1);
    for (uint32_t c = 0; c < n_cols; ++c) perm[next[classes[c]]++] = c;  // members keep their order inside a class
  }
  if (fits_host) std::fill(fits_host, fits_host + 12, NAN);
  if (n_rows == 0) return KPOP_OK;
  if (!d_storage || !d_workspace || !d_out) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  if (ld < n_rows) KPOP_FAIL(KPOP_ERR_INVALID, "%s: ld=%llu for %llu rows", who, (unsigned long long)ld, (unsigned long long)n_rows);
  Context &c = ctx();
  const DistillLayout L = distill_layout(n_cols, n_rows, n_classes);
  char *ws = reinterpret_cast<char *>(d_workspace);
  double *col_stats = reinterpret_cast<double *>(ws + L.col_stats);
  uint32_t *d_perm = reinterpret_cast<uint32_t *>(ws + L.perm), *d_cls_off = reinterpret_cast<uint32_t *>(ws + L.cls_off);
  uint64_t *poff = reinterpret_cast<uint64_t *>(ws + L.poff);
  double *psum = reinterpret_cast<double *>(ws + L.psum), *partial = reinterpret_cast<double *>(ws + L.partial);
  double *res = reinterpret_cast<double *>(ws + L.res), *cells = reinterpret_cast<double *>(ws + L.cells);
  KPOP_HIP(hipMemcpyAsync(d_perm, perm.data(), (uint64_t)n_cols * 4, hipMemcpyHostToDevice, st));
  KPOP_HIP(hipMemcpyAsync(d_cls_off, cls_off.data(), ((uint64_t)n_classes + 1) * 4, hipMemcpyHostToDevice, st));
  // no thresholding, linear statistics (lib/KMerDB.ml:819-820)
  KPOP_TRY(kpop_dev_counter_stats(d_storage, ld, n_cols, n_rows, 1., 1., ws + L.stats_ws, col_stats, nullptr, st));
  distill_prep_kernel<<<dim3(div_up(n_cols, 256)), dim3(256), 0, st>>>(d_perm, col_stats, ld, n_cols, poff, psum);
  KPOP_LAUNCH_CHECK();

  uint64_t band = L.band;
  if (c.tune_distill_band > 0)
    band = std::min<uint64_t>(band, ((uint64_t)c.tune_distill_band + kCellThreads - 1) / kCellThreads * kCellThreads);
  const uint32_t n_off = n_classes * (n_classes - 1) / 2;
  const bool reduce_lds = std::max(n_classes, n_off) <= kReduceLdsValues;
  const size_t reduce_bytes = (size_t)std::max(n_classes, n_off) * 64 * 8;
  if (reduce_lds && reduce_bytes > 65536) {
    static PerSlotOnce attr_once;
    bool &attr_set = attr_once();
    if (!attr_set) {
      KPOP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&distill_reduce_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(kReduceLdsValues * 64 * 8)));
      attr_set = true;
    }
  }
  // phase clocks (kpop_tune("distill_clock", 1)): the stream is drained after every band, for measurements only
  const bool clock = c.tune_distill_clock != 0;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  if (clock) {
    for (auto &e : ev) KPOP_HIP(hipEventCreate(&e));
    c.distill_ms[0] = c.distill_ms[1] = c.distill_ms[2] = 0.;
  }
  for (uint64_t row0 = 0; row0 < n_rows; row0 += band) {
    const uint32_t rows = (uint32_t)std::min<uint64_t>(band, n_rows - row0);
    const dim3 grid(div_up(rows, kCellThreads), n_classes);
    if (clock) KPOP_HIP(hipEventRecord(ev[0], st));
#define KPOP_DISTILL_CELLS(MM)                                                                                                     \
  distill_cells_kernel<MM><<<grid, dim3(kCellThreads), (size_t)2 * MM * kCellThreads * 8, st>>>(d_storage, row0, rows, band, poff, psum, \
                                                                                                  d_cls_off, n_classes, cells)
    if (largest <= 8) KPOP_DISTILL_CELLS(8);
    else if (largest <= 16) KPOP_DISTILL_CELLS(16);
    else KPOP_DISTILL_CELLS(32);
#undef KPOP_DISTILL_CELLS
    KPOP_LAUNCH_CHECK();
    if (clock) KPOP_HIP(hipEventRecord(ev[1], st));
#define KPOP_DISTILL_REDUCE_WAVE(RR) \
  distill_reduce_wave_kernel<RR><<<dim3(div_up(rows, 8)), dim3(512), 0, st>>>(cells, band, rows, row0, n_rows, n_classes, n_off, d_out)
    if (reduce_lds)
      distill_reduce_lds_kernel<<<dim3(div_up(rows, 64)), dim3(64), reduce_bytes, st>>>(cells, band, rows, row0, n_rows, n_classes, n_off, d_out);
    else if (n_classes <= 128 && n_off <= 64 * 16) KPOP_DISTILL_REDUCE_WAVE(16);
    else if (n_classes <= 128 && n_off <= 64 * 40) KPOP_DISTILL_REDUCE_WAVE(40);
    else if (n_classes <= 128 && n_off <= 64 * 80) KPOP_DISTILL_REDUCE_WAVE(80);
    else
      distill_reduce_bits_kernel<<<dim3(div_up(rows, 256)), dim3(256), 0, st>>>(cells, band, rows, row0, n_rows, n_classes, n_off, d_out);
#undef KPOP_DISTILL_REDUCE_WAVE
    KPOP_LAUNCH_CHECK();
    if (clock) {
      KPOP_HIP(hipEventRecord(ev[2], st));
      KPOP_HIP(hipEventSynchronize(ev[2]));
      float ms = 0.f;
      KPOP_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
      c.distill_ms[0] += ms;
      KPOP_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
      c.distill_ms[1] += ms;
    }
  }
  if (clock) KPOP_HIP(hipEventRecord(ev[0], st));
  const uint32_t fit_blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kFitBlocks, (n_rows + 4095) / 4096));
  for (int centred = 0; centred < 2; ++centred) {
    distill_fit_sums_kernel<<<dim3(fit_blocks, 6), dim3(256), 0, st>>>(d_out, n_rows, centred, res, partial);
    KPOP_LAUNCH_CHECK();
    distill_fit_finish_kernel<<<dim3(1), dim3(64), 0, st>>>(partial, fit_blocks, n_rows, centred, res);
    KPOP_LAUNCH_CHECK();
  }
  distill_residual_kernel<<<dim3((uint32_t)std::min<uint64_t>(div_up(n_rows, 256), 1u << 16), 6), dim3(256), 0, st>>>(d_out, n_rows, res);
  KPOP_LAUNCH_CHECK();
  if (clock) {
    KPOP_HIP(hipEventRecord(ev[1], st));
    KPOP_HIP(hipEventSynchronize(ev[1]));
    float ms = 0.f;
    KPOP_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    c.distill_ms[2] = ms;
    for (auto &e : ev) (void)hipEventDestroy(e);
  }
  double fit_res[24];
  KPOP_HIP(hipMemcpyAsync(fit_res, res, sizeof(fit_res), hipMemcpyDeviceToHost, st));
  KPOP_HIP(hipStreamSynchronize(st));  // the permutation above came from this frame, and the fits go to the host
  if (fits_host)
    for (int f = 0; f < 6; ++f) {
      fits_host[2 * f] = fit_res[4 * f + 2];
      fits_host[2 * f + 1] = fit_res[4 * f + 3];
    }
  return KPOP_OK;
}

}  // namespace

}  // namespace kpop

using namespace kpop;

extern "C" uint64_t kpop_dev_counter_distill_workspace_bytes(uint32_t n_cols, uint64_t n_rows, uint32_t n_classes) {
  return distill_layout(n_cols, n_rows, n_classes).total;
}

extern "C" int kpop_dev_counter_distill(const int32_t *d_storage, uint64_t ld, uint32_t n_cols, uint64_t n_rows, const uint32_t *d_classes,
                                        uint32_t n_classes, void *d_workspace, double *d_out, double *fits_host, void *stream) {
  KPOP_TRY(require_init());
  KPOP_TRY(check_class_count(n_cols, n_classes, "kpop_dev_counter_distill"));
  if (!d_classes) KPOP_FAIL(KPOP_ERR_INVALID, "kpop_dev_counter_distill: classes is null");
  hipStream_t st = as_stream(stream);
  std::vector<uint32_t> classes(n_cols);
  KPOP_HIP(hipMemcpyAsync(classes.data(), d_classes, (uint64_t)n_cols * 4, hipMemcpyDeviceToHost, st));
  KPOP_HIP(hipStreamSynchronize(st));
  return distill_run(d_storage, ld, n_cols, n_rows, classes.data(), n_classes, d_workspace, d_out, fits_host, st, "kpop_dev_counter_distill");
}

extern "C" int kpop_counter_distill(const int32_t *const *columns, uint32_t n_cols, uint64_t n_rows, const uint32_t *classes,
                                    uint32_t n_classes, double *out, double *fits) {
  KPOP_TRY(require_init());
  KPOP_TRY(check_class_count(n_cols, n_classes, "kpop_counter_distill"));
  if (!classes || (n_rows && (!columns || !out))) KPOP_FAIL(KPOP_ERR_INVALID, "kpop_counter_distill: null argument");
  hipStream_t st = nullptr;
  DevBuf ds, dw, dout;
  uint64_t ld = kpop_dev_counter_ld(n_rows);
  if (n_rows) {
    KPOP_TRY(upload_columns(columns, n_cols, n_rows, ds, &ld, st));
    KPOP_TRY(dw.alloc(kpop_dev_counter_distill_workspace_bytes(n_cols, n_rows, n_classes)));
    KPOP_TRY(dout.alloc((uint64_t)KPOP_DISTILL_ROWS * n_rows * 8));
  }
  KPOP_TRY(distill_run(ds.as<int32_t>(), ld, n_cols, n_rows, classes, n_classes, dw.p, dout.as<double>(), fits, st, "kpop_counter_distill"));
  if (n_rows) {
    KPOP_HIP(hipMemcpyAsync(out, dout.p, (uint64_t)KPOP_DISTILL_ROWS * n_rows * 8, hipMemcpyDeviceToHost, st));
    KPOP_HIP(hipStreamSynchronize(st));
  }
  return KPOP_OK;
}

extern "C" int kpop_debug_distill_clocks(double *out_ms) {
  KPOP_TRY(require_init());
  if (!out_ms) KPOP_FAIL(KPOP_ERR_INVALID, "kpop_debug_distill_clocks: null argument");
  Context &c = ctx();
  for (int i = 0; i < 3; ++i) out_ms[i] = c.distill_ms[i];
  return KPOP_OK;
}
