// refset.hip -- kpop_refset: the first operand of the distance entry points, resident in HBM with what does not depend on the
// query rows.
//
// The reference computes the norms of BOTH operands on every invocation (Base.get_normalizations, lib/Matrix.ml:42-76, called
// from get_distance_rowwise :191-266 and summarize_rowwise :691-766); a database that is queried again and again pays for a pass
// over all of it per batch.  A set keeps
//   built at creation / on append, one pass over the rows added (refset_prepare_kernel):
//     n1, s_raw   norms (0 -> 1, :67) and the sums before the scale -- row_norms_block, the body the unprepared call runs
//     ia, sa      1 / n and s_raw (1/n)^2, with their maximum: the matrix-core summary's scalars in their default form
//                 (reference_scales_kernel's arithmetic, distance_mfma.hip)
//   built by the first call that needs them, over the rows not yet covered:
//     div         rows / norm (the routes that go through prepare_operands)
//     sb          the other arithmetic of the sums of squares (row_sumsq_kernel over the operand the contraction reads), own maximum
//     smp ...     the evenly spaced sample of rows and its scalars (sized by the call's route; rebuilt after an append)
// Every piece comes out of the kernel the unprepared call would have run over the same row, so a call on a set returns that
// call's bits.  A piece made on one stream is followed by an event the other streams wait on: the query path never waits on the host.
// A set is used by one host thread at a time, and kpop_tune settings change only while no call on it is in flight.
#include <algorithm>
#include <new>

#include "common.h"
#include "distance_routes.h"
#include "refset_call.h"
#include "row_norms.h"

namespace kpop {

// rows [0, rows) of `m` (the caller passes the range's first row): norm, raw sum, reciprocal, scaled sum, and the running maximum of
// the scaled sums -- ONE pass over the rows; the 64 threads that hold a row's sum carry on with its scalars
template <int KIND>
__global__ __launch_bounds__(256) void refset_prepare_kernel(const double *__restrict__ m, uint32_t rows, uint32_t n_dims,
                                                             const double *__restrict__ metric, double p, double *norms, double *s_raw,
                                                             double *ia, double *sa, unsigned long long *smax) {
  row_norms_block<KIND>(m, rows, n_dims, metric, p, norms, nullptr, blockIdx.x, s_raw);
  if (KIND == KPOP_MINKOWSKI) return;  // (no contraction for |x|^p: nothing reads the scalars)
  __shared__ unsigned long long s_max;
  if (threadIdx.x == 0) s_max = 0;
  __syncthreads();
  const uint32_t row = blockIdx.x * kNormRows + threadIdx.x;
  if (threadIdx.x < kNormRows && row < rows) {
    // (reference_scales_kernel's operations on the values this thread has just written)
    const double r = 1.0 / norms[row], v = s_raw[row] * r * r;
    ia[row] = r;
    sa[row] = v;
    atomicMax(&s_max, (unsigned long long)__double_as_longlong(v));  // (not negative: bit patterns order as the values do)
  }
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(smax, s_max);
}

// out = m / norm, a wavefront a row (the quotients of row_norms_block's second half and of lib/Matrix.ml:248)
__global__ __launch_bounds__(256) void refset_divide_kernel(const double *__restrict__ m, uint32_t rows, uint32_t n_dims, const double *__restrict__ norms,
                                                            double *__restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += gridDim.x * 4) {
    const double nv = norms[row];
    const double *src = m + (uint64_t)row * n_dims;
    double *dst = out + (uint64_t)row * n_dims;
    for (uint32_t c = lane; c < n_dims; c += 64) dst[c] = src[c] / nv;
  }
}

static int prepare_range(kpop_refset *rs, uint32_t lo, uint32_t hi, hipStream_t st) {
  if (rs->normalize && hi > lo) {
    const uint32_t n = hi - lo;
    const double *m = rs->rows + (uint64_t)lo * rs->n_dims;
    const dim3 grid(div_up(n, kNormRows)), block(256);
    switch (rs->kind) {
      case KPOP_EUCLIDEAN:
        refset_prepare_kernel<KPOP_EUCLIDEAN><<<grid, block, 0, st>>>(m, n, rs->n_dims, rs->metric, rs->p, rs->n1 + lo, rs->s_raw + lo, rs->ia + lo, rs->sa + lo, rs->smax);
        break;
      case KPOP_COSINE:
        refset_prepare_kernel<KPOP_COSINE><<<grid, block, 0, st>>>(m, n, rs->n_dims, rs->metric, rs->p, rs->n1 + lo, rs->s_raw + lo, rs->ia + lo, rs->sa + lo, rs->smax);
        break;
      default:
        refset_prepare_kernel<KPOP_MINKOWSKI><<<grid, block, 0, st>>>(m, n, rs->n_dims, rs->metric, rs->p, rs->n1 + lo, rs->s_raw + lo, rs->ia + lo, rs->sa + lo, rs->smax);
        break;
    }
    KPOP_LAUNCH_CHECK();
  }
  KPOP_HIP(hipEventRecord(rs->ready, st));
  return 0;
}

static int set_alloc(kpop_refset *rs, uint64_t bytes, void **out) {
  KPOP_HIP(hipMalloc(out, bytes ? bytes : 8));
  rs->device_bytes += bytes ? bytes : 8;
  return 0;
}
template <class T>
static int set_alloc(kpop_refset *rs, uint64_t bytes, T **out) {
  void *p = nullptr;
  KPOP_TRY(set_alloc(rs, bytes, &p));
  *out = reinterpret_cast<T *>(p);
  return 0;
}

static void destroy(kpop_refset *rs) {
  if (!rs) return;
  if (!rs->borrowed) {
    (void)hipFree(const_cast<double *>(rs->rows));
    (void)hipFree(const_cast<double *>(rs->metric));
  }
  void *mine[] = {rs->n1, rs->s_raw, rs->ia, rs->sa, rs->smax, rs->div, rs->sb, rs->smp};
  for (void *q : mine)
    if (q) (void)hipFree(q);
  hipEvent_t ev[] = {rs->ready, rs->div_ready, rs->sb_ready, rs->smp_ready};
  for (hipEvent_t e : ev)
    if (e) (void)hipEventDestroy(e);
  delete rs;
}

static int check_handle(const kpop_refset *rs, const char *who) {
  KPOP_TRY(require_init());
  if (!rs) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null handle", who);
  if (rs->slot != current_slot() || rs->generation != ctx().generation)
    KPOP_FAIL(KPOP_ERR_INVALID, "%s: the set belongs to device slot %d, the calling thread works on slot %d", who, rs->slot, current_slot());
  return 0;
}

int refset_check_handle(const kpop_refset *rs, const char *who) { return check_handle(rs, who); }  // (within.hip, clusters.hip)

// the common part of create and wrap: arguments, the handle, the per-row arrays (rows and metric are the caller's business)
static int make_set(const char *who, uint32_t r1, uint32_t n_dims, int kind, double p, int normalize, uint32_t capacity, kpop_refset **out) {
  if (kind != KPOP_EUCLIDEAN && kind != KPOP_COSINE && kind != KPOP_MINKOWSKI) KPOP_FAIL(KPOP_ERR_INVALID, "%s: unknown distance kind %d", who, kind);
  if (kind == KPOP_MINKOWSKI && !(p >= 0.0)) KPOP_FAIL(KPOP_ERR_INVALID, "%s: negative Minkowski power", who);  // lib/Space.ml:222-223
  if (n_dims == 0) KPOP_FAIL(KPOP_ERR_INVALID, "%s: n_dims must be positive", who);
  if (n_dims >= 32768) KPOP_FAIL(KPOP_ERR_UNSUPPORTED, "%s: rows of 32768 dimensions or more go through kpop_dev_distance_rowwise", who);
  if (capacity < r1) KPOP_FAIL(KPOP_ERR_INVALID, "%s: capacity_rows (%u) below the number of rows (%u)", who, capacity, r1);
  kpop_refset *rs = new (std::nothrow) kpop_refset();
  if (!rs) KPOP_FAIL(KPOP_ERR_HIP, "%s: out of host memory", who);
  rs->slot = current_slot();
  rs->generation = ctx().generation;
  rs->r1 = r1;
  rs->n_dims = n_dims;
  rs->capacity = capacity;
  rs->kind = kind;
  rs->p = p;
  rs->normalize = normalize ? 1 : 0;
  *out = rs;
  KPOP_HIP(hipEventCreateWithFlags(&rs->ready, hipEventDisableTiming));
  KPOP_HIP(hipEventCreateWithFlags(&rs->div_ready, hipEventDisableTiming));
  KPOP_HIP(hipEventCreateWithFlags(&rs->sb_ready, hipEventDisableTiming));
  KPOP_HIP(hipEventCreateWithFlags(&rs->smp_ready, hipEventDisableTiming));
  KPOP_TRY(set_alloc(rs, 512, &rs->smax));
  KPOP_HIP(hipMemset(rs->smax, 0, 512));
  if (rs->normalize) {
    const uint64_t per_row = (uint64_t)capacity * 8;
    KPOP_TRY(set_alloc(rs, per_row, &rs->n1));
    KPOP_TRY(set_alloc(rs, per_row, &rs->s_raw));
    KPOP_TRY(set_alloc(rs, per_row, &rs->ia));
    KPOP_TRY(set_alloc(rs, per_row, &rs->sa));
  }
  return 0;
}

}  // namespace kpop

using namespace kpop;

int kpop_refset::prepared(hipStream_t st) {
  KPOP_HIP(hipStreamWaitEvent(st, ready, 0));
  return 0;
}

int kpop_refset::divided(hipStream_t st, const double **a) {
  if (!normalize) {
    *a = rows;
    return 0;
  }
  if (!div) KPOP_TRY(set_alloc(this, (uint64_t)capacity * n_dims * 8, &div));
  if (div_rows < r1) {  // the rows added since the copy was last brought up to date
    const uint32_t n = r1 - div_rows;
    KPOP_HIP(hipStreamWaitEvent(st, ready, 0));
    refset_divide_kernel<<<dim3(std::min(div_up(n, 4), 65536u)), dim3(256), 0, st>>>(rows + (uint64_t)div_rows * n_dims, n, n_dims, n1 + div_rows,
                                                                                  div + (uint64_t)div_rows * n_dims);
    KPOP_LAUNCH_CHECK();
    KPOP_HIP(hipEventRecord(div_ready, st));
    div_rows = r1;
  }
  KPOP_HIP(hipStreamWaitEvent(st, div_ready, 0));
  *a = div;
  return 0;
}

int kpop_refset::scalars_default(hipStream_t st, RefScalars *out) {
  KPOP_HIP(hipStreamWaitEvent(st, ready, 0));
  out->sa = sa;
  out->ia = ia;
  out->smax = smax;
  return 0;
}

int kpop_refset::scalars_of(const double *a, hipStream_t st, RefScalars *out) {
  unsigned long long *smax_b = smax + 32;
  if (!sb) KPOP_TRY(set_alloc(this, (uint64_t)capacity * 8, &sb));
  if (sb_of != a) {  // (a set's operand is one and the same for its life: the first call)
    KPOP_HIP(hipMemsetAsync(smax_b, 0, 256, st));
    sb_rows = 0;
    sb_of = a;
  }
  if (sb_rows < r1) {
    KPOP_HIP(hipStreamWaitEvent(st, sb_ready, 0));  // (the maximum is a running one: after whoever extended it last)
    KPOP_TRY(launch_row_sumsq_max(a + (uint64_t)sb_rows * n_dims, r1 - sb_rows, n_dims, metric, sb + sb_rows, smax_b, st));
    KPOP_HIP(hipEventRecord(sb_ready, st));
    sb_rows = r1;
  }
  KPOP_HIP(hipStreamWaitEvent(st, sb_ready, 0));
  out->sa = sb;
  out->ia = nullptr;
  out->smax = smax_b;
  return 0;
}

int kpop_refset::sample(const double *a, uint32_t s, int mode, const RefScalars *from, hipStream_t st, const double **a_s, const double **sa_s,
                        const double **ia_s) {
  const double *sa_from = (mode == kSampleGathered && from) ? from->sa : nullptr;
  const double *ia_from = (mode == kSampleGathered && from) ? from->ia : nullptr;
  const uint64_t rows_bytes = ((uint64_t)s * n_dims * 8 + 255) & ~255ull, sc_bytes = ((uint64_t)s * 8 + 255) & ~255ull;
  if (!(smp_mode == mode && smp_rows == s && smp_r1 == r1 && smp_of == a && smp_sa_of == sa_from)) {
    // another size, another route, or rows appended: made again (a change of route with calls of the old one in flight is the one
    // place that waits for the device -- the old sample may still be read)
    if (smp_mode != -1) KPOP_HIP(hipDeviceSynchronize());
    const uint64_t need = rows_bytes + 2 * sc_bytes;
    if (smp_bytes < need) {
      if (smp) {
        KPOP_HIP(hipFree(smp));
        device_bytes -= smp_bytes;
        smp = nullptr;
        smp_bytes = 0;
      }
      KPOP_TRY(set_alloc(this, need, &smp));
      smp_bytes = need;
    }
    smp_sa = reinterpret_cast<double *>(reinterpret_cast<char *>(smp) + rows_bytes);
    smp_ia = reinterpret_cast<double *>(reinterpret_cast<char *>(smp) + rows_bytes + sc_bytes);
    smp_mode = -1;
    if (s) KPOP_TRY(launch_sample_gather(a, r1, n_dims, s, smp, st));
    if (s && mode == kSampleGathered) KPOP_TRY(launch_gather_sample_scalars(sa_from, ia_from, r1, s, smp_sa, ia_from ? smp_ia : nullptr, st));
    if (s && mode == kSampleSumsq) KPOP_TRY(launch_row_sumsq(smp, s, n_dims, metric, smp_sa, st));
    KPOP_HIP(hipEventRecord(smp_ready, st));
    smp_mode = mode;
    smp_rows = s;
    smp_r1 = r1;
    smp_of = a;
    smp_sa_of = sa_from;
  }
  KPOP_HIP(hipStreamWaitEvent(st, smp_ready, 0));
  *a_s = smp;
  if (sa_s) *sa_s = smp_sa;
  if (ia_s) *ia_s = ia_from ? smp_ia : nullptr;
  return 0;
}

extern "C" int kpop_refset_create(const double *m1, uint32_t r1, uint32_t n_dims, const double *metric, int kind, double p, int normalize,
                                  uint32_t capacity_rows, kpop_refset **out) {
  KPOP_TRY(require_init());
  if (!out || !metric || (r1 && !m1)) KPOP_FAIL(KPOP_ERR_INVALID, "kpop_refset_create: null argument");
  *out = nullptr;
  kpop_refset *rs = nullptr;
  auto body = [&]() -> int {
    KPOP_TRY(make_set("kpop_refset_create", r1, n_dims, kind, p, normalize, capacity_rows ? capacity_rows : r1, &rs));
    double *d_rows = nullptr, *d_metric = nullptr;
    KPOP_TRY(set_alloc(rs, (uint64_t)rs->capacity * n_dims * 8, &d_rows));
    rs->rows = d_rows;
    KPOP_TRY(set_alloc(rs, (uint64_t)n_dims * 8, &d_metric));
    rs->metric = d_metric;
    if (r1) KPOP_HIP(hipMemcpy(d_rows, m1, (uint64_t)r1 * n_dims * 8, hipMemcpyHostToDevice));
    KPOP_HIP(hipMemcpy(d_metric, metric, (uint64_t)n_dims * 8, hipMemcpyHostToDevice));
    KPOP_TRY(prepare_range(rs, 0, r1, nullptr));
    KPOP_HIP(hipStreamSynchronize(nullptr));
    return 0;
  };
  const int rc = body();
  if (rc) {
    destroy(rs);
    return rc;
  }
  *out = rs;
  return KPOP_OK;
}

extern "C" int kpop_dev_refset_wrap(const double *d_m1, uint32_t r1, uint32_t n_dims, const double *d_metric, int kind, double p, int normalize,
                                    void *stream, kpop_refset **out) {
  KPOP_TRY(require_init());
  if (!out || !d_metric || (r1 && !d_m1)) KPOP_FAIL(KPOP_ERR_INVALID, "kpop_dev_refset_wrap: null argument");
  *out = nullptr;
  kpop_refset *rs = nullptr;
  auto body = [&]() -> int {
    KPOP_TRY(make_set("kpop_dev_refset_wrap", r1, n_dims, kind, p, normalize, r1, &rs));
    rs->borrowed = true;
    rs->rows = d_m1;
    rs->metric = d_metric;
    KPOP_TRY(prepare_range(rs, 0, r1, as_stream(stream)));
    KPOP_HIP(hipStreamSynchronize(as_stream(stream)));
    return 0;
  };
  const int rc = body();
  if (rc) {
    if (rs) rs->borrowed = true;  // (never the caller's arrays)
    destroy(rs);
    return rc;
  }
  *out = rs;
  return KPOP_OK;
}

extern "C" int kpop_refset_append(kpop_refset *rs, const double *rows, uint32_t n_rows) {
  KPOP_TRY(check_handle(rs, "kpop_refset_append"));
  if (rs->borrowed) KPOP_FAIL(KPOP_ERR_INVALID, "kpop_refset_append: the set wraps the caller's rows (kpop_dev_refset_wrap) and cannot grow");
  if (n_rows == 0) return KPOP_OK;
  if (!rows) KPOP_FAIL(KPOP_ERR_INVALID, "kpop_refset_append: null argument");
  if ((uint64_t)rs->r1 + n_rows > rs->capacity)
    KPOP_FAIL(KPOP_ERR_CAPACITY, "kpop_refset_append: %u rows and %u more exceed the capacity of %u", rs->r1, n_rows, rs->capacity);
  KPOP_HIP(hipDeviceSynchronize());  // (calls in flight read the arrays that grow)
  KPOP_HIP(hipMemcpy(const_cast<double *>(rs->rows) + (uint64_t)rs->r1 * rs->n_dims, rows, (uint64_t)n_rows * rs->n_dims * 8, hipMemcpyHostToDevice));
  KPOP_TRY(prepare_range(rs, rs->r1, rs->r1 + n_rows, nullptr));  // the new rows only
  KPOP_HIP(hipStreamSynchronize(nullptr));
  rs->r1 += n_rows;
  rs->smp_mode = -1;  // the sample's rows are spaced by r1: made again by the next call that wants one
  return KPOP_OK;
}

extern "C" int kpop_refset_info(const kpop_refset *rs, uint32_t *r1, uint32_t *n_dims, uint32_t *capacity_rows, uint64_t *device_bytes) {
  if (!rs) KPOP_FAIL(KPOP_ERR_INVALID, "kpop_refset_info: null handle");
  if (r1) *r1 = rs->r1;
  if (n_dims) *n_dims = rs->n_dims;
  if (capacity_rows) *capacity_rows = rs->capacity;
  if (device_bytes) *device_bytes = rs->device_bytes;
  return KPOP_OK;
}

extern "C" int kpop_refset_free(kpop_refset *rs) {
  if (!rs) return KPOP_OK;
  KPOP_TRY(check_handle(rs, "kpop_refset_free"));
  KPOP_HIP(hipDeviceSynchronize());
  destroy(rs);
  return KPOP_OK;
}

extern "C" uint64_t kpop_dev_refset_workspace_bytes(const kpop_refset *rs, uint32_t r2) {
  if (!rs) return 0;
  return ((uint64_t)r2 + (uint64_t)r2 * rs->n_dims) * sizeof(double) + 64;  // the query rows' norms and their divided copy
}

extern "C" int kpop_dev_refset_distance_rowwise(kpop_refset *rs, const double *d_m2, uint32_t r2, void *d_work, double *d_out, void *stream) {
  KPOP_TRY(check_handle(rs, "kpop_dev_refset_distance_rowwise"));
  return refset_dev_rowwise(rs, d_m2, r2, d_work, d_out, as_stream(stream));
}

extern "C" int kpop_dev_refset_distance_summary(kpop_refset *rs, const double *d_m2, uint32_t r2, uint32_t keep_at_most, uint32_t max_neighbours,
                                                void *d_work, double *d_out_stats, uint32_t *d_out_n, uint32_t *d_out_idx, double *d_out_dist,
                                                double *d_out_z, void *stream) {
  KPOP_TRY(check_handle(rs, "kpop_dev_refset_distance_summary"));
  return refset_dev_summary(rs, d_m2, r2, d_work, SummaryOut{d_out_stats, d_out_n, d_out_idx, d_out_dist, d_out_z, keep_at_most, max_neighbours}, as_stream(stream));
}

// ---------------------------------------------------------------------------
// host-buffer entry points: the query rows go up, the answers come down; the set stays where it is
// ---------------------------------------------------------------------------
extern "C" int kpop_refset_distance_rowwise(kpop_refset *rs, const double *m2, uint32_t r2, double *out) {
  KPOP_TRY(check_handle(rs, "kpop_refset_distance_rowwise"));
  ArenaScope scratch;
  if (rs->r1 == 0 || r2 == 0) return KPOP_OK;
  if (!m2 || !out) KPOP_FAIL(KPOP_ERR_INVALID, "kpop_refset_distance_rowwise: null argument");
  HostCall h;
  const double *d2 = h.in(m2, (uint64_t)r2 * rs->n_dims);
  void *dw = h.work(kpop_dev_refset_workspace_bytes(rs, r2));
  double *dout = h.out(out, (uint64_t)rs->r1 * r2);
  KPOP_TRY(h.upload());
  KPOP_TRY(refset_dev_rowwise(rs, d2, r2, dw, dout, h.st));
  return h.finish();
}

extern "C" int kpop_refset_distance_summary(kpop_refset *rs, const double *m2, uint32_t r2, uint32_t keep_at_most, uint32_t max_neighbours,
                                            double *out_stats, uint32_t *out_n, uint32_t *out_idx, double *out_dist, double *out_z) {
  KPOP_TRY(check_handle(rs, "kpop_refset_distance_summary"));
  ArenaScope scratch;
  if (r2 == 0) return KPOP_OK;
  if (!m2 || !out_stats || !out_n) KPOP_FAIL(KPOP_ERR_INVALID, "kpop_refset_distance_summary: null argument");
  const SummaryOut host{out_stats, out_n, out_idx, out_dist, out_z, keep_at_most, max_neighbours};
  HostCall h;
  const double *d2 = h.in(m2, (uint64_t)r2 * rs->n_dims);
  void *dw = h.work(kpop_dev_refset_workspace_bytes(rs, r2));
  const SummaryOut dev = summary_stage(h, r2, host);
  KPOP_TRY(h.upload());
  KPOP_TRY(refset_dev_summary(rs, d2, r2, dw, dev, h.st));
  KPOP_TRY(h.finish());
  return refset_fill_long_lists(rs, d2, r2, host, h.st);
}
