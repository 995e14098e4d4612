// refset.h -- kpop_refset: a first operand of the distance entry points that stays in HBM with everything about it that does
// not depend on the query rows (refset.hip).  rowwise_impl / summary_impl / summary_large_impl (distance.hip) take a pointer to
// one as the optional "prepared first operand" of their operands (DistOperands::prep, distance_routes.h) and ask it for the pieces their
// route would otherwise compute.
#pragma once
#include "common.h"
#include "summary_types.h"

namespace kpop {

// the reference rows' scalars of the matrix-core routes, wherever they live (the call's scratch, or a set)
struct RefScalars {
  const double *sa = nullptr, *ia = nullptr;
  const unsigned long long *smax = nullptr;
};

// how the sums of squares of a sample of the reference rows are made (summary_large_impl)
enum SampleScalars {
  kSampleRowsOnly = 0,  // the vector-pipe routes: rows alone
  kSampleGathered = 1,  // out of the whole set's scalars (gather_sample_scalars_kernel)
  kSampleSumsq = 2      // row_sumsq_kernel over the gathered rows (the summary_mfma = 2 form)
};

}  // namespace kpop

struct kpop_refset {
  // what the caller said
  int slot = 0;
  uint32_t generation = 0;
  uint32_t r1 = 0, n_dims = 0, capacity = 0;
  int kind = 0, normalize = 0;
  double p = 2.0;
  bool borrowed = false;          // kpop_dev_refset_wrap: rows and metric are the caller's
  const double *rows = nullptr;   // [capacity][n_dims]
  const double *metric = nullptr; // [n_dims]
  // built at creation and on append, for the rows added (normalize set): norms (0 -> 1), the sums before the scale, and the
  // matrix-core routes' scalars in their default form (reciprocal norms, sums of squares of the divided rows, their maximum)
  double *n1 = nullptr, *s_raw = nullptr, *ia = nullptr, *sa = nullptr;
  unsigned long long *smax = nullptr;  // [0] the default form's, [32] the second form's (256 bytes apart)
  hipEvent_t ready = nullptr;          // after the last preparation pass
  // built on the first call that needs them, over the rows not yet covered
  double *div = nullptr;  // rows / norm
  uint32_t div_rows = 0;
  hipEvent_t div_ready = nullptr;
  double *sb = nullptr;  // the second form of the sums of squares: row_sumsq_kernel over the operand the contraction reads
  uint32_t sb_rows = 0;
  const double *sb_of = nullptr;
  hipEvent_t sb_ready = nullptr;
  // the evenly spaced sample of rows with its scalars; stale after an append or under another route
  double *smp = nullptr, *smp_sa = nullptr, *smp_ia = nullptr;
  uint64_t smp_bytes = 0;
  uint32_t smp_rows = 0, smp_r1 = 0;
  int smp_mode = -1;
  const double *smp_of = nullptr, *smp_sa_of = nullptr;
  hipEvent_t smp_ready = nullptr;
  uint64_t device_bytes = 0;

  // (each: enqueue on `st` what is missing, make `st` wait for what another stream built)
  int prepared(hipStream_t st);                        // n1, s_raw and the default scalars are there for st
  int divided(hipStream_t st, const double **a);       // rows / norm
  int scalars_default(hipStream_t st, kpop::RefScalars *out);
  int scalars_of(const double *a, hipStream_t st, kpop::RefScalars *out);  // a: rows or div
  int sample(const double *a, uint32_t s, int mode, const kpop::RefScalars *from, hipStream_t st, const double **a_s, const double **sa_s,
             const double **ia_s);
};

namespace kpop {
// distance.hip: the device entry points' bodies with a prepared first operand
int refset_dev_rowwise(kpop_refset *rs, const double *d_m2, uint32_t r2, void *d_work, double *d_out, hipStream_t st);
int refset_dev_summary(kpop_refset *rs, const double *d_m2, uint32_t r2, void *d_work, const SummaryOut &out, hipStream_t st);
int refset_fill_long_lists(kpop_refset *rs, const double *d_m2, uint32_t r2, const SummaryOut &out, hipStream_t st);  // (out: host buffers)
int refset_query_norms(const kpop_refset *rs, const double *d_m2, uint32_t r2, double *n2, double *b_div, hipStream_t st);
// refset.hip: the handle belongs to the calling thread's device slot
int refset_check_handle(const kpop_refset *rs, const char *who);
}  // namespace kpop
