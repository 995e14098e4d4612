// distance_routes.h -- what the distance and summary routes' files call of one another: distance.hip decides and launches, summary_large.hip,
// distance_mfma.hip and class_set.hip hold the kernels of their routes with the launchers, refset.hip / within.hip the resident set.  Every
// declaration once, default arguments here and nowhere else; the defining files include it, so a signature that drifts does not compile.
#pragma once
#include <type_traits>

#include "refset.h"
#include "summary_types.h"

namespace kpop {

// the three kinds of every entry point: f(K), K an integral_constant of the kind
template <class F>
static int by_kind(int kind, F &&f) {
  switch (kind) {
    case KPOP_EUCLIDEAN: return f(std::integral_constant<int, KPOP_EUCLIDEAN>{});
    case KPOP_COSINE: return f(std::integral_constant<int, KPOP_COSINE>{});
    default: return f(std::integral_constant<int, KPOP_MINKOWSKI>{});
  }
}

// the operands of a distance or a summary as the entry points take them (m1 x m2 rows of n_dims; work: the caller's workspace, needed when
// normalising); prep: the first operand is a resident set (refset.h) that brings its own norms and copies, nullptr otherwise
struct DistOperands {
  const double *m1;
  uint32_t r1;
  const double *m2;
  uint32_t r2, n_dims;
  const double *metric;
  double p;
  int normalize;
  void *work;
  hipStream_t st;
  kpop_refset *prep;
};

// distance_mfma.hip: every pair's distance as a tiled contraction on the f64 matrix cores
bool distance_mfma_applies(int kind, uint32_t r1, uint32_t r2, uint32_t n_dims);
int launch_distance_rowwise_mfma(int kind, const double *a, uint32_t r1, const double *b, uint32_t r2, uint32_t n_dims, const double *metric, double p, double *out,
                                 hipStream_t st, const double *n1, const double *n2, const double *s1, const double *s2);

// class_set.hip: many rows against a small set of classes, a row a lane
bool class_set_applies(int kind, uint32_t r1, uint32_t r2, uint32_t n_dims, uint64_t room_doubles);
int launch_class_set_distance(int kind, const double *m1, uint32_t r1, const double *norms1, double *n1_out, const double *m2, uint32_t r2, double *n2,
                              uint32_t n_dims, const double *metric, double p, bool divide, double *room, double *out, hipStream_t st);

// summary_large.hip
int launch_summary_large(const double *rows, uint32_t n_rows, uint32_t r1, uint32_t row0, const SummaryOut &out, hipStream_t st, void *scratch,
                         SummaryLists *lists = nullptr, bool plain_rows = false, const double *srow = nullptr, uint32_t srow_n = 0);
uint64_t summary_large_scratch_bytes(uint32_t n_rows, uint32_t r1);
bool summary_fused_applies(uint32_t r1, uint32_t keep_at_most);
uint32_t summary_fused_sample_rows(uint32_t r1);
uint64_t summary_fused_scratch_bytes(uint32_t n_rows, uint32_t r1);
uint64_t summary_select_scratch_bytes(uint32_t n_rows, uint32_t r1);
int launch_sample_gather(const double *a, uint32_t r1, uint32_t n_dims, uint32_t s, double *out, hipStream_t st);
int launch_summary_fused(int kind, const double *a, uint32_t r1, const double *b, uint32_t n_rows, uint32_t n_dims, const double *metric, double p,
                         const double *srow, uint32_t s, uint32_t row0, const SummaryOut &out, double *seg, void *scratch, hipStream_t st, const uint32_t **gate);
int launch_summary_failed_rows(const double *rows, uint32_t n_rows, uint32_t r1, uint32_t row0, const SummaryOut &out, void *scratch, hipStream_t st);
int launch_summary_flagged_rows(const double *rows, uint32_t n_rows, uint32_t r1, uint32_t row0, const SummaryOut &out, const void *flags, hipStream_t st);

// distance_mfma.hip: the large-reference summary's distances on the matrix cores, and what makes its results exact again
bool summary_mfma_applies(int kind, uint32_t r1, uint32_t n_dims, uint32_t keep_at_most, uint32_t max_neighbours);
uint64_t summary_mfma_scratch_bytes(uint32_t q, uint32_t r1, uint32_t n_dims);
int launch_mfma_reference_norms(const double *a, uint32_t r1, uint32_t n_dims, const double *metric, void *scratch, uint32_t q_room, hipStream_t st,
                                const double *na = nullptr, const double *s_raw = nullptr);
int launch_mfma_copy_reference_norms(const void *from, void *to, uint32_t r1, uint32_t n_dims, uint32_t q_room, hipStream_t st);
int launch_distance_rows_mfma(int kind, const double *a, uint32_t r1, const double *b, uint32_t q, uint32_t n_dims, const double *metric, double *rows,
                              void *scratch, uint32_t q_room, hipStream_t st, bool a_raw = false, const RefScalars *ref = nullptr);
int launch_summary_refine(int kind, const double *rows, const double *a, uint32_t r1, const double *b, uint32_t q, uint32_t n_dims, const double *metric,
                          double p, uint32_t row0, const SummaryOut &out, void *scratch, uint32_t q_room, hipStream_t st, const SummaryLists &lists,
                          const uint32_t **gate, const void **row_counts, const double *na = nullptr, const RefScalars *ref = nullptr);
// ... the same without distance rows: the summary's pass inside the contraction (summary_large.hip owns its scratch, distance_mfma.hip the pass)
bool summary_select_mfma_applies(uint32_t r1, uint32_t keep_at_most);
int launch_mfma_query_prep(const double *b, uint32_t q, uint32_t r1, uint32_t n_dims, const double *metric, void *scratch, uint32_t q_room, hipStream_t st);
int launch_rows_mfma_against(int kind, const double *as, const double *sas, uint32_t s, uint32_t q, uint32_t n_dims, double *rows, void *scratch, uint32_t q_room,
                             uint32_t r1, hipStream_t st, const double *ias = nullptr);
int launch_mfma_sample_scalars(const void *scratch, uint32_t q_room, uint32_t r1, uint32_t n_dims, uint32_t s, double *sas, double *ias, hipStream_t st);
int launch_summary_fused_mfma(int kind, const double *a, uint32_t r1, uint32_t n_rows, uint32_t n_dims, const double *srow, uint32_t s, uint32_t row0,
                              const SummaryOut &out, double *seg, uint32_t *seg_i, void *scratch, const void *mscratch, uint32_t q_room, hipStream_t st,
                              SummaryLists *lists, const RefScalars *ref = nullptr);
int launch_select_mfma(int kind, const double *a, uint32_t r1, uint32_t q, uint32_t n_dims, const void *mscratch, uint32_t q_room, const FusedThr *thr, double *seg,
                       uint32_t *seg_i, StripeRec *rec, double *part, RowCounts *cnt, uint32_t *nb_idx, double *nb_d, uint32_t n_stripes, hipStream_t st, const RefScalars *ref);
// ... kernels the resident set's lazily built pieces share with the unprepared call
int launch_row_sumsq(const double *x, uint32_t rows, uint32_t n_dims, const double *metric, double *out, hipStream_t st);
int launch_row_sumsq_max(const double *x, uint32_t rows, uint32_t n_dims, const double *metric, double *out, unsigned long long *smax, hipStream_t st);
int launch_gather_sample_scalars(const double *sa, const double *ia, uint32_t r1, uint32_t s, double *sas, double *ias, hipStream_t st);

}  // namespace kpop
