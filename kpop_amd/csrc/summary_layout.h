// summary_layout.h -- the library workspace of the large-reference summary's routes (summary_large_impl, distance.hip), each route's
// layout written ONCE: run over a null base it sizes the workspace, over the real base it hands out the pointers.  Host arithmetic
// alone, nothing of the GPU runtime: tests/host/summary_layout_check.cpp runs it as it is.
#pragma once
#include <cstdint>

namespace kpop {

// regions one after the other, each rounded up to 256 bytes
struct Carver {
  char *base;
  uint64_t off = 0;
  explicit Carver(void *b) : base(static_cast<char *>(b)) {}
  template <class T>
  T *take(uint64_t count) {
    char *at = base ? base + off : nullptr;
    off += (count * sizeof(T) + 255) & ~255ull;
    return reinterpret_cast<T *>(at);
  }
  uint64_t bytes() const { return off; }
};

// The matrix-core routes.  A LANE is what one chain of a batch's kernels works in: the batch's distance rows (under `select` the candidates'
// segments, a row rounded up to whole stripes of 2,048, and their columns in seg_i), the summary's scratch, the contraction's, and
// the batch's distances to the sample.  Once a call: the sample of the reference rows, its sums of squares and its norms' reciprocals.
struct MfmaShape {
  uint32_t chunk, r1, n_dims, s_rows, n_lanes;
  bool select;
  uint64_t sum_scratch, mfma_scratch;  // what the summary's kernels and the contraction ask for, for `chunk` query rows
};
struct MfmaWork {
  struct Lane {
    double *rows;
    uint32_t *seg_i;
    void *scratch, *mscratch;
    double *srow;
  } lane[2];
  double *a_s, *sa_s, *ia_s;
  uint64_t bytes;
};
inline MfmaWork carve_summary_mfma(void *base, const MfmaShape &s) {
  Carver c(base);
  MfmaWork w{};
  const uint64_t r1_seg = s.select ? (((uint64_t)s.r1 + 2047) & ~2047ull) : s.r1;
  for (uint32_t l = 0; l < s.n_lanes; ++l) {
    w.lane[l].rows = c.take<double>((uint64_t)s.chunk * r1_seg);
    w.lane[l].seg_i = c.take<uint32_t>(s.select ? (uint64_t)s.chunk * r1_seg : 0);
    w.lane[l].scratch = c.take<char>(s.sum_scratch + 256);  // (256: the kernels' launchers align the scratch themselves)
    w.lane[l].mscratch = c.take<char>(s.mfma_scratch + 256);
  }
  w.a_s = c.take<double>((uint64_t)s.s_rows * s.n_dims);
  w.sa_s = c.take<double>(s.s_rows);
  w.ia_s = c.take<double>(s.s_rows);
  for (uint32_t l = 0; l < s.n_lanes; ++l) w.lane[l].srow = c.take<double>((uint64_t)s.chunk * s.s_rows);  // (last: with one lane every region is where it always was)
  w.bytes = c.bytes() + 512;
  return w;
}

// The vector-pipe route without distance rows (kpop_tune("summary2", 2)): per chunk of query rows the candidates' segments (the room
// distance rows would take), the sample of the reference rows, the distances to it, and the lists.
struct FusedWork {
  double *seg, *a_s, *srow;
  void *scratch;
  uint64_t bytes;
};
inline FusedWork carve_summary_fused(void *base, uint32_t chunk, uint32_t r1, uint32_t n_dims, uint32_t s, uint64_t fused_scratch) {
  Carver c(base);
  FusedWork w{};
  w.seg = c.take<double>((uint64_t)chunk * r1);
  w.a_s = c.take<double>((uint64_t)s * n_dims);
  w.srow = c.take<double>((uint64_t)chunk * s);
  w.scratch = c.take<char>(fused_scratch);  // (summary_fused_scratch_bytes: a multiple of 256 already -- carve_fused rounds every list -- so the rounding here adds nothing)
  w.bytes = c.bytes();
  return w;
}

// The plain chunked route: a chunk's distance rows, the summary's scratch, and -- s_rows > 0 -- the sample and the distances to it.
struct ChunkedWork {
  double *rows;
  void *scratch;
  double *a_s, *srow;
  uint64_t bytes;
};
inline ChunkedWork carve_summary_chunked(void *base, uint32_t chunk, uint32_t r1, uint32_t n_dims, uint32_t s_rows, uint64_t sum_scratch) {
  Carver c(base);
  ChunkedWork w{};
  w.rows = c.take<double>((uint64_t)chunk * r1);
  w.scratch = c.take<char>(sum_scratch + 256);
  w.a_s = c.take<double>((uint64_t)s_rows * n_dims);
  w.srow = c.take<double>((uint64_t)chunk * s_rows);
  w.bytes = c.bytes() + 256;
  return w;
}

}  // namespace kpop
