// summary_layout_check -- the workspace layouts of the large-reference summary (kpop_amd/csrc/summary_layout.h) as host code: every
// route's layout over a null base (the size handed to the workspace) and over a made-up base (the pointers).  Every pointer 256-byte
// aligned, no two regions overlapping, the last one ending inside the size, and the size no larger than the sums of byte counts the
// routes were written with before the layouts had a file of their own (restated below as the expectation: a larger request would be
// another allocation on a warm workspace).  Nothing of the GPU runtime; tests/test_host_layout.py builds it with the sanitizers.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../kpop_amd/csrc/summary_layout.h"
#include "../../kpop_amd/csrc/summary_types.h"

using namespace kpop;

static int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      ++failures;                                 \
      std::printf("FAILED %s: ", #cond);          \
      std::printf(__VA_ARGS__);                   \
      std::printf("\n");                          \
    }                                             \
  } while (0)

// what the kernels' launchers ask for (summary_large.hip, distance_mfma.hip), restated
static uint64_t r256(uint64_t x) { return (x + 255) & ~255ull; }
static uint32_t cand_cap_for(uint32_t r1) { return std::max<uint32_t>(65536u, ((r1 / 16 + 4095u) & ~4095u)); }
static uint32_t fused_cand_cap(uint32_t r1) { return (r1 / 4 + 4095u) & ~4095u; }
static uint64_t large_scratch(uint32_t n_rows, uint32_t r1) {
  const uint64_t n_slices = (r1 + 32768u - 1) / 32768u;
  return (uint64_t)n_rows * (sizeof(RowInfo) + sizeof(RowCounts) + sizeof(FusedThr) + (uint64_t)std::max(cand_cap_for(r1), fused_cand_cap(r1)) * 12 + (uint64_t)kNbCap * 12 + n_slices * 16) + 8192;
}
static uint64_t fused_scratch(uint32_t n_rows, uint32_t r1, uint32_t stripe) {
  const uint64_t n_stripes = stripe == kStripe ? (r1 + kStripe - 1) / kStripe : (uint64_t)(kStripe / stripe) * ((r1 + kStripe - 1) / kStripe);
  return 256 + r256((uint64_t)n_rows * sizeof(RowInfo)) + r256((uint64_t)n_rows * sizeof(RowCounts)) + r256((uint64_t)n_rows * sizeof(FusedThr)) +
         r256((uint64_t)n_rows * n_stripes * sizeof(StripeRec)) + r256((uint64_t)n_rows * n_stripes * 16) + r256((uint64_t)n_rows * n_stripes * 4) + r256((uint64_t)n_rows * kNbCap * 8) +
         r256((uint64_t)n_rows * kNbCap * 4) + r256((uint64_t)n_rows * fused_cand_cap(r1) * 8) + r256((uint64_t)n_rows * fused_cand_cap(r1) * 4) + 256;
}
static uint64_t mfma_scratch(uint32_t q, uint32_t r1, uint32_t n_dims) {
  return r256((uint64_t)r1 * 8) + r256((uint64_t)q * n_dims * 8) + r256((uint64_t)r1 * 8) + r256((uint64_t)q * 8) + 256 + r256((uint64_t)q * 12 * 4) + 256;
}
static uint32_t sample_rows(uint32_t r1) { return std::min<uint32_t>(65536, r1); }

using Regions = std::vector<std::pair<const void *, uint64_t>>;  // (pointer, bytes in use)
static char *const kBase = reinterpret_cast<char *>(uintptr_t(1) << 40);

static void check_regions(const char *what, uint32_t r1, uint32_t r2, uint32_t n_dims, Regions regions, uint64_t bytes, uint64_t sized, uint64_t expected) {
  CHECK(bytes == sized, "%s %u x %u x %u: %llu bytes over the base, %llu over a null one", what, r1, r2, n_dims, (unsigned long long)bytes, (unsigned long long)sized);
  CHECK(bytes <= expected, "%s %u x %u x %u: %llu bytes, %llu before", what, r1, r2, n_dims, (unsigned long long)bytes, (unsigned long long)expected);
  std::sort(regions.begin(), regions.end());
  const char *end = kBase;
  for (const auto &r : regions) {
    const char *at = static_cast<const char *>(r.first);
    CHECK((reinterpret_cast<uintptr_t>(at) & 255) == 0, "%s %u x %u x %u: a region at +%lld", what, r1, r2, n_dims, (long long)(at - kBase));
    CHECK(at >= end, "%s %u x %u x %u: a region at +%lld begins before +%lld", what, r1, r2, n_dims, (long long)(at - kBase), (long long)(end - kBase));
    if (r.second) end = at + r.second;
  }
  CHECK(end <= kBase + bytes, "%s %u x %u x %u: the last region ends at +%lld of %llu", what, r1, r2, n_dims, (long long)(end - kBase), (unsigned long long)bytes);
}

static void check_mfma(uint32_t r1, uint32_t r2, uint32_t n_dims, bool select, bool sample, bool lanes2) {
  const uint64_t budget = 4096ull << 20;
  uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(r2, 2 * budget / ((uint64_t)r1 * 8)));
  if (chunk > 128) chunk = chunk / 128 * 128;
  const bool two = !select && lanes2 && r2 >= 512 && chunk >= 512;
  if (two) chunk = 256;
  const bool row_sample = !select && sample;
  const uint32_t s_rows = select ? sample_rows(r1) : row_sample ? (n_dims > 128 ? std::min(32768u, sample_rows(r1)) : sample_rows(r1)) : 0;
  const uint64_t sum_scratch = std::max(large_scratch(chunk, r1), select ? fused_scratch(chunk, r1, kStripe / 4) : 0), m_scratch = mfma_scratch(chunk, r1, n_dims);
  // as the routes were written before
  const uint64_t r1_seg = select ? (((uint64_t)r1 + 2047) & ~2047ull) : r1;
  const uint64_t row_bytes = r256((uint64_t)chunk * r1_seg * 8), segi_bytes = select ? r256((uint64_t)chunk * r1_seg * 4) : 0;
  const uint64_t sum_bytes = (sum_scratch + 511) & ~255ull, m_bytes = (m_scratch + 511) & ~255ull;
  const uint64_t as_bytes = r256((uint64_t)s_rows * n_dims * 8), sas_bytes = r256((uint64_t)s_rows * 8), srow_bytes = r256((uint64_t)chunk * s_rows * 8);
  const uint64_t expected = two ? 2 * (row_bytes + sum_bytes + m_bytes + srow_bytes + 256) + as_bytes + 2 * sas_bytes + 512
                                : row_bytes + segi_bytes + sum_bytes + m_bytes + as_bytes + 2 * sas_bytes + srow_bytes + 512;
  const MfmaShape shape{chunk, r1, n_dims, s_rows, two ? 2u : 1u, select, sum_scratch, m_scratch};
  const MfmaWork sized = carve_summary_mfma(nullptr, shape), W = carve_summary_mfma(kBase, shape);
  CHECK(!sized.lane[0].rows && !sized.lane[0].mscratch && !sized.a_s && !sized.ia_s, "a null base gives null pointers");
  Regions regions;
  for (uint32_t l = 0; l < shape.n_lanes; ++l) {
    regions.push_back({W.lane[l].rows, (uint64_t)chunk * r1_seg * 8});
    regions.push_back({W.lane[l].seg_i, select ? (uint64_t)chunk * r1_seg * 4 : 0});
    regions.push_back({W.lane[l].scratch, sum_scratch + 256});
    regions.push_back({W.lane[l].mscratch, m_scratch + 256});
    regions.push_back({W.lane[l].srow, (uint64_t)chunk * s_rows * 8});
  }
  regions.push_back({W.a_s, (uint64_t)s_rows * n_dims * 8});
  regions.push_back({W.sa_s, (uint64_t)s_rows * 8});
  regions.push_back({W.ia_s, (uint64_t)s_rows * 8});
  char what[64];
  std::snprintf(what, sizeof what, "matrix cores (select %d, sample %d, lanes %u)", (int)select, (int)sample, shape.n_lanes);
  check_regions(what, r1, r2, n_dims, regions, W.bytes, sized.bytes, expected);
}

static void check_fused(uint32_t r1, uint32_t r2, uint32_t n_dims) {
  const uint64_t budget = 4096ull << 20;
  const uint32_t s = sample_rows(r1);
  const uint64_t fixed = r256((uint64_t)s * n_dims * 8) + (1u << 20);
  uint32_t chunk = r2;
  while (chunk > 1 && fixed + (uint64_t)chunk * ((uint64_t)r1 + s) * 8 + fused_scratch(chunk, r1, kStripe) > budget) chunk = chunk > 256 ? (chunk - 1) / 256 * 256 : chunk / 2;
  const uint64_t lists = fused_scratch(chunk, r1, kStripe);
  const uint64_t expected = r256((uint64_t)chunk * r1 * 8) + r256((uint64_t)s * n_dims * 8) + r256((uint64_t)chunk * s * 8) + lists;
  const FusedWork sized = carve_summary_fused(nullptr, chunk, r1, n_dims, s, lists), W = carve_summary_fused(kBase, chunk, r1, n_dims, s, lists);
  CHECK(!sized.seg && !sized.scratch, "a null base gives null pointers");
  check_regions("vector pipe, no distance rows", r1, r2, n_dims,
                {{W.seg, (uint64_t)chunk * r1 * 8}, {W.a_s, (uint64_t)s * n_dims * 8}, {W.srow, (uint64_t)chunk * s * 8}, {W.scratch, lists}}, W.bytes, sized.bytes, expected);
}

static void check_chunked(uint32_t r1, uint32_t r2, uint32_t n_dims, bool sample) {
  const uint64_t budget = 4096ull << 20;
  const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(r2, budget / ((uint64_t)r1 * 8)));
  const uint32_t s_rows = (sample && r1 >= 262144) ? sample_rows(r1) : 0;
  const uint64_t sum_scratch = large_scratch(chunk, r1);
  const uint64_t expected = r256((uint64_t)chunk * r1 * 8) + ((sum_scratch + 511) & ~255ull) + r256((uint64_t)s_rows * n_dims * 8) + r256((uint64_t)chunk * s_rows * 8) + 256;
  const ChunkedWork sized = carve_summary_chunked(nullptr, chunk, r1, n_dims, s_rows, sum_scratch), W = carve_summary_chunked(kBase, chunk, r1, n_dims, s_rows, sum_scratch);
  CHECK(!sized.rows && !sized.scratch, "a null base gives null pointers");
  check_regions(sample ? "chunks of distance rows (sample 1)" : "chunks of distance rows (sample 0)", r1, r2, n_dims,
                {{W.rows, (uint64_t)chunk * r1 * 8}, {W.scratch, sum_scratch + 256}, {W.a_s, (uint64_t)s_rows * n_dims * 8}, {W.srow, (uint64_t)chunk * s_rows * 8}}, W.bytes, sized.bytes,
                expected);
}

int main() {
  const uint32_t shapes[][3] = {{70001, 9, 64}, {70001, 640, 24}, {70001, 600, 200}, {131072, 300, 136}, {140000, 6, 16}, {270000, 6, 16}};
  for (const auto &s : shapes) {
    const uint32_t r1 = s[0], r2 = s[1], n_dims = s[2];
    for (int sample = 0; sample < 2; ++sample) {
      for (int lanes2 = 0; lanes2 < 2; ++lanes2) check_mfma(r1, r2, n_dims, false, sample != 0, lanes2 != 0);
      check_chunked(r1, r2, n_dims, sample != 0);
    }
    if (n_dims <= 128) check_mfma(r1, r2, n_dims, true, true, false);
    check_fused(r1, r2, n_dims);
  }
  std::printf("%s\n", failures ? "summary_layout_check: FAILED" : "summary_layout_check: ok");
  return failures ? 1 : 0;
}
