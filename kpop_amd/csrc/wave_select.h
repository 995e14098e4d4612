// wave_select.h -- the element of a given rank among values spread over a wavefront's registers, without sorting them
// (the rescaled median of counter.hip, the median over the class cells of distill.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace kpop {

// The element of rank `target` (0-based, ascending) among the wave's 64*R values, without sorting them: quickselect on
// wave ballots.  The values strictly between `lo` and `hi` are still candidates; the first candidate in (register, lane)
// order is the pivot (the registers are looked at until one holds a candidate); two comparisons per register count the
// values below the pivot and those not above it -- over all the values, so the bounds need not be applied -- and one of
// the bounds moves.  Every step is wave-uniform (no divergence, no LDS, no cross-lane data movement but one readlane);
// ties and the zeros that dominate sparse spectra finish in a step.  Expected ~2 ln(m) steps of ~2R comparisons against
// the ~R log^2(64R) compare-exchanges plus cross-lane shuffles of a full sort.
// The values are compared as the doubles they are (f64 comparisons issue at the full rate, 64-bit integer ones on
// order-preserving keys do not): there is no NaN among them -- the norms are positive and finite -- and +inf is the
// padding of the empty slots, never a candidate (hi starts there).  So a REAL +inf among the values is not found either: a
// target that falls on one comes back as the largest finite value (and as -inf if nothing is finite); the callers keep +inf out.
template <int R>
__device__ __forceinline__ double wave_select_rank(const double (&v)[R], uint32_t target) {
  double lo = -INFINITY, hi = INFINITY;
  for (;;) {
    double pivot = 0.;
    bool found = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!found) {
        const uint64_t alive = __ballot(v[r] > lo && v[r] < hi);
        if (alive) {
          const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)alive) - 1);  // (uniform already: v_readlane, not a trip through LDS)
          const uint64_t bits = (uint64_t)__double_as_longlong(v[r]);
          pivot = __longlong_as_double((long long)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(bits >> 32), src) << 32) |
                                                   (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bits, src)));
          found = true;
        }
      }
    }
    if (!found) return lo;  // cannot happen for target < number of values
    uint32_t n_lt = 0, n_le = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      n_lt += (uint32_t)__popcll(__ballot(v[r] < pivot));
      n_le += (uint32_t)__popcll(__ballot(v[r] <= pivot));
    }
    if (target < n_lt) hi = pivot;
    else if (target < n_le) return pivot;
    else lo = pivot;
  }
}

}  // namespace kpop
