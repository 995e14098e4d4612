// space_ops.h -- the per-dimension term and the final scale of a distance (lib/Space.ml:150-165), shared by the distance
// kernels (distance.hip), the summary that computes its distances as it goes (summary_large.hip) and the pair tile (pair_tile.h);
// and the keys under which doubles and distances order as unsigned integers.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/kpop_hip.h"

namespace kpop {

// unscaled component and scale (lib/Space.ml:150-165)
template <int KIND>
__device__ __forceinline__ double component(double diff, double m, double p) {
  if (KIND == KPOP_MINKOWSKI) return __dmul_rn(pow(fabs(diff), p), m);
  return __dmul_rn(__dmul_rn(diff, diff), m);
}

template <int KIND>
__device__ __forceinline__ double scale_distance(double x, double p) {
  if (KIND == KPOP_EUCLIDEAN) return sqrt(x);
  if (KIND == KPOP_COSINE) return x / 2.0;
  return pow(x, 1.0 / p);
}

// a double's bits mapped so that doubles order as unsigned integers, negative ones included (only a NaN's bits map to ~0), and back
__device__ __forceinline__ uint64_t f64_key(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double key_f64(uint64_t k) { return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k)); }

// a distance that is a number -> a key that orders as the distance does; -0 is taken as +0.  Pairs order by (key, index)
__device__ __forceinline__ uint64_t distance_key(double d) {
  if (d == 0.0) d = 0.0;
  return f64_key(d);
}
__device__ __forceinline__ bool key_less(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) { return ka < kb || (ka == kb && ia < ib); }

}  // namespace kpop
