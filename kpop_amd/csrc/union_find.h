// union_find.h -- the lock-free union-find of clusters.hip, dbscan.hip and forest.hip (and of a tile's forest in LDS, self_tile.h): a
// forest in an array of parent words, parent[i] == i a root.  The union hooks the LARGER root under the smaller with one compare-and-swap; finds halve the paths.  Only a root is
// ever hooked, and only under a smaller index: the forest stays acyclic, a row that has stopped being a root never becomes one
// again, and the last root of a component is its smallest index whoever arrives first.  A failed compare-and-swap means somebody
// else hooked that root: progress, and nothing waits on another workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kpop {

// parent words are read and written by many workgroups at once: relaxed atomics at SCOPE (the device's for words in HBM, the
// workgroup's for a tile's forest in LDS), so that no read is served from a stale line of a compute unit's own cache
template <int SCOPE>
__device__ __forceinline__ uint32_t uf_load(uint32_t *q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, SCOPE); }

// the root of x, halving the path on the way.  A plain store of a grandparent into a node that is not a root: whoever hooks a root
// compares against the root's own index, which a node that has a parent no longer holds
template <int SCOPE>
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x) {
  for (;;) {
    const uint32_t q = uf_load<SCOPE>(parent + x);
    if (q == x) return x;
    const uint32_t g = uf_load<SCOPE>(parent + q);
    if (g == q) return q;
    __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, SCOPE);
    x = g;
  }
}

template <int SCOPE>
__device__ __forceinline__ uint32_t uf_find_readonly(uint32_t *parent, uint32_t x) {
  for (;;) {
    const uint32_t q = uf_load<SCOPE>(parent + x);
    if (q == x) return x;
    x = q;
  }
}

// after the unions, a launch of its own: the root of i, stored in i's word unless i is that root.  A root is a row whose word is its
// own index: no store here changes that, and a word on somebody's path is that row's ancestor before the store and after it, so the
// finds of the other threads of the launch (which store nothing but this) still end at the same roots
template <int SCOPE>
__device__ __forceinline__ uint32_t uf_settle(uint32_t *parent, uint32_t i) {
  const uint32_t root = uf_find_readonly<SCOPE>(parent, i);
  if (root != i) __hip_atomic_store(parent + i, root, __ATOMIC_RELAXED, SCOPE);
  return root;
}

template <int SCOPE>
__device__ __forceinline__ void uf_unite(uint32_t *parent, uint32_t a, uint32_t b) {
  // the same parent: the same component (most hits of a dense lineage).  A shortcut and nothing else: a word only ever moves to an
  // ancestor, and ancestors stay ancestors, so two nodes seen under one parent -- at whatever two moments -- share a root for good,
  // and the loop below would find that and hook nothing.  What it skips is path halving, which moves no node to another component
  if (uf_load<SCOPE>(parent + a) == uf_load<SCOPE>(parent + b)) return;
  for (;;) {
    a = uf_find<SCOPE>(parent, a);
    b = uf_find<SCOPE>(parent, b);
    if (a == b) return;
    const uint32_t hi = max(a, b), lo = min(a, b);
    uint32_t expected = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE)) return;
    a = hi;  // somebody else hooked hi in the meantime: from there again
    b = lo;
  }
}

}  // namespace kpop
