// host_call.h -- the device side of a host-buffer entry point, once: HostCall, and the five outputs of a summary staged through it.
// refset_call.h brings it to every call on a resident set; distance.hip includes it alone (its workspace is carved by
// summary_layout.h's Carver, not refset_call.h's).
#pragma once
#include <algorithm>

#include "common.h"
#include "summary_types.h"

namespace kpop {

// The device side of a host-buffer call, inside an ArenaScope, on the null stream.  A host form names its buffers -- in(), out(),
// counted(), work(), scalars() -- then upload()s, calls its *_dev body with the pointers it was given, and finish()es:
//   - null in, null out: an output whose host pointer is null (or whose count is zero) gets no buffer and no copy and gives a null
//     device pointer, which is how the *_dev bodies are told that an optional output is not wanted;
//   - everything is allocated before anything is copied: the copies up are remembered and issued by upload(), which also returns
//     the first failure of an allocation; the copies down are remembered and issued by finish(), in the order they were named,
//     before its one synchronise;
//   - count first: read() brings a count down and waits for it; finish(n) then copies n entries of every counted() output and the
//     whole of the others.
// Nothing is copied that the caller did not name, so an early return before upload() leaves the caller's arrays as they were.
struct HostCall {
  static constexpr int kMaxBufs = 9;  // (kpop_silhouette, kpop_kmedoids)
  hipStream_t st = nullptr;

  // count elements of device memory that no copy is remembered for: a chunk's buffer, an output the body needs whoever wants it
  template <class T>
  T *dev(uint64_t count) {
    if (rc) return nullptr;
    rc = n_bufs < kMaxBufs ? bufs[n_bufs].alloc(count * sizeof(T)) : too_many();
    return rc ? nullptr : bufs[n_bufs++].as<T>();
  }
  void *work(uint64_t bytes) { return dev<char>(bytes); }
  // the 256 bytes of a call's counts; host set: count of them come down
  template <class T>
  T *scalars(T *host = nullptr, uint64_t count = 0) {
    T *d = dev<T>(256 / sizeof(T));
    if (host) down(host, d, count);
    return d;
  }
  // an operand: always a buffer (the bodies tell an empty operand by its count), and a copy up when there is something to copy
  template <class T>
  T *in(const T *host, uint64_t count) {
    T *d = dev<T>(count);
    if (host) up(d, host, count);
    return d;
  }
  // entries from .. count come down; the ones below from stay the caller's (a known prefix)
  template <class T>
  T *out(T *host, uint64_t count, uint64_t from = 0) {
    if (!host || !count) return nullptr;
    T *d = dev<T>(count);
    down(host, d, count, from);
    return d;
  }
  // room for capacity entries, of which finish(n) brings the first n down
  template <class T>
  T *counted(T *host, uint64_t capacity) {
    T *d = out(host, capacity);
    if (d) downs[n_downs - 1].counted = true;
    return d;
  }
  // a copy remembered for a buffer there is: the first count entries up, the entries from .. count down
  template <class T>
  void up(T *d, const T *host, uint64_t count) {
    remember(ups, &n_ups, const_cast<T *>(host), d, count, 0, sizeof(T));
  }
  template <class T>
  void down(T *host, const T *d, uint64_t count, uint64_t from = 0) {
    remember(downs, &n_downs, host, d, count, from, sizeof(T));
  }

  int upload() {
    KPOP_TRY(rc);
    for (int i = 0; i < n_ups; ++i) KPOP_HIP(hipMemcpyAsync(ups[i].dev, ups[i].host, ups[i].count * ups[i].elem, hipMemcpyHostToDevice, st));
    return 0;
  }
  // count entries now, and waited for: a count that decides what comes down, a done word
  template <class T>
  int read(T *host, const T *d, uint64_t count) {
    KPOP_HIP(hipMemcpyAsync(host, d, count * sizeof(T), hipMemcpyDeviceToHost, st));
    KPOP_HIP(hipStreamSynchronize(st));
    return 0;
  }
  int finish(uint64_t n = 0) {
    for (int i = 0; i < n_downs; ++i) {
      const Copy &c = downs[i];
      const uint64_t end = c.counted ? std::min(n, c.count) : c.count;
      if (end > c.from) KPOP_HIP(hipMemcpyAsync(c.host + c.from * c.elem, c.dev + c.from * c.elem, (end - c.from) * c.elem, hipMemcpyDeviceToHost, st));
    }
    KPOP_HIP(hipStreamSynchronize(st));
    return KPOP_OK;
  }

 private:
  struct Copy {
    char *host, *dev;
    uint64_t count, from;
    uint32_t elem;
    bool counted;
  };
  DevBuf bufs[kMaxBufs];
  Copy ups[kMaxBufs], downs[kMaxBufs];
  int n_bufs = 0, n_ups = 0, n_downs = 0;
  int rc = 0;  // the first failure of an allocation

  int too_many() { KPOP_FAIL(KPOP_ERR_INVALID, "HostCall: more than %d buffers or copies in a call", kMaxBufs); }
  void remember(Copy *list, int *n, void *host, const void *d, uint64_t count, uint64_t from, uint32_t elem) {
    if (rc || !count || (*n == kMaxBufs && (rc = too_many()))) return;
    list[(*n)++] = Copy{reinterpret_cast<char *>(host), reinterpret_cast<char *>(const_cast<void *>(d)), count, from, elem, false};
  }
};

// the five outputs of a summary, staged for r2 query rows: the device's SummaryOut for the body; finish() brings stats and n down,
// and the three lists when there are any.  host then goes to the long-list completion
static inline SummaryOut summary_stage(HostCall &h, uint32_t r2, const SummaryOut &host) {
  const uint64_t nn = (uint64_t)r2 * host.max_neighbours;
  SummaryOut d = host;
  d.stats = h.dev<double>((uint64_t)r2 * 4);
  d.n = h.dev<uint32_t>(r2);
  d.idx = h.dev<uint32_t>(nn);
  d.dist = h.dev<double>(nn);
  d.z = h.dev<double>(nn);
  h.down(host.stats, d.stats, (uint64_t)r2 * 4);
  h.down(host.n, d.n, r2);
  h.down(host.idx, d.idx, nn);
  h.down(host.dist, d.dist, nn);
  h.down(host.z, d.z, nn);
  return d;
}

}  // namespace kpop
