// device_primitives_check.hip -- the header primitives under kpop_amd/csrc/ on their own, each against the standard library on
// the host: the device-wide scan (scan.h), the LSD radix sort built on it (radix_sort.h), the in-launch look-back prefix
// (lookback.h), the ballot quickselect (wave_select.h) and what wave_sort_check.hip leaves out of wave_sort.h (the pair sort, the
// striped merge, the run-length collapse, the mirrors and the row shifts).  Nothing of the library is linked: the headers are
// included as they are and kpop::set_error is defined here.
//
//   device_primitives_check scan | radix | lookback | select | wave     one sub-command a process
//   device_primitives_check --selftest                                   every sub-command's comparisons on a perturbed result
//
// Every case prints one line `<case name> bad <n>`; the exit status is non-zero if any case is bad or any HIP call fails.  Every
// comparison is exact (integers, doubles by ==).  Every random input comes from a std::mt19937_64 with a fixed seed.
// Every device buffer a primitive writes is followed, right after its LOGICAL end for the case, by kGuardBytes of a pattern that
// must still be there afterwards; the buffers themselves are cut from allocations sized for the largest case, so an overrun
// shorter than the guard shows as `bad`, and a longer one still lands in memory this process owns.  The radix scratch of a case
// is radix_scratch_bytes(n) long, to the byte, with the guard behind it: a radix_carve that disagrees shows there.
// --selftest runs a few small cases of each sub-command and flips one bit of the HOST copy of a device result before it is
// compared: every such case must then report bad > 0 (status 0 if all of them do).  Nothing on the device is made to misbehave.
// Built and run on the GPU box by tests/test_gpu_device_primitives.py:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -o check device_primitives_check.hip
#include <float.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../../kpop_amd/csrc/lookback.h"
#include "../../../kpop_amd/csrc/radix_sort.h"
#include "../../../kpop_amd/csrc/scan.h"
#include "../../../kpop_amd/csrc/wave_select.h"
#include "../../../kpop_amd/csrc/wave_sort.h"

namespace kpop {
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}
}  // namespace kpop
using namespace kpop;

// ---------------------------------------------------------------------------
// plumbing
// ---------------------------------------------------------------------------
#define CK(expr)                                                                                      \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) {                                                                           \
      fprintf(stderr, "%s:%d: %s -> %s\n", __FILE__, __LINE__, #expr, hipGetErrorString(e_));         \
      exit(3);                                                                                        \
    }                                                                                                 \
  } while (0)

static bool g_selftest = false;
static int g_cases = 0, g_wrong = 0;  // wrong: bad != 0 -- or, in the self-test, bad == 0

static void report(const std::string &name, uint64_t bad) {
  printf("%s%s bad %llu\n", g_selftest ? "selftest " : "", name.c_str(), (unsigned long long)bad);
  fflush(stdout);
  ++g_cases;
  if (g_selftest ? bad == 0 : bad != 0) ++g_wrong;
}

static std::string fmt(const char *f, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

// the self-test's perturbation: one bit of one element of the host copy of a device result
template <class T>
static void perturb(std::vector<T> &h) {
  if (!g_selftest || h.empty()) return;
  unsigned char *p = reinterpret_cast<unsigned char *>(&h[h.size() / 2]);
  p[0] ^= 1u;
}

static void sync_device() {
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
}

constexpr size_t kGuardBytes = 256;
constexpr int kGuardByte = 0xA5;
constexpr int kStaleByte = 0xCD;  // what an output holds before the run: an element the primitive leaves out cannot look right

template <class T>
struct Buf {
  T *p = nullptr;
  size_t cap = 0;  // elements
  Buf() = default;
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
  ~Buf() {
    if (p && hipFree(p) != hipSuccess) {
      fprintf(stderr, "hipFree failed\n");
      ++g_wrong;
    }
  }
  void reserve(size_t n_max) {
    cap = n_max;
    CK(hipMalloc(reinterpret_cast<void **>(&p), n_max * sizeof(T) + kGuardBytes));
  }
  void need(size_t n) const {
    if (n > cap) {
      fprintf(stderr, "buffer of %zu elements asked for %zu\n", cap, n);
      exit(3);
    }
  }
  // the logical length of the case: n elements, then the guard
  void arm(size_t n) {
    need(n);
    CK(hipMemset(reinterpret_cast<char *>(p) + n * sizeof(T), kGuardByte, kGuardBytes));
  }
  void fill(size_t n, int byte) {
    need(n);
    if (n) CK(hipMemset(p, byte, n * sizeof(T)));
  }
  void upload(const std::vector<T> &h) {
    need(h.size());
    if (!h.empty()) CK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  }
  std::vector<T> download(size_t n) const {
    need(n);
    std::vector<T> h(n);
    if (n) CK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return h;
  }
  uint64_t guard_bad(size_t n) const {
    unsigned char h[kGuardBytes];
    CK(hipMemcpy(h, reinterpret_cast<const char *>(p) + n * sizeof(T), kGuardBytes, hipMemcpyDeviceToHost));
    uint64_t bad = 0;
    for (size_t i = 0; i < kGuardBytes; ++i) bad += h[i] != (unsigned char)kGuardByte;
    return bad;
  }
  uint64_t stale_bad(size_t n) const {  // n elements nobody was to write
    std::vector<T> h = download(n);
    const unsigned char *c = reinterpret_cast<const unsigned char *>(h.data());
    uint64_t bad = 0;
    for (size_t i = 0; i < n * sizeof(T); ++i) bad += c[i] != (unsigned char)kStaleByte;
    return bad;
  }
};

template <class T>
static T stale_value() {
  T v;
  memset(&v, kStaleByte, sizeof v);
  return v;
}

// ---------------------------------------------------------------------------
// scan
// ---------------------------------------------------------------------------
struct LoadAddend {
  const uint32_t *p;
  __device__ uint32_t operator()(uint64_t i) const { return p[i]; }
};
struct StorePrefixAndValue {
  uint64_t *prefix;
  uint32_t *value;
  __device__ void operator()(uint64_t i, uint64_t pre, uint32_t v) const {
    prefix[i] = pre;
    value[i] = v;
  }
};

struct ScanBufs {
  Buf<uint32_t> in, v;
  Buf<uint64_t> pre, sums;
};

static void scan_case(ScanBufs &B, uint64_t n, const char *family, std::mt19937_64 &rng) {
  std::vector<uint32_t> in(n);
  const std::string f = family;
  for (uint64_t i = 0; i < n; ++i) {
    if (f == "zeros") in[i] = 0;
    else if (f == "ones") in[i] = 1;
    else if (f == "flags") in[i] = (uint32_t)(rng() & 1);
    else if (f == "counts") in[i] = (uint32_t)(rng() % 2049);  // a radix tile's digit counts: 0 .. 2048
    else in[i] = (1u << 20) - 1;  // tile_max: a full tile totals 2^32 - 4096, the most the 32-bit in-tile prefix holds
  }
  const uint64_t nb = scan_blocks(n);
  B.in.upload(in);
  B.pre.fill(n, kStaleByte);
  B.v.fill(n, kStaleByte);
  B.sums.fill(nb + 1, kStaleByte);
  B.in.arm(n);
  B.pre.arm(n);
  B.v.arm(n);
  B.sums.arm(nb + 1);
  uint64_t bad = 0;
  bad += exclusive_scan(LoadAddend{B.in.p}, StorePrefixAndValue{B.pre.p, B.v.p}, n, B.sums.p, nullptr) != 0;
  sync_device();
  std::vector<uint64_t> pre = B.pre.download(n), sums = B.sums.download(nb + 1);
  std::vector<uint32_t> v = B.v.download(n);
  perturb(pre);
  if (n == 0) perturb(sums);
  const std::vector<uint64_t> wide(in.begin(), in.end());  // (std::partial_sum adds in the input's type)
  std::vector<uint64_t> incl(n);
  std::partial_sum(wide.begin(), wide.end(), incl.begin());
  for (uint64_t i = 0; i < n; ++i) {
    bad += pre[i] != (i ? incl[i - 1] : 0ull);
    bad += v[i] != in[i];
  }
  bad += sums[nb] != (n ? incl[n - 1] : 0ull);
  bad += B.pre.guard_bad(n) + B.v.guard_bad(n) + B.sums.guard_bad(nb + 1) + B.in.guard_bad(n);
  report(fmt("scan exclusive n=%llu %s", (unsigned long long)n, family), bad);
}

// scan_block_sums_kernel alone, in place (within.hip, sort_count.hip): u64 counts in, their offsets out, the total in [nb]
static void block_sums_case(ScanBufs &B, uint64_t nb, std::mt19937_64 &rng) {
  std::vector<uint64_t> in(nb);
  for (auto &x : in) x = rng() % ((1ull << 40) + 1);
  B.sums.fill(nb + 1, kStaleByte);
  B.sums.upload(in);
  B.sums.arm(nb + 1);
  scan_block_sums_kernel<0><<<dim3(1), dim3(1024), 0, nullptr>>>(B.sums.p, nb);
  sync_device();
  std::vector<uint64_t> out = B.sums.download(nb + 1);
  perturb(out);
  uint64_t bad = 0, run = 0;
  for (uint64_t i = 0; i < nb; ++i) {
    bad += out[i] != run;
    run += in[i];
  }
  bad += out[nb] != run;
  bad += B.sums.guard_bad(nb + 1);
  report(fmt("scan block_sums nb=%llu", (unsigned long long)nb), bad);
}

static void run_scan() {
  std::mt19937_64 rng(0x5343414eull);
  const uint64_t T = kScanTile;
  const uint64_t n_max = 2049 * T + 5;
  ScanBufs B;
  B.in.reserve(n_max);
  B.v.reserve(n_max);
  B.pre.reserve(n_max);
  B.sums.reserve(4096);
  if (g_selftest) {
    scan_case(B, 0, "zeros", rng);
    scan_case(B, T + 1, "flags", rng);
    block_sums_case(B, 65, rng);
    return;
  }
  const uint64_t ns[] = {0, 1, 255, 256, T - 1, T, T + 1, 3 * T + 17, 1024 * T, 1024 * T + 1, 2049 * T + 5};
  const char *families[] = {"zeros", "ones", "flags", "counts"};
  for (uint64_t n : ns) {
    for (const char *f : families) scan_case(B, n, f, rng);
    if (n == 3 * T + 17) scan_case(B, n, "tile_max", rng);
  }
  const uint64_t nbs[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 3000};
  for (uint64_t nb : nbs) block_sums_case(B, nb, rng);
}

// ---------------------------------------------------------------------------
// radix
// ---------------------------------------------------------------------------
struct RadixBufs {
  Buf<uint64_t> a, b;
  Buf<uint32_t> va, vb;
  Buf<unsigned char> scratch;
};

static const char *const kRadixFamilies[] = {"random64", "three_values", "all_equal", "all_ones",
                                             "ones_in_last_wave", "ascending", "descending", "equal_low_bits"};

static std::vector<uint64_t> radix_keys(const std::string &f, uint64_t n, int sorted_bits, std::mt19937_64 &rng) {
  std::vector<uint64_t> k(n);
  const uint64_t three[3] = {rng(), rng(), rng()};
  const uint64_t one = rng();
  for (uint64_t i = 0; i < n; ++i) {
    if (f == "random64" || f == "ones_in_last_wave") k[i] = rng();
    else if (f == "three_values") k[i] = three[rng() % 3];
    else if (f == "all_equal") k[i] = one;
    else if (f == "all_ones") k[i] = ~0ull;
    else if (f == "ascending") k[i] = i;
    else if (f == "descending") k[i] = n - 1 - i;
    else k[i] = sorted_bits >= 64 ? one : ((rng() << sorted_bits) | (one & ((1ull << sorted_bits) - 1)));  // equal_low_bits
  }
  if (f == "ones_in_last_wave" && n) {  // the row of 64 that holds the last key: beside it the out-of-range lanes carry ~0 too
    const uint64_t row0 = (n - 1) / 64 * 64;
    k[n - 1] = ~0ull;
    for (uint64_t i = row0; i < n; ++i)
      if (rng() % 3 == 0) k[i] = ~0ull;
  }
  return k;
}

static void radix_case(RadixBufs &B, bool pairs, uint64_t n, int bits, const char *family, std::mt19937_64 &rng) {
  const int passes = (bits + 7) / 8, sorted_bits = 8 * passes;
  const uint64_t mask = sorted_bits >= 64 ? ~0ull : ((1ull << sorted_bits) - 1);
  const std::vector<uint64_t> keys = radix_keys(family, n, sorted_bits, rng);
  std::vector<uint32_t> idx(n);
  std::iota(idx.begin(), idx.end(), 0u);
  const uint64_t sbytes = radix_scratch_bytes(n);
  B.a.upload(keys);
  B.b.fill(n, kStaleByte);
  B.a.arm(n);
  B.b.arm(n);
  if (pairs) {
    B.va.upload(idx);
    B.vb.fill(n, kStaleByte);
    B.va.arm(n);
    B.vb.arm(n);
  }
  B.scratch.fill(sbytes, kStaleByte);
  B.scratch.arm(sbytes);
  uint64_t *result = nullptr;
  uint32_t *vresult = nullptr;
  uint64_t bad = 0;
  if (pairs) bad += radix_sort_pairs_u64(B.a.p, B.b.p, B.va.p, B.vb.p, n, bits, B.scratch.p, nullptr, &result, &vresult) != 0;
  else bad += radix_sort_u64(B.a.p, B.b.p, n, bits, B.scratch.p, nullptr, &result) != 0;
  sync_device();
  // which buffer holds the result: a after an even number of passes (none included, and whenever n = 0), b after an odd one
  const bool in_a = n == 0 || passes % 2 == 0;
  bad += result != (in_a ? B.a.p : B.b.p);
  if (pairs) bad += vresult != (in_a ? B.va.p : B.vb.p);
  std::vector<uint64_t> got = (in_a ? B.a : B.b).download(n);
  std::vector<uint32_t> vgot;
  if (pairs) vgot = (in_a ? B.va : B.vb).download(n);
  if (pairs) perturb(vgot);
  else perturb(got);
  std::vector<uint32_t> order = idx;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return (keys[x] & mask) < (keys[y] & mask); });
  for (uint64_t i = 0; i < n; ++i) {
    bad += got[i] != keys[order[i]];
    if (pairs) bad += vgot[i] != order[i];
  }
  if (passes == 0 || n == 0) {  // no pass: nothing but a and va is ever looked at
    bad += B.b.stale_bad(n);
    if (pairs) bad += B.vb.stale_bad(n);
  }
  bad += B.a.guard_bad(n) + B.b.guard_bad(n) + B.scratch.guard_bad(sbytes);
  if (pairs) bad += B.va.guard_bad(n) + B.vb.guard_bad(n);
  report(fmt("radix %s n=%llu bits=%d %s", pairs ? "pairs" : "keys", (unsigned long long)n, bits, family), bad);
}

static void run_radix() {
  std::mt19937_64 rng(0x5241444958ull);
  const uint64_t n_max = 40000;
  RadixBufs B;
  B.a.reserve(n_max);
  B.b.reserve(n_max);
  B.va.reserve(n_max);
  B.vb.reserve(n_max);
  B.scratch.reserve(radix_scratch_bytes(n_max) + 65536);
  if (g_selftest) {
    radix_case(B, false, 2049, 9, "random64", rng);
    radix_case(B, true, 2049, 8, "three_values", rng);
    return;
  }
  const uint64_t ns[] = {0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 1, n_max};
  const int bitss[] = {0, 1, 8, 9, 20, 40, 63, 64};
  for (int pairs = 0; pairs < 2; ++pairs)
    for (uint64_t n : ns)
      for (int bits : bitss)
        for (const char *f : kRadixFamilies) radix_case(B, pairs != 0, n, bits, f, rng);
}

// ---------------------------------------------------------------------------
// lookback: the protocol of count_wave_kernel -- one wavefront a block, the ticket from an atomic counter (the order in which the
// blocks START, so that a predecessor is always running), every word zeroed before the launch
// ---------------------------------------------------------------------------
template <bool GROUPED>
__global__ __launch_bounds__(64) void lookback_kernel(uint32_t *ticket_counter, uint64_t *state, uint64_t *gstate, uint32_t *garr,
                                                      const uint64_t *totals, int naps, uint64_t *out) {
  __shared__ uint32_t s_ticket;
  if (threadIdx.x == 0) s_ticket = atomicAdd(ticket_counter, 1u);
  __syncthreads();
  const uint32_t ticket = s_ticket;
  const int lane = threadIdx.x;
  const uint64_t total = totals[ticket];
  // a ticket-dependent pause of 0 .. 3 x 128 cycles before publishing: the blocks do not arrive in step
  const uint32_t pause = (ticket * 2654435761u) >> 30;
  for (uint32_t z = 0; z < pause; ++z) __builtin_amdgcn_s_sleep(2);
  const uint64_t pre = GROUPED ? lookback_exclusive_grouped(state, gstate, garr, ticket, gridDim.x, total, lane, naps)
                               : lookback_exclusive(state, ticket, total, lane, naps);
  if (lane == 0) out[2 * (uint64_t)ticket] = pre;
  if (lane == 63) out[2 * (uint64_t)ticket + 1] = pre;
}

struct LookBufs {
  Buf<uint32_t> counter, garr;
  Buf<uint64_t> state, gstate, totals, out;
};

static void lookback_case(LookBufs &B, bool grouped, uint32_t n, const char *family, int naps, std::mt19937_64 &rng) {
  const std::string f = family;
  std::vector<uint64_t> totals(n);
  for (auto &t : totals) t = f == "zeros" ? 0 : f == "ones" ? 1 : f == "below_2p20" ? rng() % (1ull << 20) : rng() % (1ull << 40);
  const uint32_t ng = (n + kLookGroup - 1) / kLookGroup;
  B.totals.upload(totals);
  B.counter.fill(1, 0);
  B.state.fill(n, 0);
  B.gstate.fill(ng, 0);
  B.garr.fill(ng, 0);
  B.out.fill(2 * (size_t)n, kStaleByte);
  B.counter.arm(1);
  B.state.arm(n);
  B.gstate.arm(ng);
  B.garr.arm(ng);
  B.out.arm(2 * (size_t)n);
  if (grouped)
    lookback_kernel<true><<<dim3(n), dim3(64), 0, nullptr>>>(B.counter.p, B.state.p, B.gstate.p, B.garr.p, B.totals.p, naps, B.out.p);
  else
    lookback_kernel<false><<<dim3(n), dim3(64), 0, nullptr>>>(B.counter.p, B.state.p, B.gstate.p, B.garr.p, B.totals.p, naps, B.out.p);
  sync_device();
  std::vector<uint64_t> out = B.out.download(2 * (size_t)n), state = B.state.download(n), gstate = B.gstate.download(ng);
  std::vector<uint32_t> garr = B.garr.download(ng), counter = B.counter.download(1);
  perturb(out);
  std::vector<uint64_t> incl(n);
  std::partial_sum(totals.begin(), totals.end(), incl.begin());
  uint64_t bad = 0;
  bad += counter[0] != n;
  for (uint32_t t = 0; t < n; ++t) {
    const uint64_t excl = t ? incl[t - 1] : 0;
    bad += out[2 * (size_t)t] != excl;
    bad += out[2 * (size_t)t + 1] != excl;
    // what the protocol leaves behind: one level {2, inclusive prefix}; grouped {1, total} a block ...
    bad += state[t] != (grouped ? ((1ull << 62) | totals[t]) : ((2ull << 62) | incl[t]));
  }
  for (uint32_t g = 0; g < ng; ++g) {
    const uint32_t end = std::min(n, (g + 1) * kLookGroup);
    if (grouped) {  // ... and {2, prefix through the end of the group} a group, every member arrived
      bad += gstate[g] != ((2ull << 62) | incl[end - 1]);
      bad += garr[g] != end - g * kLookGroup;
    } else {
      bad += gstate[g] != 0;
      bad += garr[g] != 0;
    }
  }
  bad += B.counter.guard_bad(1) + B.state.guard_bad(n) + B.gstate.guard_bad(ng) + B.garr.guard_bad(ng) + B.out.guard_bad(2 * (size_t)n);
  report(fmt("lookback %s tickets=%u %s naps=%d", grouped ? "grouped" : "one_level", n, family, naps), bad);
}

static void run_lookback() {
  std::mt19937_64 rng(0x4c4f4f4bull);
  const uint32_t n_max = 1100;
  LookBufs B;
  B.counter.reserve(1);
  B.garr.reserve(64);
  B.state.reserve(n_max);
  B.gstate.reserve(64);
  B.totals.reserve(n_max);
  B.out.reserve(2 * n_max);
  if (g_selftest) {
    lookback_case(B, false, 65, "below_2p20", 1, rng);
    lookback_case(B, true, 65, "below_2p20", 1, rng);
    return;
  }
  const uint32_t ns[] = {1, 2, 63, 64, 65, 128, 129, 197, 513, n_max};
  const char *families[] = {"zeros", "ones", "below_2p20", "below_2p40"};
  const int napss[] = {1, 16};
  for (int grouped = 0; grouped < 2; ++grouped)
    for (uint32_t n : ns)
      for (const char *f : families)
        for (int naps : napss) lookback_case(B, grouped != 0, n, f, naps, rng);
}

// ---------------------------------------------------------------------------
// select: a block (one wavefront) a target; slot s of the 64 R values sits in register s / 64 of lane s % 64
// ---------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(64) void select_kernel(const double *vals, const uint32_t *targets, double *out) {
  const int lane = threadIdx.x;
  double v[R];
#pragma unroll
  for (int r = 0; r < R; ++r) v[r] = vals[r * 64 + lane];
  const double x = wave_select_rank<R>(v, targets[blockIdx.x]);
  if (lane == 0) out[2 * blockIdx.x] = x;
  if (lane == 63) out[2 * blockIdx.x + 1] = x;
}

struct SelectBufs {
  Buf<double> vals, out;
  Buf<uint32_t> targets;
};

static const char *const kSelectFamilies[] = {"distinct", "five_values", "all_equal", "mostly_zeros",
                                              "signed_zeros", "denormals_and_huge", "negatives"};

static double unit(std::mt19937_64 &rng) { return (double)(rng() >> 11) * 0x1p-53; }  // [0, 1)

static std::vector<double> select_values(const std::string &f, uint32_t m, std::mt19937_64 &rng) {
  std::vector<double> v(m);
  static const double five[5] = {0.5, 1., 2., 3.25, 1e10};
  for (;;) {
    for (uint32_t i = 0; i < m; ++i) {
      if (f == "distinct") v[i] = 1e-3 + 1000. * unit(rng);
      else if (f == "five_values") v[i] = five[rng() % 5];
      else if (f == "all_equal") v[i] = 7.25;
      else if (f == "mostly_zeros") v[i] = rng() % 100 < 95 ? 0. : 1. + unit(rng);
      else if (f == "signed_zeros") {
        const int k = (int)(rng() % 3);
        v[i] = k == 0 ? 0. : k == 1 ? -0. : 0.5 + unit(rng);
      } else if (f == "denormals_and_huge")
        v[i] = rng() & 1 ? (double)(1 + rng() % 1000) * 0x1p-1074 : DBL_MAX * (1. - (double)(rng() % 1000) * 0x1p-20);
      else v[i] = 2000. * unit(rng) - 1000.;  // negatives (and positives)
    }
    if (f != "distinct") break;
    std::vector<double> s = v;
    std::sort(s.begin(), s.end());
    if (std::adjacent_find(s.begin(), s.end()) == s.end()) break;
  }
  return v;
}

template <int R>
static void select_case(SelectBufs &B, uint32_t m, const char *family, bool shuffled, std::mt19937_64 &rng) {
  const uint32_t N = 64 * R;
  const std::vector<double> real = select_values(family, m, rng);
  std::vector<double> slots(N, INFINITY);  // the padding of the empty slots
  std::copy(real.begin(), real.end(), slots.begin());
  if (shuffled) std::shuffle(slots.begin(), slots.end(), rng);
  std::vector<uint32_t> targets;
  if (m <= 65) {
    for (uint32_t t = 0; t < m; ++t) targets.push_back(t);
  } else {
    const uint32_t ts[] = {0, 1, m / 2, m - 2, m - 1};
    targets.assign(ts, ts + 5);
  }
  const size_t nt = targets.size();
  B.vals.upload(slots);
  B.targets.upload(targets);
  B.out.fill(2 * nt, kStaleByte);
  B.out.arm(2 * nt);
  select_kernel<R><<<dim3((uint32_t)nt), dim3(64), 0, nullptr>>>(B.vals.p, B.targets.p, B.out.p);
  sync_device();
  std::vector<double> out = B.out.download(2 * nt);
  perturb(out);
  std::vector<double> sorted = real;
  std::sort(sorted.begin(), sorted.end());
  uint64_t bad = 0;
  for (size_t i = 0; i < nt; ++i) {
    bad += !(out[2 * i] == sorted[targets[i]]);  // (== : which of +0 and -0 comes back depends on the layout)
    bad += !(out[2 * i + 1] == sorted[targets[i]]);
  }
  bad += B.out.guard_bad(2 * nt);
  report(fmt("select R=%d m=%u %s %s", R, m, family, shuffled ? "shuffled" : "in_order"), bad);
}

template <int R>
static void select_all(SelectBufs &B, std::mt19937_64 &rng) {
  const uint32_t N = 64 * R;
  std::vector<uint32_t> ms;
  for (uint32_t m : {1u, 2u, 63u, 64u, 65u, N - 1, N})
    if (m <= N && std::find(ms.begin(), ms.end(), m) == ms.end()) ms.push_back(m);
  std::sort(ms.begin(), ms.end());
  for (uint32_t m : ms)
    for (const char *f : kSelectFamilies)
      for (int sh = 0; sh < 2; ++sh) select_case<R>(B, m, f, sh != 0, rng);
}

static void run_select() {
  std::mt19937_64 rng(0x53454c45ull);
  SelectBufs B;
  B.vals.reserve(64 * 32);
  B.out.reserve(2 * 65);
  B.targets.reserve(65);
  if (g_selftest) {
    select_case<2>(B, 65, "distinct", true, rng);
    return;
  }
  select_all<1>(B, rng);
  select_all<2>(B, rng);
  select_all<4>(B, rng);
  select_all<8>(B, rng);
  select_all<16>(B, rng);
  select_all<32>(B, rng);
}

// ---------------------------------------------------------------------------
// wave: a block is one wavefront with 64 R keys; blocked layout e = lane * R + r unless said otherwise
// ---------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(64) void sort_pairs_kernel(const uint64_t *kin, const uint32_t *vin, uint64_t *kout, uint32_t *vout) {
  const int lane = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * 64 * R;
  uint64_t key[R];
  uint32_t val[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    key[r] = kin[base + lane * R + r];
    val[r] = vin[base + lane * R + r];
  }
  wave_bitonic_sort_pairs<R, uint64_t>(key, val, lane);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    kout[base + lane * R + r] = key[r];
    vout[base + lane * R + r] = val[r];
  }
}

struct WaveBufs {
  Buf<uint64_t> in64, out64;
  Buf<uint32_t> in32, out32, scalars;
};
constexpr size_t kWaveMax = 64 * 64 * 16;  // elements: up to 64 blocks of 64 x 16

template <int R>
static void sort_pairs_case(WaveBufs &B, std::mt19937_64 &rng) {
  const int NB = 16, N = 64 * R;
  std::vector<uint64_t> k((size_t)NB * N);
  std::vector<uint32_t> v((size_t)NB * N);
  for (int b = 0; b < NB; ++b)
    for (int i = 0; i < N; ++i) {
      // keys: a handful of values (many equal keys), one value, or anything; values: the column (distinct) or a few values
      k[(size_t)b * N + i] = b % 4 == 0 ? rng() % 7 : b % 4 == 1 ? 42 : b % 4 == 2 ? rng() : ~0ull - rng() % 3;
      v[(size_t)b * N + i] = b & 1 ? (uint32_t)(rng() % 16) : (uint32_t)((i * 37) % N);
    }
  B.in64.upload(k);
  B.in32.upload(v);
  B.out64.fill(k.size(), kStaleByte);
  B.out32.fill(v.size(), kStaleByte);
  B.out64.arm(k.size());
  B.out32.arm(v.size());
  sort_pairs_kernel<R><<<dim3(NB), dim3(64), 0, nullptr>>>(B.in64.p, B.in32.p, B.out64.p, B.out32.p);
  sync_device();
  std::vector<uint64_t> ko = B.out64.download(k.size());
  std::vector<uint32_t> vo = B.out32.download(v.size());
  perturb(vo);
  uint64_t bad = 0;
  for (int b = 0; b < NB; ++b) {
    std::vector<std::pair<uint64_t, uint32_t>> p(N);
    for (int i = 0; i < N; ++i) p[i] = {k[(size_t)b * N + i], v[(size_t)b * N + i]};
    std::sort(p.begin(), p.end());
    for (int i = 0; i < N; ++i) {
      bad += ko[(size_t)b * N + i] != p[i].first;
      bad += vo[(size_t)b * N + i] != p[i].second;
    }
  }
  bad += B.out64.guard_bad(k.size()) + B.out32.guard_bad(v.size());
  report(fmt("wave sort_pairs R=%d", R), bad);
}

// striped layout: e = r * 64 + lane
template <int R>
__global__ __launch_bounds__(64) void merge_striped_kernel(const uint64_t *in, uint64_t *out) {
  const int lane = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * 64 * R;
  uint64_t key[R];
#pragma unroll
  for (int r = 0; r < R; ++r) key[r] = in[base + r * 64 + lane];
  wave_bitonic_merge_striped<R, uint64_t>(key, lane);
#pragma unroll
  for (int r = 0; r < R; ++r) out[base + r * 64 + lane] = key[r];
}

static const char *const kMergeFamilies[] = {"rise_fall", "fall_rise", "plateaus", "all_equal", "ascending", "descending"};

// N keys that rise over the first `turn` positions and fall over the rest (or the other way round): the sorted keys dealt to
// the two sides at random
static void bitonic_fill(uint64_t *dst, int N, int turn, bool rise_first, uint64_t modulus, std::mt19937_64 &rng) {
  std::vector<uint64_t> s(N);
  for (auto &x : s) x = modulus ? rng() % modulus : rng();
  std::sort(s.begin(), s.end());
  std::vector<int> side(N, 1);
  std::fill(side.begin(), side.begin() + turn, 0);
  std::shuffle(side.begin(), side.end(), rng);
  std::vector<uint64_t> first, second;
  for (int i = 0; i < N; ++i) (side[i] == 0 ? first : second).push_back(s[i]);
  if (rise_first) std::reverse(second.begin(), second.end());
  else std::reverse(first.begin(), first.end());
  std::copy(first.begin(), first.end(), dst);
  std::copy(second.begin(), second.end(), dst + first.size());
}

template <int R>
static void merge_striped_case(WaveBufs &B, const char *family, std::mt19937_64 &rng) {
  const int NB = 16, N = 64 * R;
  const std::string f = family;
  const int turns[NB] = {0, 1, 2, 31, 32, 33, 63, N / 2 - 1, N / 2, N / 2 + 1, N - 64, N - 2, N - 1, N,
                         (int)(rng() % (N + 1)), (int)(rng() % (N + 1))};
  std::vector<uint64_t> k((size_t)NB * N);
  for (int b = 0; b < NB; ++b) {
    uint64_t *dst = &k[(size_t)b * N];
    const int turn = std::min(std::max(turns[b], 0), N);
    if (f == "rise_fall") bitonic_fill(dst, N, turn, true, 0, rng);
    else if (f == "fall_rise") bitonic_fill(dst, N, turn, false, 0, rng);
    else if (f == "plateaus") bitonic_fill(dst, N, turn, (b & 1) != 0, 1 + (uint64_t)N / 16, rng);  // runs of ~16 equal keys
    else if (f == "all_equal") std::fill(dst, dst + N, 0x0123456789abcdefull + (uint64_t)b);
    else if (f == "ascending") bitonic_fill(dst, N, N, true, b & 1 ? 0 : (uint64_t)N, rng);
    else bitonic_fill(dst, N, 0, true, b & 1 ? 0 : (uint64_t)N, rng);  // descending
  }
  B.in64.upload(k);
  B.out64.fill(k.size(), kStaleByte);
  B.out64.arm(k.size());
  merge_striped_kernel<R><<<dim3(NB), dim3(64), 0, nullptr>>>(B.in64.p, B.out64.p);
  sync_device();
  std::vector<uint64_t> o = B.out64.download(k.size());
  perturb(o);
  uint64_t bad = 0;
  for (int b = 0; b < NB; ++b) {
    std::sort(k.begin() + (size_t)b * N, k.begin() + (size_t)(b + 1) * N);
    for (int i = 0; i < N; ++i) bad += o[(size_t)b * N + i] != k[(size_t)b * N + i];
  }
  bad += B.out64.guard_bad(k.size());
  report(fmt("wave merge_striped RP=%d %s", R, family), bad);
}

template <int R>
static void merge_striped_all(WaveBufs &B, std::mt19937_64 &rng) {
  for (const char *f : kMergeFamilies) merge_striped_case<R>(B, f, rng);
}

// wave_unique / wave_unique_count: the LDS regions start out as the stale pattern and come back whole
template <int R, typename K>
__global__ __launch_bounds__(64) void unique_kernel(const K *in, K *out_key, uint32_t *out_start, uint32_t *out_scalars) {
  __shared__ K s_key[64 * R];
  __shared__ uint32_t s_start[64 * R + 1];
  const int lane = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * 64 * R;
  K stale;
  memset(&stale, kStaleByte, sizeof stale);
  for (int i = lane; i < 64 * R + 1; i += 64) {
    if (i < 64 * R) s_key[i] = stale;
    s_start[i] = 0xCDCDCDCDu;
  }
  __syncthreads();
  K key[R];
#pragma unroll
  for (int r = 0; r < R; ++r) key[r] = in[base + lane * R + r];
  uint32_t n_valid = 0xCDCDCDCDu;
  const uint32_t nu = wave_unique<R, K>(key, (K) ~(K)0, lane, s_key, s_start, n_valid);
  const uint32_t nc = wave_unique_count<R, K>(key, (K) ~(K)0, lane);
  __syncthreads();
  for (int i = lane; i < 64 * R + 1; i += 64) {
    if (i < 64 * R) out_key[base + i] = s_key[i];
    out_start[(size_t)blockIdx.x * (64 * R + 1) + i] = s_start[i];
  }
  if (lane == 0 || lane == 63) {
    uint32_t *o = out_scalars + (size_t)blockIdx.x * 6 + (lane ? 3 : 0);
    o[0] = nu;
    o[1] = n_valid;
    o[2] = nc;
  }
}

static const char *const kUniqueFamilies[] = {"no_sentinel", "all_sentinel", "all_equal", "all_distinct",
                                              "runs_cross_lanes", "runs_end_at_lanes", "partly_valid"};
constexpr int kUniqueFamilyCount = 7;

template <typename K>
static Buf<K> &wave_in(WaveBufs &B);
template <>
Buf<uint64_t> &wave_in<uint64_t>(WaveBufs &B) { return B.in64; }
template <>
Buf<uint32_t> &wave_in<uint32_t>(WaveBufs &B) { return B.in32; }
template <typename K>
static Buf<K> &wave_out(WaveBufs &B);
template <>
Buf<uint64_t> &wave_out<uint64_t>(WaveBufs &B) { return B.out64; }
template <>
Buf<uint32_t> &wave_out<uint32_t>(WaveBufs &B) { return B.out32; }

template <int R, typename K>
static void unique_cases(WaveBufs &B, Buf<uint32_t> &d_start, std::mt19937_64 &rng) {
  const int NB = kUniqueFamilyCount, N = 64 * R;
  const K sentinel = (K) ~(K)0;
  std::vector<K> k((size_t)NB * N);
  for (int b = 0; b < NB; ++b) {
    K *dst = &k[(size_t)b * N];
    const std::string f = kUniqueFamilies[b];
    // run lengths, then ascending keys a run: sorted input, the sentinels (if any) at the end
    std::vector<int> runs;
    int valid = N;
    if (f == "no_sentinel") {
      for (int left = N; left > 0;) {
        const int len = std::min(left, 1 + (int)(rng() % (2 * R + 3)));
        runs.push_back(len);
        left -= len;
      }
    } else if (f == "all_sentinel") valid = 0;
    else if (f == "all_equal") runs.push_back(N);
    else if (f == "all_distinct") runs.assign(N, 1);
    else if (f == "runs_cross_lanes") {  // every run covers register R - 1 of a lane and register 0 of the next
      runs.push_back(R > 1 ? R / 2 : 1);
      for (int left = N - runs[0]; left > 0; left -= runs.back()) runs.push_back(std::min(left, R > 1 ? R : 2));
    } else if (f == "runs_end_at_lanes") {  // every run ends in register R - 1, the next starts in register 0
      for (int left = N; left > 0; left -= runs.back()) runs.push_back(std::min(left, R * (1 + (int)(rng() % 3))));
    } else {  // partly_valid: the sentinels start in the middle of a lane (or, with one register a lane, of the wave)
      valid = R > 1 ? 37 * R + R / 2 : 37;
      for (int left = valid; left > 0;) {
        const int len = std::min(left, 1 + (int)(rng() % (2 * R + 3)));
        runs.push_back(len);
        left -= len;
      }
    }
    K key = (K)(rng() % 1000);
    int at = 0;
    if (valid)
      for (int len : runs) {
        for (int i = 0; i < len; ++i) dst[at++] = key;
        key = (K)(key + 1 + (K)(rng() % 1000) * (sizeof(K) == 8 ? (K)0x100000001ull : (K)1));
      }
    for (; at < N; ++at) dst[at] = sentinel;
  }
  Buf<K> &d_in = wave_in<K>(B), &d_key = wave_out<K>(B);
  const size_t n_start = (size_t)NB * (N + 1);
  d_in.upload(k);
  d_key.fill(k.size(), 0x11);
  d_start.fill(n_start, 0x11);
  B.scalars.fill((size_t)NB * 6, 0x11);
  d_key.arm(k.size());
  d_start.arm(n_start);
  B.scalars.arm((size_t)NB * 6);
  unique_kernel<R, K><<<dim3(NB), dim3(64), 0, nullptr>>>(d_in.p, d_key.p, d_start.p, B.scalars.p);
  sync_device();
  std::vector<K> okey = d_key.download(k.size());
  std::vector<uint32_t> ostart = d_start.download(n_start), sc = B.scalars.download((size_t)NB * 6);
  perturb(ostart);
  const uint64_t guards = d_key.guard_bad(k.size()) + d_start.guard_bad(n_start) + B.scalars.guard_bad((size_t)NB * 6);
  const int only = g_selftest ? (int)((n_start / 2) / (size_t)(N + 1)) : -1;  // (the self-test: the block of the perturbed element)
  for (int b = 0; b < NB; ++b) {
    if (only >= 0 && b != only) continue;
    const K *src = &k[(size_t)b * N], *gk = &okey[(size_t)b * N];
    const uint32_t *gs = &ostart[(size_t)b * (N + 1)], *s = &sc[(size_t)b * 6];
    // the host walk
    std::vector<K> ukey;
    std::vector<uint32_t> ustart;
    uint32_t n_valid = 0;
    for (int i = 0; i < N; ++i) {
      if (src[i] == sentinel) continue;
      ++n_valid;
      if (i == 0 || src[i] != src[i - 1]) {
        ukey.push_back(src[i]);
        ustart.push_back((uint32_t)i);
      }
    }
    const uint32_t nu = (uint32_t)ukey.size();
    ustart.push_back(n_valid);
    uint64_t bad = guards;
    for (int l = 0; l < 2; ++l) {  // lane 0's and lane 63's copies
      bad += s[3 * l] != nu;
      bad += s[3 * l + 1] != n_valid;
      bad += s[3 * l + 2] != nu;
    }
    for (uint32_t u = 0; u < (uint32_t)N; ++u) bad += gk[u] != (u < nu ? ukey[u] : stale_value<K>());
    for (uint32_t u = 0; u <= (uint32_t)N; ++u) bad += gs[u] != (u <= nu ? ustart[u] : 0xCDCDCDCDu);
    report(fmt("wave unique K=%d R=%d %s", (int)(8 * sizeof(K)), R, kUniqueFamilies[b]), bad);
  }
}

// mirrors and row shifts against their definitions, on values that differ in every lane and in both halves of a 64-bit word
template <typename K>
__device__ __host__ inline K lane_value(int lane) {
  const uint32_t lo = (uint32_t)lane * 2654435761u + 12345u, hi = ((uint32_t)lane * 40503u + 977u) | 0x80000000u;
  return sizeof(K) == 8 ? (K)(((uint64_t)hi << 32) | lo) : (K)lo;
}
template <int G, typename K>
__global__ __launch_bounds__(64) void mirror_kernel(K *out) {
  out[threadIdx.x] = wave_mirror(lane_value<K>((int)threadIdx.x), G);
}
template <int CTRL, typename K>
__global__ __launch_bounds__(64) void row_shift_kernel(K *out) {
  out[threadIdx.x] = wave_row_shift<CTRL>(lane_value<K>((int)threadIdx.x));
}

template <int G, typename K>
static void mirror_case(WaveBufs &B) {
  Buf<K> &d = wave_out<K>(B);
  d.fill(64, kStaleByte);
  d.arm(64);
  mirror_kernel<G, K><<<dim3(1), dim3(64), 0, nullptr>>>(d.p);
  sync_device();
  std::vector<K> o = d.download(64);
  perturb(o);
  uint64_t bad = d.guard_bad(64);
  for (int l = 0; l < 64; ++l) bad += o[l] != lane_value<K>(l ^ (G - 1));
  report(fmt("wave mirror G=%d K=%d", G, (int)(8 * sizeof(K))), bad);
}
template <int G>
static void mirror_both(WaveBufs &B) {
  mirror_case<G, uint32_t>(B);
  mirror_case<G, uint64_t>(B);
}

// row_shl:4 (0x104): lane i reads lane i + 4 of its row of 16; row_shr:4 (0x114): lane i - 4; 0 where that lies outside the row
template <int CTRL, typename K>
static void row_shift_case(WaveBufs &B) {
  Buf<K> &d = wave_out<K>(B);
  d.fill(64, kStaleByte);
  d.arm(64);
  row_shift_kernel<CTRL, K><<<dim3(1), dim3(64), 0, nullptr>>>(d.p);
  sync_device();
  std::vector<K> o = d.download(64);
  perturb(o);
  uint64_t bad = d.guard_bad(64);
  for (int l = 0; l < 64; ++l) {
    const int in_row = (l & 15) + (CTRL == 0x104 ? 4 : -4);
    const K want = (in_row >= 0 && in_row < 16) ? lane_value<K>((l & ~15) + in_row) : (K)0;
    bad += o[l] != want;
  }
  report(fmt("wave row_shift 0x%x K=%d", CTRL, (int)(8 * sizeof(K))), bad);
}

static void run_wave() {
  std::mt19937_64 rng(0x57415645ull);
  WaveBufs B;
  B.in64.reserve(kWaveMax);
  B.out64.reserve(kWaveMax);
  B.in32.reserve(kWaveMax);
  B.out32.reserve(kWaveMax);
  B.scalars.reserve(1024);
  Buf<uint32_t> d_start;
  d_start.reserve(kWaveMax + 64);
  if (g_selftest) {
    sort_pairs_case<2>(B, rng);
    merge_striped_case<2>(B, "rise_fall", rng);
    unique_cases<2, uint32_t>(B, d_start, rng);
    mirror_case<8, uint64_t>(B);
    row_shift_case<0x104, uint32_t>(B);
    return;
  }
  sort_pairs_case<1>(B, rng);  // distance.hip: R = 1, 2, 4, 8
  sort_pairs_case<2>(B, rng);
  sort_pairs_case<4>(B, rng);
  sort_pairs_case<8>(B, rng);
  merge_striped_all<1>(B, rng);  // distance.hip: RP = 1, 2, 4, 8 (16 is what its rounding rule allows next)
  merge_striped_all<2>(B, rng);
  merge_striped_all<4>(B, rng);
  merge_striped_all<8>(B, rng);
  merge_striped_all<16>(B, rng);
  unique_cases<1, uint32_t>(B, d_start, rng);
  unique_cases<2, uint32_t>(B, d_start, rng);
  unique_cases<4, uint32_t>(B, d_start, rng);
  unique_cases<8, uint32_t>(B, d_start, rng);
  unique_cases<1, uint64_t>(B, d_start, rng);
  unique_cases<2, uint64_t>(B, d_start, rng);
  unique_cases<4, uint64_t>(B, d_start, rng);
  unique_cases<8, uint64_t>(B, d_start, rng);
  mirror_both<2>(B);
  mirror_both<4>(B);
  mirror_both<8>(B);
  mirror_both<16>(B);
  mirror_both<32>(B);
  mirror_both<64>(B);
  row_shift_case<0x104, uint32_t>(B);
  row_shift_case<0x104, uint64_t>(B);
  row_shift_case<0x114, uint32_t>(B);
  row_shift_case<0x114, uint64_t>(B);
}

// ---------------------------------------------------------------------------
struct Sub {
  const char *name;
  void (*run)();
};
static const Sub kSubs[] = {{"scan", run_scan}, {"radix", run_radix}, {"lookback", run_lookback}, {"select", run_select}, {"wave", run_wave}};

int main(int argc, char **argv) {
  const char *what = argc == 2 ? argv[1] : "";
  int device_count = 0;
  CK(hipGetDeviceCount(&device_count));
  if (device_count < 1) {
    fprintf(stderr, "no device\n");
    return 3;
  }
  CK(hipSetDevice(0));
  if (!strcmp(what, "--selftest")) {
    g_selftest = true;
    for (const Sub &s : kSubs) {
      const int before = g_cases;
      s.run();
      if (g_cases == before) ++g_wrong;  // a sub-command without a perturbed case proves nothing
    }
    CK(hipDeviceSynchronize());
    printf("selftest: %d of %d perturbed cases went unnoticed\n", g_wrong, g_cases);
    return g_wrong != 0;
  }
  for (const Sub &s : kSubs)
    if (!strcmp(what, s.name)) {
      s.run();
      CK(hipDeviceSynchronize());
      return g_wrong != 0;
    }
  fprintf(stderr, "usage: %s scan | radix | lookback | select | wave | --selftest\n", argv[0]);
  return 2;
}
