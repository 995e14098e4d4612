// count_twist_plan_check -- the plan of kpop_dev_count_twist (kpop_amd/csrc/count_twist_plan.h) as host code: pick_R and windows_of
// at their edges, the default segment length against the formula the GPU tests mirror, the route taken at every turn of the logic as
// it stood in kpop_dev_count_twist before the plan had a file of its own (restated below -- seven booleans and thirteen byte counts
// -- as the expectation), the sub-batch rule, and the workspace of every route over a null and over a made-up base: every region
// 64-byte aligned, no two overlapping, the last one ending inside the size, and the size EQUAL to the sum it was written as before (a
// larger request would be a new allocation on a warm workspace, a smaller one a region forgotten).  The same for count_wave_kernel's
// scratch, whose words follow one another unpadded as they always did (so: aligned as their types ask, the first two to 64 bytes).
// Nothing of the GPU runtime; tests/test_host_count_twist_plan.py builds it with the sanitizers.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../kpop_amd/csrc/count_twist_plan.h"

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

static uint32_t div_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// a batch of `n` sequences of `len` bases against a twister of k-mers of length k with `d` dimensions, every knob at its default
// (common.h), on a device of 256 CUs and 288 GB
static CountTwistInput batch(int k, uint32_t d, uint32_t n, uint32_t len) {
  CountTwistInput in{};
  in.k = in.hk = k;
  in.n_rows = k <= 14 ? (1ull << (2 * k)) / 2 : 1ull << 28;
  in.n_dims = d;
  in.d_pad = (d + 15u) & ~15u;
  in.has_rsel = k <= 14;
  in.n_reads = n;
  in.n_bases = (uint64_t)n * len;
  in.max_len = len;
  in.protein = false;
  in.tune_nt = 2, in.tune_unroll = 8, in.tune_seg = 0, in.tune_dense = 2, in.tune_tileg = 64, in.tune_tilepipe = 1, in.tune_tilewide = 0, in.tune_tilecap_mb = 0;
  in.n_cus = 256;
  in.device_bytes = 288ull << 30;
  return in;
}
static CountTwistInput protein_batch(int k, uint32_t d, uint32_t n, uint32_t len) {
  CountTwistInput in = batch(13, d, n, len);  // (a protein twister is loaded with the k whose 2 k bits hold the 5-bit residues)
  in.hk = k;
  in.protein = true;
  return in;
}

// ---- kpop_dev_count_twist as it decided before (the names are its locals') ----
struct Before {
  bool sub_batches;
  uint64_t m;
  int R, tile_g;
  bool wide_keys, nt_reads, long_part, tiles, pipe, wide, nt, refused, residual_launch;
  uint32_t seg_windows, seg_least, max_long, max_seg, max_groups;
  uint64_t max_slots, bytes;
};
static uint64_t tile_workspace_cap(const CountTwistInput &in) {
  if (in.tune_tilecap_mb > 0) return (uint64_t)in.tune_tilecap_mb << 20;
  uint64_t cap = (4ull << 30) * div_up(in.d_pad, 64u);
  if (in.device_bytes) cap = std::min<uint64_t>(cap, std::max<uint64_t>(4ull << 30, in.device_bytes / 4));
  return cap;
}
static Before before(const CountTwistInput &in) {
  Before b{};
  const bool protein = in.protein;
  const bool tile_route_pipe = in.has_rsel && in.hk <= 15 && in.tune_tilepipe != 0 && in.n_rows <= (1ull << 29) && in.n_rows * (in.d_pad / 16) < 0xFFFFFFFFull;
  const bool tile_route_wide = tile_route_pipe && (in.n_dims > 64 || in.tune_tilewide == 1);
  const uint32_t max_windows = in.max_len >= (uint32_t)in.hk ? in.max_len - in.hk + 1 : 0;
  if (!protein && max_windows > 512 && tile_route_wide && in.tune_dense != 0 && !in.tune_seg && in.n_reads >= 16) {
    const uint64_t max_long0 = std::min<uint64_t>(in.n_reads, in.n_bases / 512 + 1);
    const uint64_t per_slot = (uint64_t)in.n_dims * 8 + 4 + 4 + 8, cap = tile_workspace_cap(in);
    if ((in.n_bases / 512 + max_long0) * per_slot > cap) {
      const uint64_t m = cap / (((uint64_t)in.max_len / 512 + 2) * per_slot);
      if (m >= 4096 && m < in.n_reads) {
        b.sub_batches = true;
        b.m = m;
        return b;
      }
    }
  }
  b.R = max_windows <= 64 ? 1 : max_windows <= 128 ? 2 : max_windows <= 256 ? 4 : 8;
  b.wide_keys = protein ? 5 * in.hk > 30 : in.hk > 15;
  b.nt_reads = !protein && (in.tune_nt == 1 || (in.tune_nt == 2 && in.n_rows * in.d_pad * 8 > (2ull << 30)));
  b.long_part = max_windows > 512;
  if (!b.long_part) return b;
  const uint32_t seg_windows = in.tune_seg ? (uint32_t)in.tune_seg : std::max<uint32_t>(1024u, std::min<uint32_t>(16384u, (uint32_t)((3ull << 19) / ((uint64_t)in.d_pad * 8)) / 64 * 64));
  bool tiles_wanted = !protein && in.tune_dense != 0 && in.has_rsel && in.n_reads >= 16 && in.hk <= 15 && !in.tune_seg;
  b.nt = in.tune_nt == 1;
  const uint32_t max_long = (uint32_t)std::min<uint64_t>(in.n_reads, in.n_bases / 512 + 1);
  const bool pipe_able = tile_route_pipe, wide = tile_route_wide;
  if (tiles_wanted) {
    const uint64_t slots = in.n_bases / std::min(seg_windows, 512u) + max_long;
    const uint64_t per_slot = (uint64_t)in.n_dims * 8 + 4 + 4 + 8 + (in.n_dims > 64 && !wide ? (uint64_t)512 * 4 : 0);
    const uint64_t cap = wide ? tile_workspace_cap(in) : (4ull << 30);
    if (slots * per_slot > cap) tiles_wanted = false;
  }
  const bool tiles = tiles_wanted;
  const uint32_t seg_least = tiles ? std::min(seg_windows, 512u) : seg_windows;
  const uint64_t max_slots = in.n_bases / seg_least + max_long;
  const uint64_t nb = (in.n_reads + 4095) / 4096;
  const uint32_t max_seg = div_up(max_windows, seg_least), max_groups = div_up(max_long, 64);
  const uint64_t n_dims = in.n_dims, n_reads = in.n_reads;
  const uint64_t bytes_nseg = (n_reads * 4 + 63) & ~63ull, bytes_off = ((n_reads + 1) * 8 + 63) & ~63ull, bytes_sums = ((nb + 1) * 8 + 63) & ~63ull,
                 bytes_cnt = (max_slots * 4 + 63) & ~63ull, bytes_part = (max_slots * n_dims * 8 + 63) & ~63ull, bytes_done = tiles ? ((max_slots * 4 + 63) & ~63ull) : 0,
                 bytes_long = (n_reads * 4 + 64 + 63) & ~63ull, bytes_olong = tiles ? (((uint64_t)max_long * 4 + 63) & ~63ull) : 0,
                 bytes_gmax = tiles ? (((uint64_t)max_groups * 4 + 63) & ~63ull) : 0, bytes_res = tiles && n_dims > 64 && !wide ? max_slots * 512 * 4 : 0,
                 bytes_todo = tiles ? ((max_slots * 8 + 1024 + 63) & ~63ull) : 0, bytes_perread = tiles ? bytes_nseg : 0;
  const bool pipe = tiles && pipe_able;
  const uint64_t bytes_wlists = !tiles ? 0 : pipe ? (uint64_t)in.n_cus * (wide ? 3 : 2) * 8 * (8 * 512) * 4 : (uint64_t)in.n_cus * 16 * 4 * 512 * 4;
  b.bytes = bytes_nseg + bytes_off + 2 * bytes_sums + bytes_cnt + bytes_part + bytes_done + bytes_long + bytes_olong + 2 * bytes_gmax + bytes_res + bytes_todo + 2 * bytes_perread + bytes_wlists;
  b.tiles = tiles, b.pipe = pipe, b.wide = tiles && wide, b.tile_g = in.tune_tileg == 64 ? 64 : 32;
  b.residual_launch = tiles && n_dims > 64 && !pipe;
  b.refused = tiles && n_dims > 255u * 256u;
  b.seg_windows = seg_windows, b.seg_least = seg_least, b.max_long = max_long, b.max_seg = max_seg, b.max_groups = max_groups, b.max_slots = max_slots;
  return b;
}

static const char *name_of(LongRoute r) {
  switch (r) {
    case LongRoute::Stream: return "Stream";
    case LongRoute::TilePipe: return "TilePipe";
    case LongRoute::TilePipeWide: return "TilePipeWide";
    case LongRoute::TileRound4: return "TileRound4";
    default: return "TileRound4Residual";
  }
}

using Regions = std::vector<std::pair<const void *, uint64_t>>;  // (pointer, bytes in use)
static char *const kBase = reinterpret_cast<char *>(uintptr_t(1) << 40);

static void check_regions(const char *what, Regions regions, uint64_t bytes, uintptr_t align) {
  std::sort(regions.begin(), regions.end());
  const char *end = kBase;
  for (const auto &r : regions) {
    const char *at = static_cast<const char *>(r.first);
    if (!r.second) continue;  // (an empty region: a null pointer)
    CHECK(at != nullptr, "%s: a region of %llu bytes has no pointer", what, (unsigned long long)r.second);
    CHECK((reinterpret_cast<uintptr_t>(at) & (align - 1)) == 0, "%s: a region at +%lld", what, (long long)(at - kBase));
    CHECK(at >= end, "%s: a region at +%lld begins before +%lld", what, (long long)(at - kBase), (long long)(end - kBase));
    end = at + r.second;
  }
  CHECK(end <= kBase + bytes, "%s: the last region ends at +%lld of %llu", what, (long long)(end - kBase), (unsigned long long)bytes);
}

// the plan of `in` against the logic as it stood, and its workspace; returns the plan
static CountTwistPlan check_case(const char *what, const CountTwistInput &in) {
  const CountTwistPlan p = plan_count_twist(in);
  const Before b = before(in);
  CHECK((p.sub_batch_seqs != 0) == b.sub_batches && p.sub_batch_seqs == b.m, "%s: sub-batches of %u, before %llu", what, p.sub_batch_seqs, (unsigned long long)b.m);
  if (b.sub_batches) return p;
  CHECK(p.R == b.R && p.wide_keys == b.wide_keys && p.reads_nt == b.nt_reads, "%s: reads R %d keys %d nt %d, before %d %d %d", what, p.R, (int)p.wide_keys, (int)p.reads_nt, b.R,
        (int)b.wide_keys, (int)b.nt_reads);
  CHECK(p.reads_unroll == (!in.protein && in.tune_unroll == 16 ? 16 : 8), "%s: unroll %d", what, p.reads_unroll);
  CHECK(p.has_long == b.long_part, "%s: long part %d, before %d", what, (int)p.has_long, (int)b.long_part);
  if (!b.long_part) {
    CHECK(p.route == LongRoute::Stream && !p.refused, "%s: a route without a long part", what);
    return p;
  }
  const LongRoute want = !b.tiles ? LongRoute::Stream
                         : b.pipe ? (b.wide ? LongRoute::TilePipeWide : LongRoute::TilePipe)
                                  : (b.residual_launch ? LongRoute::TileRound4Residual : LongRoute::TileRound4);
  CHECK(p.route == want, "%s: route %s, before %s", what, name_of(p.route), name_of(want));
  CHECK(p.tiles() == b.tiles && p.pipe() == b.pipe, "%s: tiles %d pipe %d", what, (int)p.tiles(), (int)p.pipe());
  CHECK(p.tile_g == b.tile_g && p.stream_nt == (b.nt && !in.protein) && p.refused == b.refused, "%s: G %d nt %d refused %d", what, p.tile_g, (int)p.stream_nt, (int)p.refused);
  CHECK(p.seg_windows == b.seg_windows && p.seg_least == b.seg_least && p.max_long == b.max_long && p.max_seg == b.max_seg && p.max_groups == b.max_groups &&
            p.max_slots == b.max_slots,
        "%s: %u %u %u %u %u %llu, before %u %u %u %u %u %llu", what, p.seg_windows, p.seg_least, p.max_long, p.max_seg, p.max_groups, (unsigned long long)p.max_slots, b.seg_windows,
        b.seg_least, b.max_long, b.max_seg, b.max_groups, (unsigned long long)b.max_slots);
  // the workspace
  const CountTwistWorkspace sized = carve_count_twist(nullptr, in, p), w = carve_count_twist(kBase, in, p);
  CHECK(!sized.nseg && !sized.part && !sized.long_ids && !sized.todo && !sized.wave_lists && !sized.seg_total && !sized.n_olong && !sized.stream_next, "%s: a null base gives null pointers", what);
  CHECK(sized.bytes == w.bytes && w.bytes == b.bytes, "%s: %llu bytes over a null base, %llu over the base, %llu before", what, (unsigned long long)sized.bytes,
        (unsigned long long)w.bytes, (unsigned long long)b.bytes);
  const uint64_t n = in.n_reads, nb = (n + 4095) / 4096, t = p.tiles() ? 1 : 0;
  CHECK(w.seg_total == w.sums + nb && w.n_olong == w.sums2 + nb, "%s: the scans' totals", what);
  CHECK(!p.tiles() || (w.stream_next == w.n_todo + 1 && reinterpret_cast<char *>(w.todo) == reinterpret_cast<char *>(w.n_todo) + 1024), "%s: the to-do list's counters", what);
  CHECK(reinterpret_cast<char *>(w.long_ids) == reinterpret_cast<char *>(w.n_long) + 64, "%s: the list of long sequences", what);
  CHECK(p.tiles() || (!w.slot_done && !w.todo && !w.lpos && !w.segw && !w.n_todo && !w.stream_next), "%s: no tile route, but its regions", what);
  CHECK(w.slot_done_bytes == t * ((p.max_slots * 4 + 63) & ~63ull), "%s: slot_done", what);
  const uint64_t lists = !p.tiles() ? 0 : p.pipe() ? (uint64_t)in.n_cus * (p.route == LongRoute::TilePipeWide ? 3 : 2) * 8 * 4096 * 4 : (uint64_t)in.n_cus * 16 * 4 * 512 * 4;
  check_regions(what,
                {{w.nseg, n * 4},
                 {w.seg_off, (n + 1) * 8},
                 {w.sums, (nb + 1) * 8},
                 {w.sums2, (nb + 1) * 8},
                 {w.pcnt, p.max_slots * 4},
                 {w.part, p.max_slots * in.n_dims * 8},
                 {w.slot_done, t * p.max_slots * 4},
                 {w.n_long, 64},
                 {w.long_ids, n * 4},
                 {w.olong, t * p.max_long * 4},
                 {w.gmax, t * p.max_groups * 4},
                 {w.grel, t * p.max_groups * 4},
                 {w.res_rows, p.route == LongRoute::TileRound4Residual ? p.max_slots * 512 * 4 : 0},
                 {w.n_todo, t * 1024},
                 {w.todo, t * p.max_slots * 8},
                 {w.lpos, t * n * 4},
                 {w.segw, t * n * 4},
                 {w.wave_lists, lists}},
                w.bytes, 64);
  return p;
}

static void check_edges() {
  for (int k : {1, 3, 11, 16, 30}) {
    CHECK(windows_of(0, k) == 0 && windows_of((uint64_t)k - 1, k) == 0 && windows_of(k, k) == 1, "windows_of around k = %d", k);
    CHECK(windows_of((1ull << 32) + k, k) == (1ull << 32) + 1, "windows_of past 32 bits");
    const struct {
      uint32_t extra;  // max_len = k + extra: extra + 1 windows
      int R;
    } edges[] = {{0, 1}, {63, 1}, {64, 2}, {127, 2}, {128, 4}, {255, 4}, {256, 8}, {511, 8}, {512, 0}};
    for (const auto &e : edges) {
      const uint32_t len = (uint32_t)k + e.extra;
      CHECK(windows_of(len, k) == e.extra + 1 && pick_R(windows_of(len, k)) == e.R, "k %d, %u bases: R %d", k, len, pick_R(windows_of(len, k)));
      if (k > 14) continue;
      const CountTwistPlan p = check_case("edges of R", batch(k, 64, 40, len));  // (beyond 512 windows the reads kernel runs at R = 8 and skips the long ones)
      CHECK(p.R == (e.R ? e.R : 8) && p.has_long == (e.R == 0), "k %d, %u bases: the plan's R %d, long %d", k, len, p.R, (int)p.has_long);
    }
    CHECK(pick_R(0) == 1, "no window at all: R %d", pick_R(0));  // (max_len of k - 1)
    if (k <= 14) CHECK(check_case("max_len = k - 1", batch(k, 64, 40, (uint32_t)k - 1)).R == 1, "max_len = k - 1");
  }
}

static void check_segment_length() {
  for (uint32_t d : {9u, 64u, 100u, 256u, 1635u}) {
    const uint32_t d_pad = (d + 15) / 16 * 16;
    const uint32_t want = std::max<uint32_t>(1024, std::min<uint32_t>(16384, (3u << 19) / (d_pad * 8) / 64 * 64));
    CountTwistInput in = batch(11, d, 3, 40000);
    CountTwistPlan p = check_case("segment length", in);
    CHECK(default_seg_windows(d_pad) == want && p.seg_windows == want && p.seg_least == want, "d = %u: segments of %u windows, the formula %u", d, p.seg_windows, want);
    in.n_reads = 64, in.n_bases = 64ull * 40000;
    p = check_case("segment length, tiles", in);
    CHECK(p.tiles() && p.seg_windows == want && p.seg_least == 512, "d = %u with a tile route: %u / %u", d, p.seg_windows, p.seg_least);
    in.tune_seg = 4096;
    p = check_case("kpop_tune(seg)", in);
    CHECK(p.seg_windows == 4096 && p.seg_least == 4096 && p.route == LongRoute::Stream, "d = %u, seg 4096: %u windows, route %s", d, p.seg_windows, name_of(p.route));
  }
}

#define ROUTE(in, want) \
  do { \
    const CountTwistPlan p_ = check_case(#in, in); \
    CHECK(p_.route == LongRoute::want && !p_.sub_batch_seqs, "%s: route %s (sub-batches of %u), expected %s", #in, name_of(p_.route), p_.sub_batch_seqs, #want); \
  } while (0)

static void check_routes() {
  const CountTwistInput mutants = batch(11, 64, 64, 4000);  // 64 assemblies of 4,000 bases at 64 dimensions
  ROUTE(mutants, TilePipe);
  CountTwistInput in = mutants;
  in.n_reads = 15, in.n_bases = 15 * 4000;
  ROUTE(in, Stream);  // fewer than 16 sequences
  in.n_reads = 16, in.n_bases = 16 * 4000;
  ROUTE(in, TilePipe);
  in = mutants, in.tune_dense = 0;
  ROUTE(in, Stream);
  in = mutants, in.has_rsel = false;
  ROUTE(in, Stream);  // no rank-select index of words
  in = batch(16, 64, 64, 4000);
  CHECK(!in.has_rsel, "k = 16 has no index of words");
  in.has_rsel = true;  // (even if it had)
  ROUTE(in, Stream);
  CHECK(check_case("hk 16", in).wide_keys, "k = 16: 64-bit keys");
  in = batch(14, 64, 64, 4000), in.k = 15, in.hk = 15;
  CHECK(!check_case("hk 15", in).wide_keys, "k = 15: 32-bit keys");
  for (int k : {3, 6, 7}) {
    for (uint32_t len : {300u, 4000u}) {
      in = protein_batch(k, 64, 64, len);
      in.tune_nt = 1, in.tune_unroll = 16;
      const CountTwistPlan p = check_case("protein", in);
      CHECK(p.route == LongRoute::Stream && p.wide_keys == (k > 6) && !p.reads_nt && !p.stream_nt && p.reads_unroll == 8 && p.has_long == (len > 600),
            "protein k = %d, %u residues: route %s, keys %d", k, len, name_of(p.route), (int)p.wide_keys);
    }
  }
  in = batch(11, 65, 64, 4000);
  ROUTE(in, TilePipeWide);
  in = batch(11, 72, 64, 4000);
  ROUTE(in, TilePipeWide);
  in = mutants, in.tune_tilewide = 1;
  ROUTE(in, TilePipeWide);
  for (int g : {32, 64, 48}) {
    in = mutants, in.tune_tilepipe = 0, in.tune_tileg = g;
    ROUTE(in, TileRound4);
    CHECK(check_case("tileg", in).tile_g == (g == 64 ? 64 : 32), "tileg %d", g);
    in.n_dims = 65, in.d_pad = 80;
    ROUTE(in, TileRound4Residual);
    in.n_dims = 130, in.d_pad = 144;
    ROUTE(in, TileRound4Residual);
    in.tune_tilewide = 1;  // (means nothing without the pipeline)
    ROUTE(in, TileRound4Residual);
  }
  in = mutants, in.n_rows = (1ull << 29) + 1, in.k = in.hk = 15;  // a row's number no longer fits the residual lists' 29 bits: round 4's kernel
  ROUTE(in, TileRound4);
  // tables past 4 GiB on the narrow route: 140,000 assemblies of 30,000 bases at 64 dimensions are 8.3 M slots of 528 bytes
  in = batch(11, 64, 140000, 30000);
  ROUTE(in, Stream);
  in = batch(11, 64, 100000, 30000);  // ... and 5.9 M slots are 3.1 GB
  ROUTE(in, TilePipe);
  // the refusal: more than 65,280 dimensions with a tile route on, and not without
  in = batch(9, 65281, 64, 4000);  // (k = 9: a row's offset in 128-byte units still fits a word)
  CHECK(check_case("65,281 dimensions", in).refused && check_case("65,281 dimensions", in).route == LongRoute::TilePipeWide, "65,281 dimensions are refused");
  in.n_dims = 65280, in.d_pad = 65280;
  CHECK(!check_case("65,280 dimensions", in).refused, "65,280 dimensions are taken");
  in = batch(11, 65281, 64, 4000);
  CHECK(check_case("65,281 dimensions, k = 11", in).refused && check_case("65,281 dimensions, k = 11", in).route == LongRoute::TileRound4Residual, "... on round 4's kernel too");
  in.tune_dense = 0;
  CHECK(!check_case("65,281 dimensions, dense 0", in).refused, "kpop_tune(dense, 0) lifts the refusal");
  in = batch(11, 65281, 64, 300);
  CHECK(!check_case("65,281 dimensions, reads", in).refused, "reads are not refused");
  // the row-load policies
  in = mutants;
  CHECK(!check_case("nt 2", in).reads_nt && !check_case("nt 2", in).stream_nt, "nt 2, a small twister: plain loads");
  in.n_rows = (2ull << 30) / (64 * 8) + 1;
  CHECK(check_case("nt 2, rows past 2 GiB", in).reads_nt && !check_case("nt 2, rows past 2 GiB", in).stream_nt, "nt 2 past 2 GiB of rows: the reads kernel alone");
  in = mutants, in.tune_nt = 1;
  CHECK(check_case("nt 1", in).reads_nt && check_case("nt 1", in).stream_nt, "nt 1: both");
  in.tune_nt = 0, in.n_rows = 1ull << 28;
  CHECK(!check_case("nt 0", in).reads_nt && !check_case("nt 0", in).stream_nt, "nt 0: neither");
  in = mutants, in.tune_unroll = 16;
  CHECK(check_case("unroll 16", in).reads_unroll == 16, "unroll 16");
}

static void check_sub_batches() {
  // tests/test_gpu_twist.py, test_a_batch_past_the_tile_routes_bound_goes_through_in_sub_batches: k 11, d 72, 9,000 sequences of 6,000
  // bases under kpop_tune("tilecap_mb", 40)
  CountTwistInput in = batch(11, 72, 9000, 6000);
  in.tune_tilecap_mb = 40;
  const uint64_t m = (40ull << 20) / ((6000 / 512 + 2) * (72 * 8 + 16));
  CHECK(m == 5449, "the formula gives %llu", (unsigned long long)m);  // (41,943,040 / 7,696 = 5,449.98)
  CountTwistPlan p = check_case("sub-batches at 40 MiB", in);
  CHECK(p.sub_batch_seqs == m, "sub-batches of %u sequences, the formula %llu", p.sub_batch_seqs, (unsigned long long)m);
  CHECK(!cap_reads_device_bytes(in), "a cap of the caller's asks nothing of the device");
  in.tune_tilecap_mb = 0;
  p = check_case("the same at the default cap", in);
  CHECK(p.sub_batch_seqs == 0 && p.route == LongRoute::TilePipeWide && cap_reads_device_bytes(in), "the default cap: sub-batches of %u, route %s", p.sub_batch_seqs, name_of(p.route));
  // one sub-batch of that batch goes through whole
  in = batch(11, 72, (uint32_t)m, 6000), in.tune_tilecap_mb = 40;
  p = check_case("a sub-batch", in);
  CHECK(p.sub_batch_seqs == 0 && p.route == LongRoute::TilePipeWide, "a sub-batch: sub-batches of %u, route %s", p.sub_batch_seqs, name_of(p.route));
  // m below 4,096: no sub-batches, the streaming kernel
  in = batch(11, 72, 9000, 6000), in.tune_tilecap_mb = 30;
  CHECK((30ull << 20) / (13 * 592) == 4087, "30 MiB");
  p = check_case("m below 4,096", in);
  CHECK(p.sub_batch_seqs == 0 && p.route == LongRoute::Stream, "m = 4,087: sub-batches of %u, route %s", p.sub_batch_seqs, name_of(p.route));
  // m at or above n_reads (long sequences among short ones: the slots are counted from n_bases, a sub-batch is sized from max_len)
  in = batch(11, 72, 5000, 1023), in.max_len = 600, in.tune_tilecap_mb = 8;
  p = check_case("m above n_reads", in);
  CHECK((8ull << 20) / (3 * 592) == 4723 && p.sub_batch_seqs == 4723, "8 MiB, sequences of up to 600 bases");
  in.n_reads = 4723;
  p = check_case("m = n_reads", in);
  CHECK(p.sub_batch_seqs == 0 && p.route == LongRoute::Stream, "m = n_reads: sub-batches of %u, route %s", p.sub_batch_seqs, name_of(p.route));
  in.n_reads = 4500;
  p = check_case("m above n_reads", in);
  CHECK(p.sub_batch_seqs == 0 && p.route == LongRoute::Stream, "m > n_reads: sub-batches of %u, route %s", p.sub_batch_seqs, name_of(p.route));
  // tools/probes/count_twist_routes_digest.py: the smallest batch that still splits
  in = batch(11, 72, 4800, 1023), in.tune_tilecap_mb = 8;
  p = check_case("the digest's sub-batch case", in);
  CHECK(p.sub_batch_seqs == 4723, "4,800 sequences of 1,023 bases at 8 MiB: sub-batches of %u", p.sub_batch_seqs);
  // the narrow route never splits
  in = batch(11, 64, 140000, 30000);
  CHECK(check_case("narrow", in).sub_batch_seqs == 0, "the narrow route has no sub-batches");
  // the device's memory in the default cap: 4 GiB per 64 columns, a quarter of the device at most, never under 4 GiB
  in = batch(11, 256, 50000, 30000);  // 2.98 M slots of 2,064 bytes: 6.1 GB
  CHECK(check_case("config 3 at 256 dimensions", in).route == LongRoute::TilePipeWide, "6.1 GB of tables on 288 GB");
  in.device_bytes = 16ull << 30;  // a quarter: 4 GiB
  p = check_case("the same on 16 GB", in);
  CHECK(p.sub_batch_seqs == (4ull << 30) / ((30000 / 512 + 2) * 2064), "on 16 GB: sub-batches of %u", p.sub_batch_seqs);
  in.device_bytes = 0;  // not known: 4 GiB per 64 columns
  CHECK(check_case("the same, memory unknown", in).route == LongRoute::TilePipeWide, "memory unknown");
}

// The cases of tools/probes/count_twist_routes_digest.py that reach kpop_dev_count_twist, shape by shape and knob by knob, each with the
// route its label there ends in: the listing of that probe provably reaches every route.  (n_bases is the upper bound sequences x
// longest: the route depends on it through the caps alone, which a smaller batch stays under all the more.)
static void check_digest_cases() {
  enum Want { Reads, ToStream, ToTilePipe, ToTilePipeWide, ToRound4, ToRound4Residual, SubBatches };
  struct Knobs {
    int unroll = 8, nt = 2, seg = 0, dense = 2, tileg = 64, tilepipe = 1, tilewide = 0, tilecap_mb = 0;
  };
  const auto knobs = [](auto set) {
    Knobs kn;
    set(kn);
    return kn;
  };
  const Knobs none;
  const struct {
    const char *name;
    int k, protein_k;  // protein_k: 0 for DNA, else the residues' k (the twister loaded with k = (5 protein_k + 1) / 2)
    uint32_t d, n, longest;
    Knobs kn;
    Want want;
    int R;
  } cases[] = {
      {"reads R=1", 11, 0, 64, 300, 74, none, Reads, 1},
      {"reads R=2 (also ldspad, packed)", 11, 0, 64, 300, 138, none, Reads, 2},
      {"reads R=2 unroll 16", 11, 0, 64, 300, 138, knobs([](Knobs &q) { q.unroll = 16; }), Reads, 2},
      {"reads R=2 nt 1 (also packed)", 11, 0, 64, 300, 138, knobs([](Knobs &q) { q.nt = 1; }), Reads, 2},
      {"packed, one long sequence among 300 reads", 11, 0, 64, 301, 3000, none, ToTilePipe, 8},
      {"reads R=4", 11, 0, 64, 300, 266, none, Reads, 4},
      {"reads R=8", 11, 0, 64, 300, 522, none, Reads, 8},
      {"reads hk 16 (also packed)", 16, 0, 64, 300, 150, none, Reads, 4},
      {"protein k=3", 8, 3, 64, 200, 400, none, Reads, 8},
      {"protein k=3, three long among 40", 8, 3, 64, 43, 4000, none, ToStream, 8},
      {"protein k=7", 18, 7, 64, 200, 400, none, Reads, 8},
      {"protein k=7, three long among 40", 18, 7, 64, 43, 4000, none, ToStream, 8},
      {"three long among 10 reads, d=9", 11, 0, 9, 13, 45000, none, ToStream, 8},
      {"three long among 10 reads, d=100", 11, 0, 100, 13, 45000, none, ToStream, 8},
      {"three long among 10 reads, d=100 seg 2048", 11, 0, 100, 13, 45000, knobs([](Knobs &q) { q.seg = 2048; }), ToStream, 8},
      {"three long among 10 reads, d=100 nt 1", 11, 0, 100, 13, 45000, knobs([](Knobs &q) { q.nt = 1; }), ToStream, 8},
      {"three long among 10 reads, d=300", 11, 0, 300, 13, 45000, none, ToStream, 8},
      {"three long among 10 reads, hk 16", 16, 0, 64, 13, 45000, none, ToStream, 8},
      {"mutants d=64", 11, 0, 64, 74, 4000, none, ToTilePipe, 8},
      {"mutants d=64 tilewide 1", 11, 0, 64, 74, 4000, knobs([](Knobs &q) { q.tilewide = 1; }), ToTilePipeWide, 8},
      {"mutants d=64 tilepipe 0 tileg 32", 11, 0, 64, 74, 4000, knobs([](Knobs &q) { q.tilepipe = 0, q.tileg = 32; }), ToRound4, 8},
      {"mutants d=64 tilepipe 0 tileg 64", 11, 0, 64, 74, 4000, knobs([](Knobs &q) { q.tilepipe = 0; }), ToRound4, 8},
      {"mutants d=64 dense 0", 11, 0, 64, 74, 4000, knobs([](Knobs &q) { q.dense = 0; }), ToStream, 8},
      {"mutants d=72", 11, 0, 72, 74, 4000, none, ToTilePipeWide, 8},
      {"mutants d=130 tilepipe 0", 11, 0, 130, 74, 4000, knobs([](Knobs &q) { q.tilepipe = 0; }), ToRound4Residual, 8},
      {"mutants d=130 tilepipe 0 nt 1", 11, 0, 130, 74, 4000, knobs([](Knobs &q) { q.tilepipe = 0, q.nt = 1; }), ToRound4Residual, 8},
      {"4800 x 1023 at d=72, tilecap_mb 8", 11, 0, 72, 4800, 1023, knobs([](Knobs &q) { q.tilecap_mb = 8; }), SubBatches, 0},
      {"kpop_spectra_twist d=64", 11, 0, 64, 200, 300, none, Reads, 8},
      {"kpop_count_twist d=16, a genome among 200 reads", 11, 0, 16, 201, 5000, none, ToTilePipe, 8},
      {"kpop_count_twist d=64, a genome among 200 reads", 11, 0, 64, 201, 5000, none, ToTilePipe, 8},
  };
  for (const auto &c : cases) {
    CountTwistInput in = batch(c.k, c.d, c.n, c.longest);
    if (c.protein_k) in.hk = c.protein_k, in.protein = true;
    in.n_rows = 50000;  // (four fifths of the k-mers of a small batch)
    in.tune_unroll = c.kn.unroll, in.tune_nt = c.kn.nt, in.tune_seg = c.kn.seg, in.tune_dense = c.kn.dense, in.tune_tileg = c.kn.tileg, in.tune_tilepipe = c.kn.tilepipe;
    in.tune_tilewide = c.kn.tilewide, in.tune_tilecap_mb = c.kn.tilecap_mb;
    const CountTwistPlan p = check_case(c.name, in);
    if (c.want == SubBatches) {
      CHECK(p.sub_batch_seqs == 4723, "%s: sub-batches of %u", c.name, p.sub_batch_seqs);
      continue;
    }
    const LongRoute route = c.want == ToTilePipe ? LongRoute::TilePipe : c.want == ToTilePipeWide ? LongRoute::TilePipeWide : c.want == ToRound4 ? LongRoute::TileRound4
                            : c.want == ToRound4Residual ? LongRoute::TileRound4Residual : LongRoute::Stream;
    CHECK(!p.sub_batch_seqs && !p.refused && p.has_long == (c.want != Reads) && p.route == route && p.R == c.R, "%s: long %d, route %s, R %d", c.name, (int)p.has_long, name_of(p.route), p.R);
    CHECK(p.tile_g == (p.has_long ? c.kn.tileg : 0) && p.reads_unroll == (c.protein_k ? 8 : c.kn.unroll) && p.reads_nt == (!c.protein_k && c.kn.nt == 1) &&
              p.stream_nt == (p.has_long && !c.protein_k && c.kn.nt == 1) && p.wide_keys == (c.protein_k ? c.protein_k > 6 : c.k > 15),
          "%s: the knobs", c.name);
    if (c.kn.seg) CHECK(p.seg_windows == (uint32_t)c.kn.seg, "%s: segments of %u", c.name, p.seg_windows);
  }
  // the streaming kernel's passes where it runs without a to-do list: 9 -> one of 64; 100 -> one of 128; 300 -> 256 + 64
}

// every knob against every kind of batch: the plan is the logic as it stood, whatever the combination
static void check_sweep() {
  int cases = 0;
  const uint32_t shapes[][2] = {{40, 150}, {3, 4000}, {64, 4000}, {9000, 6000}, {200000, 30000}};  // sequences, bases each
  for (int k : {7, 11, 14, 16})
    for (uint32_t d : {9u, 64u, 65u, 100u, 130u, 300u, 1635u})
      for (const auto &s : shapes)
        for (int dense : {0, 2})
          for (int pipe : {0, 1})
            for (int wide : {0, 1})
              for (int seg : {0, 2048})
                for (int cap : {0, 8, 40})
                  for (int nt : {0, 1, 2}) {
                    CountTwistInput in = batch(k, d, s[0], s[1]);
                    in.tune_dense = dense, in.tune_tilepipe = pipe, in.tune_tilewide = wide, in.tune_seg = seg, in.tune_tilecap_mb = cap, in.tune_nt = nt;
                    in.tune_tileg = (cases & 1) ? 32 : 64;
                    check_case("sweep", in);
                    ++cases;
                  }
  std::printf("count_twist_plan_check: %d combinations of the sweep\n", cases);
}

static void check_count_wave_scratch() {
  for (uint32_t n : {1u, 7u, 8u, 9u, 64u, 511u, 512u, 513u, 4096u, 100000u, 1000003u}) {
    // as launch_count_wave_sb carved it by hand
    const uint64_t blocks = (uint64_t)div_up(n, 2 * 4) + 1, groups = blocks / 64 + 2;
    const uint64_t want = 64 + blocks * 8 + groups * 8 + ((groups * 4 + 63) & ~63ull);
    const CountWaveScratch sized = carve_count_wave(nullptr, n), s = carve_count_wave(kBase, n);
    CHECK(!sized.ticket && !sized.state && !sized.gstate && !sized.garr, "a null base gives null pointers");
    CHECK(sized.bytes == want && s.bytes == want && count_wave_scratch_bytes(n) == want, "%u reads: %llu bytes, %llu before", n, (unsigned long long)s.bytes, (unsigned long long)want);
    CHECK(reinterpret_cast<char *>(s.ticket) == kBase && reinterpret_cast<char *>(s.state) == kBase + 64 && s.gstate == s.state + blocks &&
              reinterpret_cast<uint64_t *>(s.garr) == s.gstate + groups,
          "%u reads: the words where they were", n);
    check_regions("count_wave scratch, u64", {{s.ticket, 4}, {s.state, blocks * 8}, {s.gstate, groups * 8}}, s.bytes, 8);
    check_regions("count_wave scratch", {{s.ticket, 4}, {s.state, blocks * 8}, {s.gstate, groups * 8}, {s.garr, groups * 4}}, s.bytes, 4);
  }
}

int main() {
  check_edges();
  check_segment_length();
  check_routes();
  check_sub_batches();
  check_digest_cases();
  check_sweep();
  check_count_wave_scratch();
  std::printf("%s\n", failures ? "count_twist_plan_check: FAILED" : "count_twist_plan_check: ok");
  return failures ? 1 : 0;
}
