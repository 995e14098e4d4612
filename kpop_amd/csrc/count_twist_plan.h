// count_twist_plan.h -- what kpop_dev_count_twist (count_twist.hip) does with a batch, decided ONCE and as plain host code: which
// instantiation of the reads kernel, whether there is a long part, which route its sequences take, how they are cut into segments,
// and where every region of the library's workspace lies (run over a null base the layout sizes the workspace, over the real base
// it hands out the pointers, as summary_layout.h does).  Nothing of the GPU runtime: tests/host/count_twist_plan_check.cpp runs it
// as it is.  The constants the decision reads are defined here and nowhere else; count_twist.hip and tile_pipe.h use them from here.
// (Two exceptions, for the layouts' sake: kPlanScanTile and kPlanLookGroup repeat scan.h's and lookback.h's, which are device headers;
// count_twist.hip asserts them equal.)
#pragma once
#include <algorithm>
#include <cstdint>

namespace kpop {

constexpr int kWavesPerBlock = 4;
constexpr uint32_t kWaveMaxWindows = 512;  // 64 lanes x R=8: the per-read kernels' limit
constexpr uint32_t kSegWindows = 16384;    // upper bound of a segment
// Row-load policy, kpop_tune("nt", 2) = automatic (measured: profiles/r02_b_realistic_inputs.txt).
// Non-temporal loads keep once-read rows from displacing the name -> row index, which is worth 0-6 % when reads are
// uniformly random over a table many times the 256 MB Infinity Cache -- and costs 6-35 % whenever rows ARE re-read:
// tables up to ~1 GB even under uniform access (the cache holds a useful share of them), reads drawn from a few
// genomes, assemblies of one organism.  So: reads kernel non-temporal only above 2 GiB of rows; genome kernel never
// (a batch of assemblies is one species more often than not, and there plain loads are 1.5x faster).
constexpr uint64_t kStreamingRowBytes = 2ull << 30;
constexpr uint32_t kTileProbeG = 64, kTileS = 512, kTileH = 2048;  // sequences of a probed group; windows of a stretch; slots of the set's table
constexpr uint32_t tile_set_rows(int g) { return g == 64 ? 1024u : 896u; }  // rows the numbering has room for (X rows are padded by 2: 16 rows on 16 banks)
constexpr uint32_t kTileSetCap = 768;    // rows in the set beyond which the seeds after the first add no more
constexpr uint32_t kTileStageW = 136;    // dwords of a sequence's staged stretch: 3 + 512 + 14 bytes and the thirteenth dword of the last thread
constexpr uint32_t kTileMinSeqs = 16;    // sequences with segments in a batch below which the tile kernel does not try
constexpr uint32_t kPipeListCap = 8 * kTileS;    // entries of a producer wavefront's residual list: 8 sequences x 512 windows
constexpr uint32_t kStreamMaxPasses = 255;       // take-the-next counters of the streaming launches: 256 dimensions a pass, 65,280 at most with a to-do list
constexpr uint64_t kPlanScanTile = 4096;         // scan.h's kScanTile (count_twist.hip asserts it): an exclusive scan keeps a sum per tile of this many
constexpr uint64_t kPlanLookGroup = 64;          // lookback.h's kLookGroup (likewise)

constexpr uint64_t windows_of(uint64_t len, int k) { return len >= (uint64_t)k ? len - (uint64_t)k + 1 : 0; }

// 64-window rounds a wavefront of the per-read kernels makes (0: the read is not theirs)
constexpr int pick_R(uint64_t max_windows) {
  return max_windows <= 64 ? 1 : max_windows <= 128 ? 2 : max_windows <= 256 ? 4 : max_windows <= 512 ? 8 : 0;
}

// a segment = the stretch of a sequence one block of the streaming kernel sums: its rows should sit in one XCD's L2 (4 MB) next to
// those of the neighbouring segment
constexpr uint32_t default_seg_windows(uint32_t d_pad) {
  return std::max<uint32_t>(1024u, std::min<uint32_t>(kSegWindows, (uint32_t)((3ull << 19) / ((uint64_t)d_pad * 8)) / 64 * 64));
}

struct CountTwistInput {
  // the twister
  int k, hk;  // k of its index; k the batch is hashed with (TwisterView::hk: never 0)
  uint64_t n_rows;
  uint32_t n_dims, d_pad;
  bool has_rsel;  // a rank-select index of words
  // the call
  uint32_t n_reads;
  uint64_t n_bases;
  uint32_t max_len;
  bool protein;  // content == KPOP_PROTEIN: five bits a residue (bin/KPopCount.ml:246-248)
  // the context
  int tune_nt, tune_unroll, tune_seg, tune_dense, tune_tileg, tune_tilepipe, tune_tilewide, tune_tilecap_mb;
  int n_cus;
  uint64_t device_bytes;  // the device's total memory, 0 when not known (asked for only where cap_reads_device_bytes says so)
};

enum class LongRoute {
  Stream,             // the streaming kernel alone
  TilePipe,           // count_twist_tile_pipe_kernel, up to 64 dimensions; what it leaves is the streaming kernel's, from a to-do list
  TilePipeWide,       // ... its three-stage form: more than 64 dimensions, or kpop_tune("tilewide", 1)
  TileRound4,         // kpop_tune("tilepipe", 0) or a twister the pipeline does not take: count_twist_tile_kernel, G sequences a chunk
  TileRound4Residual  // ... beyond 64 dimensions: the residual rows in a launch of their own (tile_residual_kernel)
};

struct CountTwistPlan {
  // every sequence of up to 512 windows: a wavefront each
  int R;
  bool wide_keys;    // 64-bit hashes (more than 30 bits: the all-ones sentinel needs one value free)
  int reads_unroll;  // 8 or 16 row loads in flight
  bool reads_nt;     // non-temporal row loads
  bool has_long;     // some sequence has more windows: everything below
  bool refused;      // more than 65,280 dimensions with a tile route on
  uint32_t sub_batch_seqs;  // not 0: the batch goes through in calls of this many sequences each, and nothing else here is used
  LongRoute route;
  int tile_g;        // TileRound4: 32 or 64 sequences a chunk
  bool stream_nt;
  uint32_t seg_windows, seg_least;  // windows of a segment of the streaming kernel; of the shortest segment any sequence is cut into
  uint32_t max_long, max_seg, max_groups;  // at most: sequences with segments, segments of one, probed groups
  uint64_t max_slots;                      // ... segments in all
  bool tiles() const { return route != LongRoute::Stream; }
  bool pipe() const { return route == LongRoute::TilePipe || route == LongRoute::TilePipeWide; }
};

namespace plan_detail {
struct TileFacts {
  bool wanted, pipe_able, wide;
};
// Batches of assemblies first go through a tile kernel (the consensus rows of a stretch of 64 sequences gathered once and multiplied
// on the matrix cores, the private rows gathered one by one); what it leaves -- stretches that share little with their seeds, found
// from a sample -- is the streaming kernel's as before.  kpop_tune("dense", 0) opts out (the streaming kernel alone: the reference's
// order of additions within a segment), and so does a segment length of the caller's (kpop_tune("seg")).
// The pipelined kernel (tile_pipe.h) takes a twister with a rank-select index of words (k <= 14), a row's number in 29 bits (it
// shares a word with three bits of tag in the residual lists) and a row's offset in 128-byte units in 32 (beyond 64 dimensions).
constexpr TileFacts tile_facts(const CountTwistInput &in) {
  const bool narrow = in.has_rsel && in.hk <= 15;
  const bool pipe_able = narrow && in.tune_tilepipe != 0 && in.n_rows <= (1ull << 29) && in.n_rows * (in.d_pad / 16) < 0xFFFFFFFFull;
  return TileFacts{!in.protein && in.tune_dense != 0 && narrow && in.n_reads >= kTileMinSeqs && !in.tune_seg, pipe_able,
                   pipe_able && (in.n_dims > 64 || in.tune_tilewide == 1)};
}
}  // namespace plan_detail

// does the plan of this call read CountTwistInput::device_bytes?  (The caller asks the runtime for it only then.)
constexpr bool cap_reads_device_bytes(const CountTwistInput &in) {
  const plan_detail::TileFacts t = plan_detail::tile_facts(in);
  return windows_of(in.max_len, in.hk) > kWaveMaxWindows && t.wanted && t.wide && in.tune_tilecap_mb <= 0;
}

inline CountTwistPlan plan_count_twist(const CountTwistInput &in) {
  CountTwistPlan p{};
  const uint32_t max_windows = (uint32_t)windows_of(in.max_len, in.hk);  // (max_len is 32 bits)
  p.R = pick_R(std::min(max_windows, kWaveMaxWindows));
  p.wide_keys = (in.protein ? 5 : 2) * in.hk > 30;
  p.reads_unroll = !in.protein && in.tune_unroll == 16 ? 16 : 8;
  p.reads_nt = !in.protein && (in.tune_nt == 1 || (in.tune_nt == 2 && in.n_rows * in.d_pad * 8 > kStreamingRowBytes));
  p.has_long = max_windows > kWaveMaxWindows;
  p.route = LongRoute::Stream;
  if (!p.has_long) return p;
  p.stream_nt = !in.protein && in.tune_nt == 1;
  p.seg_windows = in.tune_seg ? (uint32_t)in.tune_seg : default_seg_windows(in.d_pad);
  p.tile_g = in.tune_tileg == 64 ? 64 : 32;
  // (a sequence with segments has more than kWaveMaxWindows windows: at most this many of them)
  p.max_long = (uint32_t)std::min<uint64_t>(in.n_reads, in.n_bases / kWaveMaxWindows + 1);
  const plan_detail::TileFacts t = plan_detail::tile_facts(in);
  bool tiles = t.wanted;
  // The tile routes cut sequences into 512-window segments, so their per-slot tables are sized for n_bases / 512 slots whatever the
  // probe later finds (BASELINE config 3, D = 64: 1.5 GB of partial rows against 0.28 GB; round 4's kernel beyond 64 dimensions: 2 KB
  // of residual list a slot on top).  Where that would pass 4 GiB of workspace -- per stream -- the batch keeps the streaming kernel.
  // The three-stage kernel's bound is 4 GiB per 64 columns, a quarter of the device's memory at most, or kpop_tune("tilecap_mb") --
  // the same for every call: how a batch is cut must not depend on what happens to be free -- (BASELINE config 3 at 256 dimensions:
  // 6.1 GB of partial rows; at the reference's 1,635, README.md:1029, 39 GB), and a batch beyond THAT goes through in SUB-BATCHES of
  // sequences, m of them at most m x max_len bases, each a call of its own -- if that leaves 4,096 sequences a call or more.
  if (tiles) {
    const uint64_t slots = in.n_bases / std::min(p.seg_windows, kTileS) + p.max_long;
    const uint64_t per_slot = (uint64_t)in.n_dims * 8 + 4 + 4 + 8 + (in.n_dims > 64 && !t.wide ? (uint64_t)kTileS * 4 : 0);
    uint64_t cap = 4ull << 30;
    if (t.wide && in.tune_tilecap_mb > 0) cap = (uint64_t)in.tune_tilecap_mb << 20;
    else if (t.wide) {
      cap = (4ull << 30) * ((in.d_pad + 63) / 64);
      if (in.device_bytes) cap = std::min<uint64_t>(cap, std::max<uint64_t>(4ull << 30, in.device_bytes / 4));
    }
    if (slots * per_slot > cap) {
      const uint64_t m = t.wide ? cap / (((uint64_t)in.max_len / kTileS + 2) * per_slot) : 0;
      if (m >= 4096 && m < in.n_reads) {
        p.sub_batch_seqs = (uint32_t)m;
        return p;
      }
      tiles = false;
    }
  }
  p.route = !tiles ? LongRoute::Stream
            : t.pipe_able ? (t.wide ? LongRoute::TilePipeWide : LongRoute::TilePipe)
                          : (in.n_dims > 64 ? LongRoute::TileRound4Residual : LongRoute::TileRound4);
  p.refused = tiles && in.n_dims > kStreamMaxPasses * 256u;
  p.seg_least = tiles ? std::min(p.seg_windows, kTileS) : p.seg_windows;
  p.max_slots = in.n_bases / p.seg_least + p.max_long;  // every sequence with segments adds at most W / seg + 1 of them
  p.max_seg = (max_windows + p.seg_least - 1) / p.seg_least;
  p.max_groups = (p.max_long + kTileProbeG - 1) / kTileProbeG;
  return p;
}

// regions one after the other, each rounded up to 64 bytes; an empty region is a null pointer
struct Carver64 {
  char *base;
  uint64_t off = 0;
  explicit Carver64(void *b) : base(static_cast<char *>(b)) {}
  template <class T>
  T *take(uint64_t count) {
    char *at = base && count ? base + off : nullptr;
    off += (count * sizeof(T) + 63) & ~63ull;
    return reinterpret_cast<T *>(at);
  }
};

// The long part's workspace.  Without a tile route: the segment table, the partial rows and the list of long sequences.
struct CountTwistWorkspace {
  uint32_t *nseg;                 // [n_reads] segments of a sequence
  uint64_t *seg_off;              // [n_reads + 1] its first slot
  uint64_t *sums, *seg_total;     // the scan's sums a tile of nseg, the last of them: the segments in all
  uint64_t *sums2, *n_olong;      // ... of the long sequences' scan, and how many there are
  uint32_t *pcnt;                 // [max_slots] windows found a slot
  double *part;                   // [max_slots][n_dims] partial rows
  uint32_t *slot_done;            // [max_slots] tile routes: the slot's sums are complete
  uint32_t *n_long, *long_ids;    // the long sequences as segment_count_kernel appends them: their number (a line of its own), [n_reads]
  uint32_t *olong;                // [max_long] ... in batch order
  uint32_t *gmax, *grel;          // [max_groups] a probed group's longest sequence in stretches; is it one organism
  uint32_t *res_rows;             // [max_slots][kTileS] TileRound4Residual: the residual lists
  uint32_t *n_todo, *stream_next; // the to-do list's length; [kStreamMaxPasses] a take-the-next counter per streaming launch (1 KB together)
  uint32_t (*todo)[2];            // [max_slots] (sequence, segment) the tile kernel left
  uint32_t *lpos, *segw;          // [n_reads] a long sequence's place in olong; the segment length it is cut with
  uint32_t *wave_lists;           // the tile kernels' per-wavefront lists
  uint64_t slot_done_bytes, bytes;
};
inline CountTwistWorkspace carve_count_twist(void *base, const CountTwistInput &in, const CountTwistPlan &p) {
  Carver64 c(base);
  CountTwistWorkspace w{};
  const bool tiles = p.tiles();
  const uint64_t nb = (in.n_reads + kPlanScanTile - 1) / kPlanScanTile, if_tiles = tiles ? 1 : 0;
  w.nseg = c.take<uint32_t>(in.n_reads);
  w.seg_off = c.take<uint64_t>((uint64_t)in.n_reads + 1);
  w.sums = c.take<uint64_t>(nb + 1);
  w.seg_total = w.sums ? w.sums + nb : nullptr;
  w.sums2 = c.take<uint64_t>(nb + 1);
  w.n_olong = w.sums2 ? w.sums2 + nb : nullptr;
  w.pcnt = c.take<uint32_t>(p.max_slots);
  w.part = c.take<double>(p.max_slots * in.n_dims);
  w.slot_done = c.take<uint32_t>(if_tiles * p.max_slots);
  w.slot_done_bytes = if_tiles * ((p.max_slots * 4 + 63) & ~63ull);
  w.n_long = c.take<uint32_t>(16);
  w.long_ids = c.take<uint32_t>(in.n_reads);
  w.olong = c.take<uint32_t>(if_tiles * p.max_long);
  w.gmax = c.take<uint32_t>(if_tiles * p.max_groups);
  w.grel = c.take<uint32_t>(if_tiles * p.max_groups);
  w.res_rows = c.take<uint32_t>(p.route == LongRoute::TileRound4Residual ? p.max_slots * kTileS : 0);
  w.n_todo = c.take<uint32_t>(if_tiles * (1 + kStreamMaxPasses));
  w.stream_next = w.n_todo ? w.n_todo + 1 : nullptr;
  w.todo = c.take<uint32_t[2]>(if_tiles * p.max_slots);
  w.lpos = c.take<uint32_t>(if_tiles * in.n_reads);
  w.segw = c.take<uint32_t>(if_tiles * in.n_reads);
  w.wave_lists = c.take<uint32_t>(!tiles ? 0
                                  : p.pipe() ? (uint64_t)in.n_cus * (p.route == LongRoute::TilePipeWide ? 3 : 2) * 8 * kPipeListCap
                                             : (uint64_t)in.n_cus * 16 * 4 * kTileS);
  w.bytes = c.off;
  return w;
}

// count_wave_kernel's scratch: the ticket counter (a line of its own), one look-back word per block and, for the two-level look-back,
// a word and an arrival counter per group of kLookGroup blocks (lookback.h).  The words follow one another unpadded.
struct CountWaveScratch {
  uint32_t *ticket;
  uint64_t *state, *gstate;
  uint32_t *garr;
  uint64_t bytes;
};
inline CountWaveScratch carve_count_wave(void *base, uint32_t n_reads) {
  const uint64_t blocks = ((uint64_t)n_reads + 2 * kWavesPerBlock - 1) / (2 * kWavesPerBlock) + 1, groups = blocks / kPlanLookGroup + 2;
  char *b = static_cast<char *>(base);
  CountWaveScratch s{};
  if (b) {
    s.ticket = reinterpret_cast<uint32_t *>(b);
    s.state = reinterpret_cast<uint64_t *>(b + 64);
    s.gstate = s.state + blocks;
    s.garr = reinterpret_cast<uint32_t *>(s.gstate + groups);
  }
  s.bytes = 64 + blocks * 8 + groups * 8 + ((groups * 4 + 63) & ~63ull);
  return s;
}
inline uint64_t count_wave_scratch_bytes(uint32_t n_reads) { return carve_count_wave(nullptr, n_reads).bytes; }

}  // namespace kpop
