/*
 * kpop_hip.h -- C ABI of libkpop_hip.so: KPop's count -> twist -> distance hot
 * path on AMD MI355X (gfx950).
 *
 * The reference (PaoloRibeca/KPop) is pure OCaml and has no FFI of its own
 * (SURVEY.md F1); these are the entry points an OCaml `ctypes`/stub binding
 * would bind to replace the three OCaml call sites on the hot path.  Each
 * entry point cites the reference code it replaces (file:line under the
 * reference checkout).  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain C, no exceptions/callbacks across the boundary, no torch types;
 *   - every function returns 0 on success or a negative kpop_status;
 *     kpop_last_error() returns a thread-local message for the last failure;
 *   - host entry points (kpop_*) take caller-owned host buffers and do
 *     H2D / compute / D2H internally;
 *   - device entry points (kpop_dev_*) take pointers that already live in HBM
 *     plus a hipStream_t passed as void* (NULL = default stream); they only
 *     enqueue work and do not synchronise, with these exceptions: kpop_dev_ca
 *     (host work between its launches: complete when it returns),
 *     kpop_dev_refset_wrap (it waits for its preparation pass), the first
 *     call on a stream that needs more of the library's workspace than any
 *     before it (it waits for the device, frees the block and allocates a
 *     larger one; kpop_dev_workspace_reserve[_stream] ahead of time avoids
 *     that), and kpop_dev_distance_summary against 65,536 rows and more
 *     under kpop_tune("summary_audit", 1) (it reads its counter back).  The
 *     completion of neighbour lists longer than 2,048 entries synchronises
 *     too: it belongs to the HOST entry points (kpop_distance_summary,
 *     kpop_refset_distance_summary), the device ones report such a row's
 *     length and fill 2,048 entries;
 *   - call from the PARENT process only (a HIP context does not survive
 *     fork(); the reference's fork()ed workers at lib/Twister.ml:90 are
 *     replaced wholesale, not per-worker).
 *   - threads and streams (tests/test_gpu_concurrency.py holds the library
 *     to every line of this).  Host entry points of one device slot run one
 *     at a time, whatever threads call them (a lock per slot; their device
 *     scratch is an arena that every call rewinds to where it found it).
 *     Device entry points on DIFFERENT streams may be enqueued back to back
 *     and run concurrently: the library's scratch is a block per stream (two
 *     for kpop_dev_count_twist_packed, and a stream with four events of the
 *     library's own beside a caller's stream for the two-lane summary).
 *     Calls on ONE stream may follow each other without synchronisation,
 *     whichever routes they take: each leaves the stream's block ready for
 *     the next.  One stream is driven by one host thread at a time.  A
 *     stream's workspace lives until kpop_shutdown (a pipeline's compute
 *     stream's: until kpop_pipeline_destroy).  Handles made outside a host
 *     entry point's scope by a second thread (kpop_twister_load,
 *     kpop_refset_create) get device memory of their own, never the arena's.
 *     kpop_last_error() is per thread.  A host thread works on the device
 *     slot it chose (kpop_use_device; slot 0 until it says otherwise), with
 *     handles made on that slot.  kpop_tune knobs are per slot, set for all
 *     slots at once, and must not change while a call is in flight on any
 *     thread or stream;
 *   - kpop_init(device) drives one GPU; kpop_init_devices(devices, n) drives
 *     n of them from ONE process (SURVEY.md 8b "multi-GPU sharding is
 *     internal"): handles (twisters, pipelines) belong to the device slot that
 *     was current when they were made, and kpop_sharded_* spread a batch over
 *     all slots.
 *
 * k-mer encoding (declared by this repository, see kpop_amd/csrc/kmer.h; the
 * reference keeps it in the absent BiOCamLib): A0 C1 G2 T3 either case,
 * big-endian 2-bit packing, DNA-ds key = min(fwd, reverse complement), any
 * other byte breaks the window.  Protein k-mers (KMers.ProteinHash): the 20 standard amino acids in alphabetical
 * order of their one-letter codes are 0..19, 5 bits per residue big-endian, any other byte breaks the window;
 * names are ceil(5k/4) hex digits.  Twisting takes hashes of either kind (they are just column keys).
 */
#ifndef KPOP_HIP_H
#define KPOP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  KPOP_OK = 0,
  KPOP_ERR_INVALID = -1,     /* bad argument */
  KPOP_ERR_CAPACITY = -2,    /* caller buffer too small */
  KPOP_ERR_UNSUPPORTED = -3, /* valid request the HIP path does not cover yet */
  KPOP_ERR_HIP = -4,         /* HIP runtime error (no device, OOM, launch failure) */
  KPOP_ERR_NOT_INIT = -5
} kpop_status;

/* bin/KPopCount.ml:66-82 (Content.t) */
#define KPOP_DNA_DS 0
#define KPOP_DNA_SS 1
#define KPOP_PROTEIN 2 /* k <= 12; counting, and since round 6 the fused count->twist calls too (kpop_count_twist, kpop_dev_count_twist,
                          kpop_spectra_twist, the pipeline: five bits a residue, a twister loaded with 2 k_load >= 5 k bits); not the packed form */
/* lib/Space.ml:140-143 (Distance.t) */
#define KPOP_EUCLIDEAN 0
#define KPOP_COSINE 1
#define KPOP_MINKOWSKI 2
/* lib/Space.ml:81-84 (Metric.t) */
#define KPOP_METRIC_FLAT 0
#define KPOP_METRIC_POWERS 1

/* ---------------------------------------------------------------- runtime */
int kpop_init(int device);          /* select the GPU this process drives (= kpop_init_devices(&device, 1)) */
/* Several GPUs in one process: devices[i] becomes device SLOT i (the same GPU may be named twice: two independent
   slots on it -- how the multi-device code is exercised on a one-GPU box).  Replaces `-T` / Parallel.get_nproc,
   bin/KPopTwistDB.ml:103, and the fork()ed workers of lib/Twister.ml:90-196.  The calling thread works on slot 0
   afterwards; kpop_use_device(slot) moves it (thread-local, like hipSetDevice).  Peer access between distinct GPUs is
   enabled where the hardware allows it (xGMI).                                                                       */
int kpop_init_devices(const int *devices, int n);
int kpop_use_device(int slot);
int kpop_device_slots(void);        /* slots initialised by the last kpop_init / kpop_init_devices */
int kpop_shutdown(void);            /* release workspaces */
int kpop_device_count(void);        /* >=0, or negative kpop_status */
const char *kpop_last_error(void);
const char *kpop_version(void);
int kpop_synchronize(void *stream);
/* performance knobs for A/B measurements.  A value outside what is listed is KPOP_ERR_INVALID.  What a setting may do to RESULTS, knob by
   knob (tests/tune_contract.py keeps this as a table, tests/test_gpu_tune_contract.py and the tests it names hold the kernels to it):
     the SAME BITS as the default's, every setting: "unroll", "nt", "ldspad", "pipeprio", "tilewide" (up to 64 dimensions), "hist", "histlds",
       "histguess", "blocksort", "class_set", "summary_mfma_lists", "summary_lanes", "distill_band";
     another ORDER of the same additions -- equal to the reference within 1e-12 of the result's scale (what the tests enforce), not bit for
       bit: "seg", "dense", "tilepipe", "tileg", "tilecap_mb", "direct" (a twister that lacks rows; a complete one: the same bits).  Measured,
       as max|got - reference| over max(max|reference|, 1): "seg" 64 2.6e-15, 1024 6.2e-15, 16384 1.3e-14, the default's own segments 1.2e-14
       (sequences of up to 40,000 bases, 24 to 300 dimensions); "tileg" 32 and 64 under "tilepipe" 0 1.2e-14 (70 assemblies of 3 kb, 40 to 130);
     the matrix cores' APPROXIMATION of distances, and what chooses among its paths -- distances <= 1e-12 relative; a summary's medians, MADs
       and neighbour lists bit for bit, its mean and standard deviation sums of approximate values (1e-13 relative): "distance_mfma",
       "summary_mfma", "summary2", "summary_sample", "summary_rawref", "summary_pass";
     nothing (instrumentation): "summary_audit", "distill_clock"; and "dbg", development switches under some of which results are wrong.
   "unroll" 8 (default) | 16 row loads in flight per wave; "nt" row loads 0 plain | 1 non-temporal | 2 chosen by the size of the
   twister (default); "seg" 0 (default) | 64..16384 in steps of 64: windows per segment of the genome kernel, 0 = sized to an XCD's L2 (with
   a value set the tile route is off: the streaming kernel alone, its partial sums cut where the segments end); "hist" 1 (default) | 0: the
   merged spectrum of kpop_count_reads(per_read = 0) by atomic histogram where the hashes fit 26 bits, or always by sort;
   "histlds" 1 (default) | 0 | 2 | 3 | 4: that histogram staged through LDS as the batch suggests (private tables up to k = 7;
   (hash, count) tables over the same stretch of 64 assemblies of one organism; for what does not repeat -- a read set,
   unrelated genomes -- the hashes partitioned by their top bits and every bucket counted in LDS, the table written without
   a global atomic, and -- round 5 -- the (hash, count) pairs of every bucket written straight into the spectrum at an offset taken
   by a decoupled look-back: the 4^k-counter table is never written), direct global atomics as in round 2, chunks always
   combined, always partitioned, or (4) partitioned with the dense table and its compaction as in round 4;
   "histguess" 1 (default) | 0: that partition sizes its buckets from a sample of the batch (one piece in 32; a bucket that
   overflows its room sends the call back to the exact count) or always counts every window first;
   "summary2" 1 (default) | 3 | 0 | 2: summaries against more than 4,096 rows by brackets from a sample and ONE pass over the
   distance rows, the same in two passes, round 2's one block per row, or (131,072 rows and more) with the distances
   computed and reduced in one kernel and no distance rows in memory -- same results, 1, 3 and 2 level;
   "distance_mfma" 1 (default) | 0: kpop_dev_distance_rowwise of 2^32 products and more (rows x rows x dimensions), euclidean / cosine: the
   pairs' dot products as f64 MFMAs (a tiled contraction, any number of dimensions), pairs whose d^2 is a small part of |a|^2 + |b|^2
   recomputed with the reference's chain -- <= 1e-12 relative (3e-15 measured), not bit for bit; 0: the chain for every pair (the reference's bits);
   "summary_mfma" 1 (default) | 2 | 0: summaries against 65,536 rows and more, euclidean / cosine, 4 dimensions and more (up to 128 the query rows
   stay in registers, beyond a tiled contraction; 2: up to 128 dimensions the summary's pass runs inside the contraction and no approximate row
   is written -- same results, measured level to slower: 2.77 against 2.71 ms for 256 x 1M x 64, 9.1 against 8.6 for 1,024): the distances
   as f64 MFMAs (|a|^2 + |b|^2 - 2 a.b) that only LOCATE the neighbours, the median and the MAD's edges; everything reported is
   recomputed with the reference's chain, rows the refinement cannot vouch for are redone from exact distance rows
   (distance_mfma.hip).  Same medians, MADs and neighbour lists bit for bit; mean and standard deviation are sums of the
   approximate values (1e-13 relative; values cancellation would show in are replaced by exact ones).  0: the chain for every pair.
   "summary_mfma_lists" 1 (default) | 0: that refinement reads the candidate lists the summary's one pass left, or scans the rows;
   "summary_lanes" 1 (default) | 2: 512 query rows and more of such a summary in batches of 256 on two streams (measured level);
   "summary_audit" 0 (default) | 1: count the rows left to the exact fall-back (kpop_debug_summary_fallbacks);
   "summary_sample" 1 (default) | 0: such a summary's brackets and bands from the query rows' distances to a sample of the REFERENCE ROWS at even
   spacing (a small contraction of its own; whatever the layout of the database), or from 64 runs of 1,024 consecutive elements of the distance
   rows (a database laid out lineage by lineage makes those runs speak for a few lineages: the brackets miss, the rows take the slow kernel);
   "summary_rawref" 1 (default) | 0: such a summary takes its reference set as it is (no normalised copy of it is made: the norms' pass keeps the
   rows' sums of squares, dot products are scaled where they come out, the exact chains divide as they go -- the same bits), or makes the copy;
   "class_set" 1 (default) | 0 | 2: kpop_dev_distance_rowwise (and _norms, and a resident set's) against a set of classes -- a first operand of
   fewer than 128 rows of at most 64 dimensions, euclidean or cosine, a workspace given -- through the kernel that holds a row of the second
   operand in a lane's registers and takes the class values as scalar operands (class_set.hip), from 128 rows of the second operand on; 0: never
   (the tiled kernel: the same bits); 2: every eligible shape whatever its number of rows;
   "summary_pass" 1 (default) | 0: the pass over such a summary's approximate rows written for rows the library made itself, or the general one;
   "tilepipe" 1 (default) | 0: the tile route's kernel with producer and consumer wavefronts (tile_pipe.h; beyond 64 dimensions its three-stage
   form: producers / MFMA wavefronts / gather wavefronts), or round 4's; "tilewide" 0 (default) | 1: that three-stage form at any number of
   dimensions (up to 64: the same bits); "tilecap_mb" 0 (default: 4 GiB per 64 columns, a quarter of the device at most) | MiB: the per-slot tables
   a call of that route may take before the batch goes through in sub-batches of sequences; "pipeprio" 1 (default) | 0..7: the low two bits are
   the issue priority of its MFMA wavefronts, bit 2 is accepted and read by nothing (4..7 run what 0..3 run);
   "tileg" 64 (default) | 32: sequences a chunk of round 4's kernel -- one block of 1,024 threads a CU or two of 512 (measured slower) --, read
   under "tilepipe" 0 only; "blocksort" 1 (default) | 0: kpop_count_reads(per_read = 1) on sequences of 513..32,768 windows sorts each in the LDS
   of a block of its own, or all of them in one device-wide sort;
   "dense" 2 (default) | 1 | 0: the matrix-core routes of the twist.  2: chosen by the batch -- sequences of more than 512
   windows (assemblies, k <= 15) go through count_twist_tile_kernel: the CONSENSUS rows of a stretch of 64 sequences x 512
   windows (the rows of four seed sequences, an LDS set) are multiplied on the f64 matrix cores, the rows private to one
   sequence are gathered per sequence (tile_residual_kernel), stretches that share little with their seeds stay with the
   streaming kernel; kpop_count_twist's batches of assemblies at small k go through the dense image of their
   counts (kpop_dev_count_twist_dense); kpop_twist takes the dense contraction when the spectra are dense enough.  1: kpop_twist
   always by the dense contraction (a twister small enough for the dense image).  0: opt out -- the sparse mat-vec in the reference's
   order of additions everywhere.  Results change in the last bits (<= 2e-15 relative measured; north_star allows 1e-5);
   "ldspad" 0 (default) | up to 65536: bytes of extra LDS per block of the fused reads kernel (an occupancy probe; a launch that no longer fits
   the CU's LDS fails with KPOP_ERR_HIP); "dbg" development switches (also KPOP_TUNE_DBG)  */
int kpop_tune(const char *key, int value);
/* development: the phase clocks count_twist_tile_kernel adds up under kpop_tune("dbg", 16 << 24) (s_memtime ticks of thread 0 of
   every block, eight phases in out[0..7]; tools/probes/ab_tile_kernel.py prints them) and, under kpop_tune("dbg", 32 << 24), the
   chunks it took (out[14]) and the rows of their consensus sets as multiplied on the matrix cores (out[15]: 2 x 64 x n_dims
   flops each; bench.py's MFMA roofline); read and cleared; synchronises the device */
int kpop_debug_counters(uint64_t *out, int n);
/* development: under kpop_tune("summary_audit", 1) the large-reference summaries (kpop_dev_distance_summary against 65,536 rows and
   more) count the query rows they leave to a fall-back -- rows whose sample-based brackets missed (the ten-pass kernel) or whose
   certificates failed (exact distance rows); the
   results are the same either way, the fall-back costs milliseconds.  Read and cleared.                                         */
int kpop_debug_summary_fallbacks(uint64_t *rows);

/* plain device-memory helpers so a non-HIP host language can stage buffers */
int kpop_dev_malloc(void **ptr, uint64_t bytes);
int kpop_dev_free(void *ptr);
int kpop_memcpy_h2d(void *dst, const void *src, uint64_t bytes);
int kpop_memcpy_d2h(void *dst, const void *src, uint64_t bytes);
int kpop_dev_memset(void *dst, int value, uint64_t bytes);
/* Page-locked host memory.  The streaming pipeline below copies straight from / to the caller's buffers; when they are
   page-locked the copy engines run beside the kernels and kpop_pipeline_submit returns without waiting.  An OCaml
   binding wraps kpop_host_alloc'ed memory as a Bigarray (Ctypes.bigarray_of_ptr) once and reuses it for every batch;
   kpop_host_register pins memory the caller already owns (costly per call: do it once per buffer, not per batch). */
int kpop_host_alloc(void **ptr, uint64_t bytes);
int kpop_host_free(void *ptr);
int kpop_host_register(void *ptr, uint64_t bytes);
int kpop_host_unregister(void *ptr);

/* ------------------------------------------------------------------ count
 * Replaces the per-read loop of KMerCounter.compute, bin/KPopCount.ml:36-50:
 *   KIH.iterc res read.seq (:38) + KIHF.iter dump (:46,:60) + KIHF.clear (:49).
 * bases: concatenated, already linted sequences (read r = bases[offsets[r] ..
 * offsets[r+1])).  per_read=1 is -L (one spectrum per read, :39-50); per_read=0
 * is -l (one spectrum for all reads, :60).  Output: CSR of unique
 * (hash, count), hashes ascending inside a spectrum (the reference's Hashtbl
 * order is unspecified; consumers key by name).  out_offsets has n_reads+1
 * entries (per_read=1) or 2 (per_read=0).  k: 1..30.  Integer, bit-exact.    */
int kpop_count_reads(const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, int k, int content,
                     int per_read, uint64_t *out_hash, uint32_t *out_count, uint64_t *out_offsets,
                     uint64_t out_capacity);

/* ---------------------------------------------------------------- twister
 * Device-resident twister: replaces Twister.t.twister (lib/Twister.ml:22-25)
 * plus the inverted name->column Hashtbl (lib/Twister.ml:71-76).
 * T_dims_major is the reference layout: n_dims rows (one Float.Array per
 * dimension) of n_cols coefficients; col_hash[c] = hash of the k-mer naming
 * column c (hex name parsed by the binding).  On device it is re-laid k-mer-
 * major so one k-mer's coefficients are one contiguous row.                  */
typedef struct kpop_twister kpop_twister;
int kpop_twister_load(const double *T_dims_major, uint64_t n_cols, uint32_t n_dims, const uint64_t *col_hash,
                      int k, kpop_twister **out);
/* synthetic twister generated on device: columns = every
   canonical (DNA-ds) / every (DNA-ss) k-mer ascending, coefficient(d,h) from
   SplitMix64 -- bench/test tooling, same function as the oracle's.           */
int kpop_twister_synth(uint64_t seed, int k, int content, uint32_t n_dims, kpop_twister **out);
/* One rank's slice of the same twister when its k-mer rows are sharded over GPUs (k = 15 / large D):
   only the k-mers with hash in [hash_lo, hash_hi).  acc_dim = 1 appends a dimension of ones, so an un-normalised
   twist also carries the shard's part of the normaliser `acc` (lib/Twister.ml:158): the ranks all-reduce
   [n x (n_dims+1)] partials and divide by the last column (kpop_amd/shard.py).                                  */
int kpop_twister_synth_slice(uint64_t seed, int k, int content, uint32_t n_dims, uint64_t hash_lo,
                             uint64_t hash_hi, int acc_dim, kpop_twister **out);
/* The fused count -> twist entry points hash the reads with the k the twister was loaded with.  A twister read from
   a file only shows the WIDTH of its k-mer names, ceil(k/2) hex digits (bin/KPopCount.ml:46), so a loader that
   had to infer k loads with the even candidate and, once the producer of the reads has said which k it counts
   with, sets it here (k <= the loaded k: the name -> row index of the larger k also holds every smaller hash). */
int kpop_twister_set_count_k(kpop_twister *tw, int k);
int kpop_twister_free(kpop_twister *tw);
int kpop_twister_info(const kpop_twister *tw, uint64_t *n_cols, uint32_t *n_dims, int *k,
                      uint64_t *device_bytes);
/* Bytes (part of device_bytes) of the twister's second copy of its rows AT THEIR HASHES, 0 when it keeps none.  A nearly
   complete twister of k = 13..15 and up to 32 dimensions keeps one when it fits the free memory with room to spare
   (k = 15, 16 dimensions: 137 GB beside 69 GB): the fused count -> twist of reads then needs no name -> row look-up, which
   for such a twister is a cache line of index for every cache line of row (lib/Twister.ml:151 is a Hashtbl.find_opt per
   k-mer).  kpop_tune("direct", 0 | 1 | 2) before loading: never | whenever it fits | by that rule (default).  Same results. */
int kpop_twister_direct_bytes(const kpop_twister *tw, uint64_t *bytes);

/* ------------------------------------------------------------------ twist
 * Replaces the worker closure of Twister.add_twisted_from_files,
 * lib/Twister.ml:146-188: name->column lookup (:151), acc over found k-mers
 * only (:158), duplicate k-mers summed (:160-163), normalise by acc when
 * normalize && acc<>0 (:177-178), sparse mat-vec (:183).
 * Spectra are CSR (hash, value) lines; out is n_spectra x n_dims row-major
 * (the "transposed" product of :52,:190).                                    */
int kpop_twist(const kpop_twister *tw, const uint64_t *hash, const double *value, const uint64_t *offsets,
               uint32_t n_spectra, int normalize, double *out);

/* Fused count -> twist (bin/KPopCount.ml:36-50 piped into lib/Twister.ml:146-188,
 * the README.md:606 pipeline) without materialising text spectra.            */
int kpop_count_twist(const kpop_twister *tw, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                     int content, int normalize, double *out);

/* ------------------------------------------------------------ packed bases
 * BASELINE north_star's "packed bases" at the boundary: 16 bases a 32-bit word of 2-bit codes (A 0, C 1, G 2, T 3, either case; base i
 * of the batch in bits 2 (i % 16).. of word i / 16) and one bit a base that is none of ACGTacgt (32 bases a word; such a base starts
 * no k-mer, as after Sequences.Lint.dnaize, bin/KPopCount.ml:242-245): 2.25 bits a base where every other entry point takes 8.  A host
 * that keeps its sequences packed sends 3.56 x fewer bytes over the bus -- BASELINE config 3's 1.5 GB of bases cost 26 ms of bus
 * against 9.6 ms of kernels.  kpop_pack_bases packs on the host (threads <= 0: the library chooses); on the device the words are
 * spread back to one byte a base at HBM's rate and the kernels run as they are: the ASCII entry points' results bit for bit.
 * offsets are in bases, from base 0 of the packed arrays.  Replaces the sequence side of bin/KPopCount.ml:36-50.                  */
uint64_t kpop_packed_code_words(uint64_t n_bases);   /* (n_bases + 15) / 16 */
uint64_t kpop_packed_mask_words(uint64_t n_bases);   /* (n_bases + 31) / 32 */
int kpop_pack_bases(const uint8_t *bases, uint64_t n_bases, uint32_t *codes, uint32_t *invalid, int threads);
int kpop_count_twist_packed(const kpop_twister *tw, const uint32_t *codes, const uint32_t *invalid, const uint64_t *offsets, uint32_t n_reads,
                            int content, int normalize, double *out);

/* The same pipeline with the count spelled out: the rows that kpop_count_reads(k, content, per_read = 1) followed
 * by kpop_twist would give, bit for bit, for sequences of any length, with the spectra never leaving the device.
 * k is the caller's (k <= the k the twister was loaded with: a twister file shows only the width of its k-mer names).
 * This is what KPopTwistDB runs when KPopCount hands it reads instead of text spectra (kpop_amd/host/fast_seq.h). */
int kpop_spectra_twist(const kpop_twister *tw, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                       int k, int content, int normalize, double *out);

/* ------------------------------------------------------- streaming pipeline
 * Reads in host memory -> twisted rows / distances to a set of class vectors / per-read summary in host memory: the
 * README.md:606 + :641 / :656 chain (bin/KPopCount.ml:36-50 -> lib/Twister.ml:58-206 -> lib/Matrix.ml:191-266 or
 * :691-766) as one call, with the upload of chunk c+1, the kernels of chunk c and the download of chunk c-1 running at
 * the same time on three streams (SURVEY.md 7 "pinned-memory double-buffered ingest ... never materialise").
 * `outputs` selects what crosses the bus back: a caller after -d or -s never pulls the twisted rows.  Every output
 * row depends on its own read only; results are bit-identical to kpop_dev_count_twist + kpop_dev_distance_rowwise /
 * kpop_dev_distance_summary on the whole batch.
 * A pipeline belongs to the device slot that was current at creation; twister, classes (n_classes x n_dims row-major)
 * and metric are those of kpop_count_twist / kpop_distance_rowwise (first operand = classes, as `-d` has the register
 * on the column side, lib/Matrix.ml:253).                                                                            */
#define KPOP_OUT_TWISTED 1
#define KPOP_OUT_DISTANCES 2
#define KPOP_OUT_SUMMARY 4
typedef struct kpop_pipeline kpop_pipeline;
typedef struct {
  uint32_t struct_size;      /* = sizeof(kpop_pipeline_config) */
  int content;               /* KPOP_DNA_DS | KPOP_DNA_SS */
  int normalize_counts;      /* --counts-normalize, lib/Twister.ml:177 */
  int kind;                  /* KPOP_EUCLIDEAN | KPOP_COSINE | KPOP_MINKOWSKI */
  double p;                  /* Minkowski power */
  int normalize_distances;   /* --distance-normalize, lib/Matrix.ml:197-202 */
  int outputs;               /* KPOP_OUT_* ored */
  uint32_t keep_at_most;     /* summary: --summary-keep-at-most, 0 = all */
  uint32_t max_neighbours;   /* summary: stride of the neighbour outputs */
  uint32_t chunk_reads;      /* reads per chunk, 0 = chosen from the batch (a quarter of it, 16,384..131,072, after a short first chunk) */
  uint32_t depth;            /* chunks in flight (device slots), 0 = 4 */
  uint64_t chunk_bases;      /* bases per chunk, 0 = 256 MiB (a longer sequence gets a chunk of its own) */
  int record_timeline;       /* 1: timing events around every chunk's upload, kernels and download (kpop_pipeline_timeline) */
} kpop_pipeline_config;
typedef struct {
  double *twisted;           /* n_reads x n_dims            (KPOP_OUT_TWISTED)   */
  double *distances;         /* n_reads x n_classes         (KPOP_OUT_DISTANCES) */
  double *stats;             /* n_reads x 4: mean, sd, median, MAD (KPOP_OUT_SUMMARY, as kpop_distance_summary) */
  uint32_t *n_neighbours;    /* n_reads */
  uint32_t *nb_index;        /* n_reads x max_neighbours */
  double *nb_distance;       /* n_reads x max_neighbours */
  double *nb_z;              /* n_reads x max_neighbours */
} kpop_pipeline_outputs;
int kpop_pipeline_create(const kpop_twister *tw, const double *classes, uint32_t n_classes, const double *metric,
                         const kpop_pipeline_config *cfg, kpop_pipeline **out);
/* Enqueue one batch.  bases / offsets / the output buffers must stay valid and untouched until the ticket is
   collected.  With page-locked buffers the call only enqueues (several batches may be in flight: submit the next
   before collecting the previous and the bus never idles); with pageable ones it may wait for copies.            */
int kpop_pipeline_submit(kpop_pipeline *pl, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                         const kpop_pipeline_outputs *out, uint64_t *ticket);
int kpop_pipeline_submit_packed(kpop_pipeline *pl, const uint32_t *codes, const uint32_t *invalid, const uint64_t *offsets, uint32_t n_reads,
                                const kpop_pipeline_outputs *out, uint64_t *ticket);  /* the batch in 2.25 bits a base (see "packed bases") */
int kpop_pipeline_collect(kpop_pipeline *pl, uint64_t ticket);  /* returns once that batch's outputs are in host memory */
int kpop_pipeline_run(kpop_pipeline *pl, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                      const kpop_pipeline_outputs *out);        /* submit + collect */
/* of the last submit: chunks it was cut into, whether every buffer was page-locked, slots in the ring */
int kpop_pipeline_stats(const kpop_pipeline *pl, uint32_t *chunks, int *pinned, uint32_t *depth);
/* The device-side timeline of the last submit of a pipeline created with record_timeline (call after its collect): per
   chunk six times in milliseconds from the start of the first upload -- upload start, end; kernels start, end; download
   start, end -- taken with events on the three streams.  ms holds max_chunks x 6 doubles; *n_chunks = chunks written. */
int kpop_pipeline_timeline(kpop_pipeline *pl, uint32_t max_chunks, double *ms, uint32_t *n_chunks);
int kpop_pipeline_destroy(kpop_pipeline *pl);

/* ------------------------------------------------------------ several GPUs
 * "multi-GPU sharding is internal".  After kpop_init_devices(devices, n) these calls spread one batch
 * over all n device slots from inside the library -- one host thread per device, started per call -- replacing `-T`
 * (bin/KPopTwistDB.ml:103) and the fork()ed workers of lib/Twister.ml:90-196 and lib/Matrix.ml:212-266,712-766.
 * Every sequence is independent through count and twist: reads are cut into contiguous shards
 * (kpop_shard_bounds), twister / classes / metric are replicated, results land in the caller's rows.                 */
/* rows [lo, hi) of n_items that `rank` of `world` owns: balanced, the first n_items % world ranks get one more.
   Pure host arithmetic (no GPU).                                                                                    */
int kpop_shard_bounds(uint64_t n_items, int rank, int world, uint64_t *lo, uint64_t *hi);
/* a twister on another device slot: copied device to device (xGMI where peers are enabled); onto a slot of the SAME
   GPU it is a second handle on the same arrays.  Free with kpop_twister_free.                                       */
int kpop_twister_replicate(const kpop_twister *src, int slot, kpop_twister **out);
typedef struct kpop_sharded kpop_sharded;
/* One streaming pipeline (above) per device slot; `tw` may live on any slot and is replicated to the others.
   classes / metric may be NULL for a twisted-rows-only job (metric alone is enough for the all-vs-all summary).     */
int kpop_sharded_create(const kpop_twister *tw, const double *classes, uint32_t n_classes, const double *metric,
                        const kpop_pipeline_config *cfg, kpop_sharded **out);
int kpop_sharded_slots(const kpop_sharded *sh);
/* kpop_pipeline_run over all devices: host memory to host memory, rows of shard s written by device s.  Distances
   against a reference set need no exchange between devices.  Bit-identical to one pipeline on one device.           */
int kpop_sharded_run(kpop_sharded *sh, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                     const kpop_pipeline_outputs *out);
/* kpop_spectra_twist with the reads cut over the devices (any sequence length; bit for bit the rows of kpop_count_reads
   + kpop_twist)                                                                                                      */
int kpop_sharded_spectra_twist(kpop_sharded *sh, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, int k,
                               int content, int normalize, double *out);
/* BASELINE config 4 with the reads already resident: slot s holds n_reads[s] reads in ITS HBM (d_bases[s],
   d_offsets[s] = n_reads[s] + 1 offsets into d_bases[s]; n_bases[s] bytes; max_len = longest read anywhere).  Every
   device twists its shard in `chunks` pieces and -- gather != 0 -- pushes each finished piece into every peer's copy
   of the full n_total x n_dims matrix (hipMemcpyPeerAsync on one stream per destination: the all-gather of
   SURVEY.md 8e over point-to-point xGMI links) while it twists the next; then the distances of its rows to the
   classes.  Returns when all devices are done and every copy of the matrix is complete.                             */
int kpop_sharded_resident_step(kpop_sharded *sh, const uint8_t *const *d_bases, const uint64_t *const *d_offsets,
                               const uint32_t *n_reads, const uint64_t *n_bases, uint32_t max_len, int chunks, int gather);
/* device pointers of slot `slot` after a resident step: the full matrix (read order), the slot's first row and row
   count in it, its distances to the classes (n_rows x n_classes)                                                    */
int kpop_sharded_resident_buffers(const kpop_sharded *sh, int slot, double **d_full, uint64_t *first_row, uint64_t *n_rows,
                                  double **d_distances);
/* of the last resident step on that slot: host time until its kernels were done, and the time it then still waited
   for its pushes to land (the exposed part of the exchange)                                                         */
int kpop_sharded_timings(const kpop_sharded *sh, int slot, double *ms_compute, double *ms_exposed_comm);
/* ... and its fused count->twist launches chunk by chunk (HIP events on the slot's compute stream; what a roofline of the
   in-process path is computed from): ms[0 .. *n_chunks), at most max_chunks                                          */
int kpop_sharded_chunk_timings(const kpop_sharded *sh, int slot, double *ms, int max_chunks, int *n_chunks);
/* After a resident step with gather: slot s summarises the first min(queries_per_slot, n_s) rows of its shard (0 =
   all) against ALL n_total twisted vectors (Matrix.summarize_rowwise, lib/Matrix.ml:691-766; N x N is never formed).
   One output row per query, slots in order; out_query = the query's global read number; neighbour indices are global
   read numbers.  capacity = rows the output arrays hold.                                                            */
int kpop_sharded_all_vs_all_summary(kpop_sharded *sh, uint32_t queries_per_slot, uint32_t keep_at_most, uint32_t max_neighbours,
                                    uint64_t capacity, uint64_t *n_queries_out, uint64_t *out_query, double *out_stats,
                                    uint32_t *out_n, uint32_t *out_idx, double *out_dist, double *out_z);
int kpop_sharded_destroy(kpop_sharded *sh);
/* kpop_distance_rowwise / kpop_distance_summary with the rows of the second operand cut over the device slots        */
int kpop_sharded_distance_rowwise(const double *m1, uint32_t r1, const double *m2, uint32_t r2, uint32_t n_dims,
                                  const double *metric, int kind, double p, int normalize, double *out);
int kpop_sharded_distance_summary(const double *m1, uint32_t r1, const double *m2, uint32_t r2, uint32_t n_dims,
                                  const double *metric, int kind, double p, int normalize, uint32_t keep_at_most,
                                  uint32_t max_neighbours, double *out_stats, uint32_t *out_n, uint32_t *out_idx,
                                  double *out_dist, double *out_z);

/* ------------------------------------------------------ twister generation
 * Replaces the R stage of src/KPopTwist:93-116 (library `ca`): correspondence analysis of a k-mers x spectra
 * count table.  counts is n_kmers x n_spectra row-major (what `KPopCountDB -t` exports, src/KPopTwist:38-44);
 * normalize = divide every column by its sum first (:93-94).  n_dims = min(n_kmers, n_spectra) - 1.  Outputs:
 * twisted (n_spectra x n_dims: the class positions, :98-100), inertia (n_dims, :105) and the twister
 * (n_dims x n_kmers, dims-major: exactly what kpop_twister_load takes, :110-116).  Dimension signs are
 * arbitrary, as they are in R.  The dense S'S and S*W contractions run on the f64 matrix cores.            */
int kpop_ca(const double *counts, uint64_t n_kmers, uint32_t n_spectra, int normalize, uint32_t *n_dims_out,
            double *twisted, double *inertia, double *twister);
/* development: what the eigen-solver did in the last kpop_ca / kpop_dev_ca of the calling thread's device slot.  out[0] blocked
   steps (0/1), out[1] the iteration ran on the Cholesky factor of the Gram matrix (0/1, after the pivot count), out[2] pivots at
   the rounding floor, out[3] the kernel (0 plain steps, 1..8 rows a thread of the register kernel, 9 the looped kernel), out[4]
   sweeps run, out[5] converged (0/1), out[6] the last sweep's largest cosine between two columns (the bits of the double),
   out[7] how many of the sweeps were the closing ones on G after a run on the factor (0 otherwise).  Reads host words only: no
   synchronisation.                                                                                                           */
int kpop_debug_ca(uint64_t out[8]);

/* ----------------------------------------------------------------- metric
 * Replaces Space.Distance.Metric.compute, lib/Space.ml:88-105 (called from
 * Twister.get_metrics_vector, lib/Twister.ml:208-209).  O(n_dims) host code. */
int kpop_metric_compute(int metric_kind, const double *inertia, uint32_t n_dims, double power_int,
                        double threshold, double power_ext, double *out);

/* --------------------------------------------------------------- distance
 * Replaces Base.get_normalizations + Base.get_distance_rowwise,
 * lib/Matrix.ml:42-76,191-266 (Space.Distance.compute, lib/Space.ml:182-205).
 * out is r2 x r1 row-major: out[j*r1+i] = d(m1 row i, m2 row j) (:253).      */
int kpop_distance_rowwise(const double *m1, uint32_t r1, const double *m2, uint32_t r2, uint32_t n_dims,
                          const double *metric, int kind, double p, int normalize, double *out);

/* Replaces Matrix.summarize_rowwise + summarize_distance_matrix_row,
 * lib/Matrix.ml:691-766,632-690: per m2 row the mean, sample sd, upper median
 * and MAD of its r1 distances (out_stats r2 x 4), then the keep_at_most
 * closest m1 rows, whole tie groups included (:648-649).  Neighbour outputs
 * have a fixed stride max_neighbours per row; out_n[j] is the reference's
 * eff_len (may exceed max_neighbours: entries beyond the stride are dropped).
 * keep_at_most=0 means "all" (:723-726).  The r2 x r1 matrix is never formed.
 * Lists of any length: against a first operand of more than 4,096 rows the summary kernels themselves return at most
 * 2,048 neighbours per row; a longer list (keep_at_most = all, :723-726; a tie group of thousands, :648-649) is completed
 * by the host entry points -- the row's distances sorted by (distance, column) with the device-wide radix sort.  The
 * device entry points (kpop_dev_*) report out_n and fill at most 2,048 entries of such a row.
 * Cost of a long row: its distances recomputed, an 8-pass radix sort of r1 keys, two copies and a stream synchronisation --
 * about 30 launches and ~0.3 ms a row (r1 = 100,000), one row after the other under the slot's lock.  keep_at_most = 0 against
 * more than 4,096 rows makes EVERY query row long: meant for the reference's use (a few rows inspected in full), not for
 * 100,000 queries (tens of seconds). */
int kpop_distance_summary(const double *m1, uint32_t r1, const double *m2, uint32_t r2, uint32_t n_dims,
                          const double *metric, int kind, double p, int normalize, uint32_t keep_at_most,
                          uint32_t max_neighbours, double *out_stats, uint32_t *out_n, uint32_t *out_idx,
                          double *out_dist, double *out_z);

/* Replaces Base.get_embeddings, lib/Matrix.ml:78-128 (KPopTwistDB -e): every row times metric ** (1/2, or 1/p for
 * Minkowski), then -- if normalize -- divided by its own norm under the same distance and metric (left as is when
 * that norm is 0).  out is rows x n_dims.                                                                         */
int kpop_embeddings(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p,
                    int normalize, double *out);

/* Replaces Matrix.get_splits with SplitsAlgorithm.Gaps, lib/Matrix.ml:524-600 (KPopTwistDB -p, the default algorithm):
 * per dimension the rows sorted by coordinate and the gaps between consecutive ones; all gaps by decreasing size, then
 * dimension, then position; the s-th (s < *n_splits <= max_splits) is the split { perm[out_dim[s]][0 .. out_idx[s]] }
 * with weight out_gap[s].  perm is n_dims x rows (the row order of every dimension); rows with equal coordinates stay in
 * ascending row order.  The container the reference puts splits in (BiOCamLib Trees.Splits) is declared host-side.     */
int kpop_splits_gaps(const double *embeddings, uint32_t rows, uint32_t n_dims, uint32_t max_splits, uint32_t *n_splits,
                     double *out_gap, uint32_t *out_dim, uint32_t *out_idx, uint32_t *perm);

/* Replaces Matrix.summarize_distance, lib/Matrix.ml:767-810 (KPopTwistDB -S): the same per-row summary
 * over a distance matrix that already exists (r2 rows x r1 columns, row-major).                      */
int kpop_summarize_distances(const double *dist, uint32_t r2, uint32_t r1, uint32_t keep_at_most,
                             uint32_t max_neighbours, double *out_stats, uint32_t *out_n, uint32_t *out_idx,
                             double *out_dist, double *out_z);

/* --------------------------------------------------- device-resident path
 * Same operations on buffers already in HBM; enqueue only.                   */
int kpop_dev_synth_reads(uint64_t seed, uint64_t n_reads, uint32_t read_len, uint64_t first_read,
                         uint8_t *d_bases, uint64_t *d_offsets, void *stream);
/* -L counting with everything resident (bin/KPopCount.ml:36-50), reads of up to 512 windows.  The CSR lands
   in d_out_hash / d_out_count (the caller sizes them for the worst case, one entry per window) and
   d_out_offsets (n_reads+1); d_scratch needs kpop_dev_count_reads_scratch_bytes().                        */
uint64_t kpop_dev_count_reads_scratch_bytes(uint32_t n_reads, uint32_t max_len, int k);
int kpop_dev_count_reads(const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint32_t max_len,
                         int k, int content, void *d_scratch, uint64_t *d_out_hash, uint32_t *d_out_count,
                         uint64_t *d_out_offsets, void *stream);
/* The library-owned workspace (segment partials here; distance rows of a chunk in kpop_dev_distance_summary
   against a large first operand) is one PER STREAM (per device slot), so calls on different streams may overlap;
   the first call on a stream that needs more of it than any before synchronises the device to grow it.
   kpop_dev_workspace_reserve[_stream](bytes) grows it ahead of time, after which those calls only enqueue.
   n_bases = offsets[n_reads] (size of d_bases), max_len = longest read in the batch: the host
   knows both from the offsets it uploaded (a read longer than max_len says comes back as a row of NaNs).  Reads of up to 512 windows take the one-wavefront-
   per-read kernel; longer sequences (genomes) the streaming kernel, whose segment partials
   live in a library-owned workspace (grown with hipMalloc on the first call that needs more). */
int kpop_dev_workspace_reserve(uint64_t bytes);                       /* the null stream's */
int kpop_dev_workspace_reserve_stream(uint64_t bytes, void *stream);
int kpop_dev_count_twist(const kpop_twister *tw, const uint8_t *d_bases, const uint64_t *d_offsets,
                         uint32_t n_reads, uint64_t n_bases, uint32_t max_len, int content, int normalize,
                         double *d_out, void *stream);
/* ... from the packed form (see "packed bases"): d_codes / d_invalid as kpop_pack_bases writes them, resident on the device; the bases are
   spread back to bytes into a second library-owned block of the stream (n_bases bytes), then kpop_dev_count_twist.  kpop_dev_unpack_bases
   is that first step by itself (d_bases: n_bases bytes; A C G T, N for a base marked invalid).                                        */
int kpop_dev_unpack_bases(const uint32_t *d_codes, const uint32_t *d_invalid, uint64_t n_bases, uint8_t *d_bases, void *stream);
int kpop_dev_count_twist_packed(const kpop_twister *tw, const uint32_t *d_codes, const uint32_t *d_invalid, const uint64_t *d_offsets,
                                uint32_t n_reads, uint64_t n_bases, uint32_t max_len, int content, int normalize, double *d_out, void *stream);
/* max_lines = lines of the longest spectrum of the batch, or 0 when the caller does not know: up to 512 the kernel keeps
   the columns it finds while summing the counts (lib/Twister.ml:158) for the products (:183) instead of looking them up
   twice.  A spectrum longer than a non-zero max_lines says comes back as a row of NaNs.                              */
int kpop_dev_twist(const kpop_twister *tw, const uint64_t *d_hash, const double *d_value,
                   const uint64_t *d_offsets, uint32_t n_spectra, uint64_t max_lines, int normalize,
                   double *d_out, void *stream);
/* The same twist as a dense contraction on the f64 matrix cores (v_mfma_f64_16x16x4_f64): the spectra of a batch tile
   are laid out as X[tile x n_kmers] and multiplied by the twister's rows.  2 n_kmers D flops per spectrum whatever it
   holds: worth it for many dense spectra of a small k only.  Equal to kpop_dev_twist up to rounding
   (the order of additions is the GEMM's).  d_work needs kpop_dev_twist_dense_workspace_bytes().                    */
uint64_t kpop_dev_twist_dense_workspace_bytes(const kpop_twister *tw, uint32_t n_spectra);
int kpop_dev_twist_dense(const kpop_twister *tw, const uint64_t *d_hash, const double *d_value,
                         const uint64_t *d_offsets, uint32_t n_spectra, int normalize, void *d_work, double *d_out,
                         void *stream);
/* The same for spectra whose lines ASCEND BY HASH (the order kpop_count_reads / kpop_dev_count_reads produce; repeated
   and unknown k-mers allowed): the spectra are densified inside the contraction -- 64 spectra x 128 twister rows at a
   time in LDS, v_mfma_f64_16x16x4_f64 against the twister's rows from L2 -- with no dense image in HBM.  acc
   (lib/Twister.ml:158) is applied once to the finished sums.  A spectrum whose lines do not ascend comes back as a row of
   NaNs.  Same workspace.                                                                                            */
int kpop_dev_twist_dense_sorted(const kpop_twister *tw, const uint64_t *d_hash, const double *d_value,
                                const uint64_t *d_offsets, uint32_t n_spectra, int normalize, void *d_work,
                                double *d_out, void *stream);
/* Sequences -> twisted rows with the counts handed to the contraction DENSE: for a twister of at most 36,864 k-mers
   (every canonical k-mer up to k = 8) and 256 dimensions, one block per sequence counts into an LDS table with one
   counter per twister row and writes it out as a row of u32; the contraction loads those rows (4 bytes per sequence and
   k-mer), divides by acc as it stages them (lib/Twister.ml:177-178, element by element) and multiplies on the f64 matrix
   cores.  What kpop_dev_count_twist gives, to rounding (the order of additions is the GEMM's), for batches of ASSEMBLIES
   at small k, where every spectrum holds most of the columns.  Any sequence length.                                  */
uint64_t kpop_dev_count_twist_dense_workspace_bytes(const kpop_twister *tw, uint32_t n_reads);
int kpop_dev_count_twist_dense(const kpop_twister *tw, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads,
                               int content, int normalize, void *d_work, double *d_out, void *stream);
/* kpop_ca on device-resident data: d_counts (n_kmers x n_spectra, row-major, not modified) in, d_twisted (n_spectra x
   n_dims), d_inertia (n_dims) and d_twister (n_dims x n_kmers, dims-major) out, all device pointers; *n_dims_out is a
   host word.  d_work needs kpop_dev_ca_workspace_bytes() (the standardised copy of the table).  The weights of the
   columns and the order of the eigenvalues are host work between launches: the call synchronises `stream` on the way
   and has completed when it returns.                                                                                */
uint64_t kpop_dev_ca_workspace_bytes(uint64_t n_kmers, uint32_t n_spectra);
/* (d_work == d_counts is allowed: the table is then standardised where it stands and is lost) */
int kpop_dev_ca(const double *d_counts, uint64_t n_kmers, uint32_t n_spectra, int normalize, void *d_work,
                uint32_t *n_dims_out, double *d_twisted, double *d_inertia, double *d_twister, void *stream);
/* What KPopTwist does to the table between the transformation and the analysis (src/KPopTwist:76-91: a keep list, a
   sample, a threshold on the row sums), on a row-major k-mers x spectra table that stays on the device: sums of the
   rows (lane-strided partial sums and a fixed tree per row) and of the columns (slabs of rows added in order), and the
   rows d_rows[0 .. n_sel) copied, in that order, into d_out (n_sel x n_cols).                                          */
int kpop_dev_table_row_sums(const double *d_table, uint64_t n_rows, uint32_t n_cols, double *d_out, void *stream);
int kpop_dev_table_col_sums(const double *d_table, uint64_t n_rows, uint32_t n_cols, double *d_out, void *stream);
int kpop_dev_table_gather_rows(const double *d_table, uint32_t n_cols, const uint64_t *d_rows, uint64_t n_sel,
                               double *d_out, void *stream);
/* Distance workspace: row norms and the pre-normalised copies a/n_i, b/n_j of
   both operands (the per-element divisions of lib/Matrix.ml:247-249, done once).
   kpop_dev_distance_workspace_bytes gives the size d_work must have.          */
uint64_t kpop_dev_distance_workspace_bytes(uint32_t r1, uint32_t r2, uint32_t n_dims);
int kpop_dev_distance_rowwise(const double *d_m1, uint32_t r1, const double *d_m2, uint32_t r2,
                              uint32_t n_dims, const double *d_metric, int kind, double p, int normalize,
                              void *d_work, double *d_out, void *stream);
/* Base.get_normalizations, lib/Matrix.ml:42-76: the norms of the rows of one operand under the distance and metric
   (0 -> 1, :67).  A caller that measures many batches against ONE first operand (the class vectors) computes its norms
   once and hands them to kpop_dev_distance_rowwise_norms with every batch (d_norms1 = NULL: computed inside, = plain
   kpop_dev_distance_rowwise; they are used where the kernel divides while staging -- fewer than 128 rows in the first
   operand, normalize set -- and recomputed otherwise).                                                              */
int kpop_dev_row_norms(const double *d_m, uint32_t rows, uint32_t n_dims, const double *d_metric, int kind, double p,
                       double *d_norms, void *stream);
int kpop_dev_distance_rowwise_norms(const double *d_m1, uint32_t r1, const double *d_norms1, const double *d_m2, uint32_t r2,
                                    uint32_t n_dims, const double *d_metric, int kind, double p, int normalize,
                                    void *d_work, double *d_out, void *stream);
int kpop_dev_distance_summary(const double *d_m1, uint32_t r1, const double *d_m2, uint32_t r2,
                              uint32_t n_dims, const double *d_metric, int kind, double p, int normalize,
                              uint32_t keep_at_most, uint32_t max_neighbours, void *d_work,
                              double *d_out_stats, uint32_t *d_out_n, uint32_t *d_out_idx,
                              double *d_out_dist, double *d_out_z, void *stream);

int kpop_dev_summarize_distances(const double *d_dist, uint32_t r2, uint32_t r1, uint32_t keep_at_most,
                                 uint32_t max_neighbours, double *d_out_stats, uint32_t *d_out_n,
                                 uint32_t *d_out_idx, double *d_out_dist, double *d_out_z, void *stream);

/* ------------------------------------------------- resident reference set
 * A first operand of the distance calls that is prepared ONCE and queried many times (a database of genomes, the class
 * vectors of a classifier).  The reference computes the norms of both operands on every invocation
 * (Base.get_normalizations, lib/Matrix.ml:42-76, called from get_distance_rowwise :191-266 and summarize_rowwise
 * :691-766); a set keeps, in device memory, the rows and everything about them that does not depend on the query rows:
 * norms (0 -> 1, :67) and sums before the scale, the matrix-core summary's scalars, and -- made by the first call that
 * needs them -- the divided copy a / n (:248) and the evenly spaced sample of rows.  Every call on a set returns the
 * arrays of the unprepared call on the same rows BIT FOR BIT, under whatever kpop_tune settings hold at the time of the
 * call: each piece comes out of the kernel the unprepared call runs, over the same row.
 * A set belongs to the device slot that was current when it was made, is used by one host thread at a time, and
 * kpop_tune settings change only while no call on it is in flight.                                                    */
typedef struct kpop_refset kpop_refset;
/* Rows copied from host memory (replaces the first operand of lib/Matrix.ml:191-266 and :691-766 when one register is
   queried repeatedly).  capacity_rows >= r1 (0 = r1) is the room for kpop_refset_append; r1 = 0 makes an empty set.
   n_dims of 32,768 and more: KPOP_ERR_UNSUPPORTED (as kpop_dev_row_norms).  Synchronises.                            */
int kpop_refset_create(const double *m1, uint32_t r1, uint32_t n_dims, const double *metric, int kind, double p,
                       int normalize, uint32_t capacity_rows, kpop_refset **out);
/* Rows and metric already in device memory, BORROWED: not copied, not freed; the caller keeps them alive and unchanged
   for the life of the set.  No append.  The preparation pass (lib/Matrix.ml:42-76 over the rows) runs on `stream`,
   which the call waits for.                                                                                          */
int kpop_dev_refset_wrap(const double *d_m1, uint32_t r1, uint32_t n_dims, const double *d_metric, int kind,
                         double p, int normalize, void *stream, kpop_refset **out);
/* n_rows more rows from host memory (Matrix.merge_rowwise, lib/Matrix.ml:130-147, for a register that grows): a copy and
   one pass over the NEW rows.  r1 + n_rows > capacity: KPOP_ERR_CAPACITY, the set stays as it was.  Waits for the device. */
int kpop_refset_append(kpop_refset *rs, const double *rows, uint32_t n_rows);
/* any of the outputs may be NULL; device_bytes counts everything the set has allocated so far */
int kpop_refset_info(const kpop_refset *rs, uint32_t *r1, uint32_t *n_dims, uint32_t *capacity_rows,
                     uint64_t *device_bytes);
int kpop_refset_free(kpop_refset *rs);
/* kpop_distance_rowwise / kpop_distance_summary (lib/Matrix.ml:191-266 / :691-766) with the set as first operand: only
   the query rows cross the bus.  Long neighbour lists are completed as there.                                        */
int kpop_refset_distance_rowwise(kpop_refset *rs, const double *m2, uint32_t r2, double *out);
int kpop_refset_distance_summary(kpop_refset *rs, const double *m2, uint32_t r2, uint32_t keep_at_most,
                                 uint32_t max_neighbours, double *out_stats, uint32_t *out_n, uint32_t *out_idx,
                                 double *out_dist, double *out_z);
/* kpop_dev_distance_rowwise / kpop_dev_distance_summary with the set as first operand; enqueue only (a piece of the set
   that the call's route needs and nobody has made yet is made on `stream`, other streams wait for it on an event).
   d_work holds the QUERY side alone: kpop_dev_refset_workspace_bytes does not grow with the set.                     */
uint64_t kpop_dev_refset_workspace_bytes(const kpop_refset *rs, uint32_t r2);
int kpop_dev_refset_distance_rowwise(kpop_refset *rs, const double *d_m2, uint32_t r2, void *d_work, double *d_out,
                                     void *stream);
int kpop_dev_refset_distance_summary(kpop_refset *rs, const double *d_m2, uint32_t r2, uint32_t keep_at_most,
                                     uint32_t max_neighbours, void *d_work, double *d_out_stats, uint32_t *d_out_n,
                                     uint32_t *d_out_idx, double *d_out_dist, double *d_out_z, void *stream);

/* ------------------------------------------------- neighbours within a distance (range queries on a resident set)
 * Every row of the set within max_distance of a query row: H_j = { i < r1 : d(j, i) <= max_distance }, where d is the
 * reference chain's distance (lib/Space.ml:182-205 with the adaptors of lib/Matrix.ml:243-250) -- the bits
 * kpop_refset_distance_rowwise writes under kpop_tune("distance_mfma", 0) -- whatever kpop_tune says.  A row's list is in
 * ascending (distance, index) order with -0 as +0: the multimap order of summarize_distance_matrix_row
 * (lib/Matrix.ml:632-690, the order :641-650), cut at a distance where the summary cuts at a count; the reference's
 * Space.Distance.Iterator (lib/Space.ml:231-487) bounds its pairs by a max_distance_component in the same way.  A NaN
 * distance is never a hit; max_distance may be +inf, a negative one gives empty lists, NaN is KPOP_ERR_INVALID.
 * CSR layout: out_offsets[r2 + 1] (out_offsets[0] = 0), out_idx[] and out_dist[] of out_offsets[r2] entries.  The same
 * bits on every run.  out_offsets is always complete and exact; r1 = 0 and r2 = 0 give all-zero offsets.  The r2 x r1
 * matrix is never formed.  The set's limits, slot and thread ownership hold as for every call on a set.               */
/* (lib/Matrix.ml:632-690 cut at a distance; lib/Space.ml:182-205.)  out_offsets[r2] > capacity: KPOP_ERR_CAPACITY, out_idx
   and out_dist untouched.  out_idx == out_dist == NULL: count only, KPOP_OK.  Synchronises.                           */
int kpop_neighbours_within(kpop_refset *rs, const double *m2, uint32_t r2, double max_distance, uint64_t capacity,
                           uint64_t *out_offsets, uint32_t *out_idx, double *out_dist);
/* bytes of d_work for kpop_dev_neighbours_within (the lists of lib/Matrix.ml:632-690 cut at a distance, see the block above): the
   query side and 32 bytes a list entry of `capacity`; does not grow with the set                                     */
uint64_t kpop_dev_neighbours_within_workspace_bytes(const kpop_refset *rs, uint32_t r2, uint64_t capacity);
/* (lib/Matrix.ml:632-690 cut at a distance; lib/Space.ml:182-205.)  Enqueues only.  The lists are written only when they
   fit `capacity`: the caller reads d_out_offsets[r2].  NULL lists: count only.                                        */
int kpop_dev_neighbours_within(kpop_refset *rs, const double *d_m2, uint32_t r2, double max_distance, uint64_t capacity,
                               void *d_work, uint64_t *d_out_offsets, uint32_t *d_out_idx, double *d_out_dist,
                               void *stream);
/* unprepared convenience (lib/Matrix.ml:191-266 for the distances, :632-690 for the order): a temporary set over m1, then
   kpop_neighbours_within                                                                                              */
int kpop_distance_within(const double *m1, uint32_t r1, const double *m2, uint32_t r2, uint32_t n_dims,
                         const double *metric, int kind, double p, int normalize, double max_distance,
                         uint64_t capacity, uint64_t *out_offsets, uint32_t *out_idx, double *out_dist);

/* ------------------------------------------------- clusters at a distance (connected components of a resident set)
 * The graph on the set's r1 rows: i < j are joined iff d(j, i) <= max_distance, where d is the reference chain's distance
 * (lib/Space.ml:182-205 with the adaptors of lib/Matrix.ml:243-250) -- the bits kpop_refset_distance_rowwise writes to
 * out[j][i] under kpop_tune("distance_mfma", 0) when the set's own rows are the query -- whatever kpop_tune says.  The chain
 * is symmetric bit for bit, so only i < j is examined, and i == j never.  A NaN distance joins nothing: a row with a NaN in
 * it is a cluster of its own.  labels[i] is the SMALLEST row index of row i's connected component (labels[i] <= i,
 * labels[labels[i]] == labels[i]), *n_clusters the number of i with labels[i] == i: the same bits on every run.
 * max_distance negative: every row alone; +inf: every pair whose distance is a number; NaN: KPOP_ERR_INVALID.  r1 = 0:
 * KPOP_OK and *n_clusters = 0.  Neither the r1 x r1 matrix nor any neighbour list is formed: the transitive closure of
 * kpop_neighbours_within's lists of the set against itself, without them.
 * known_rows <= r1 (0: none) says that labels[0 .. known_rows) hold, on entry, what this call returned for the first
 * known_rows rows at the same max_distance: pairs of two such rows are not examined, and the result is that of
 * known_rows = 0, bit for bit -- after kpop_refset_append a re-cluster costs new x all, not all x all.  known_rows = r1
 * examines nothing.  The set's limits, slot and thread ownership hold as for every call on a set.                      */
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  labels: r1 entries, the first known_rows read, all written.  The incoming
   labels are checked against the two invariants above (KPOP_ERR_INVALID).  Synchronises.                              */
int kpop_clusters_within(kpop_refset *rs, double max_distance, uint32_t known_rows, uint32_t *labels,
                         uint32_t *n_clusters);
/* bytes of d_work for kpop_dev_clusters_within (lib/Space.ml:182-205 over the set against itself, see the block above): a
   constant -- the union-find forest lives in d_labels, the divided copy in the set                                    */
uint64_t kpop_dev_clusters_within_workspace_bytes(const kpop_refset *rs);
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Enqueues only.  d_labels[r1] (the first known_rows TRUSTED to be an
   earlier result), d_n_clusters[1].                                                                                   */
int kpop_dev_clusters_within(kpop_refset *rs, double max_distance, uint32_t known_rows, void *d_work, uint32_t *d_labels,
                             uint32_t *d_n_clusters, void *stream);
/* unprepared convenience (lib/Matrix.ml:191-266 for the distances, m against itself): a temporary set over m, then
   kpop_clusters_within with known_rows = 0                                                                            */
int kpop_distance_clusters(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p,
                           int normalize, double max_distance, uint32_t *labels, uint32_t *n_clusters);

/* ------------------------------------------------- single-linkage tree (minimum spanning forest of a resident set)
 * The graph of the block above: nodes are the set's r1 rows, d(j, i) the reference chain's distance (lib/Space.ml:182-205
 * with the adaptors of lib/Matrix.ml:243-250), symmetric bit for bit, so that an edge is an unordered pair written i < j;
 * a NaN distance is no edge; no kpop_tune setting is read.  An edge exists iff d <= max_distance (+inf: every pair whose
 * distance is a number, +inf distances included; negative: none; NaN: KPOP_ERR_INVALID).  Edges are ordered by
 * (d with -0 taken as +0, i, j) ascending -- a strict total order, under which the minimum spanning forest is UNIQUE: the
 * result is defined without reference to an algorithm and is the same bits on every run.  *n_edges = r1 - (the number of
 * components at max_distance); edge_i[e] < edge_j[e] with edge_dist[e] (a zero as +0), e in [0, *n_edges), listed in
 * that order; room is the caller's: r1 - 1 entries each (none for r1 <= 1).  labels[r1] (may be NULL) are what
 * kpop_clusters_within(rs, max_distance, 0, ...) returns, bit for bit.  r1 = 0: KPOP_OK and *n_edges = 0.
 * THE CUT: for any T <= max_distance, uniting the ends of the edges with edge_dist <= T (kpop_forest_cut) gives exactly
 * the labels and the count of kpop_clusters_within at T -- one forest answers every threshold.  Neither the r1 x r1
 * matrix nor a neighbour list is formed.  The set's limits, slot and thread ownership hold as for every call on a set. */
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Host arrays.  Synchronises.                                           */
int kpop_spanning_forest(kpop_refset *rs, double max_distance, uint32_t *n_edges, uint32_t *edge_i, uint32_t *edge_j,
                         double *edge_dist, uint32_t *labels);
/* bytes of d_work for kpop_dev_spanning_forest (lib/Space.ml:182-205 over the set against itself, see the block above),
   for the set's r1 at the time of the call                                                                             */
uint64_t kpop_dev_spanning_forest_workspace_bytes(const kpop_refset *rs);
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Enqueues only: ceil(log2 r1) rounds, each of which returns at once
   when the round before added no edge; nothing is read back.  d_n_edges[1], d_edge_i / d_edge_j / d_edge_dist[r1 - 1]
   (the first *d_n_edges written), d_labels[r1] or NULL.                                                                 */
int kpop_dev_spanning_forest(kpop_refset *rs, double max_distance, void *d_work, uint32_t *d_n_edges, uint32_t *d_edge_i,
                             uint32_t *d_edge_j, double *d_edge_dist, uint32_t *d_labels, void *stream);
/* unprepared convenience (lib/Matrix.ml:191-266 for the distances, m against itself): a temporary set over m, then
   kpop_spanning_forest                                                                                                  */
int kpop_distance_spanning_forest(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind,
                                  double p, int normalize, double max_distance, uint32_t *n_edges, uint32_t *edge_i,
                                  uint32_t *edge_j, double *edge_dist, uint32_t *labels);
/* pure host arithmetic, no GPU and no kpop_init: the connected components of ANY list of edges i < j < r1 (a forest or
   not) cut at T -- the edges with edge_dist <= T united (a NaN joins nothing), labels[i] the smallest row index of row i's
   component, *n_clusters their number.  Over a forest of kpop_spanning_forest and T <= its max_distance: the labels of
   the reference chain's distances (lib/Space.ml:182-205; lib/Matrix.ml:243-250) at T.  KPOP_ERR_INVALID for a NaN T and
   for an edge that is not i < j < r1.                                                                                   */
int kpop_forest_cut(uint32_t r1, uint32_t n_edges, const uint32_t *edge_i, const uint32_t *edge_j,
                    const double *edge_dist, double T, uint32_t *labels, uint32_t *n_clusters);

/* ------------------------------------------------- k-NN vote (classify query rows against a labelled resident set)
 * The classifier of the reference's README (README.md:758-775: `--keep-at-most k -s Test Train`, then a count of the
 * classes among the listed neighbours), on the device.  class_of[r1] gives every row of the set a class in
 * [0, n_classes); the labels travel with the call, the set stays what it is.  d(j, i) is the reference chain's distance
 * (lib/Space.ml:182-205 with the adaptors of lib/Matrix.ml:243-250) -- the bits kpop_refset_distance_rowwise writes under
 * kpop_tune("distance_mfma", 0) -- whatever kpop_tune says.  THE LIST of query row j: the set rows whose distance to j is
 * a number, ordered by (d with -0 taken as +0, index) ascending; its first k, plus every further row whose distance
 * equals the k-th one -- eff_len of summarize_distance_matrix_row (lib/Matrix.ml:641-650): whole tie groups; fewer than
 * k numbers: all of them.  A NaN distance is never a neighbour (a summary line of a row that holds a NaN differs: there
 * the NaN takes a place in the order); +inf is a number.  THE VOTE: out_n[j] the length of the list, out_class[j] the
 * class with the most members in it -- among classes with equally many, the one whose nearest member comes first in the
 * list's order (README.md:775) --, out_votes[j] its count, out_first_dist[j] (may be NULL) the distance of that nearest
 * member, bits kept.  An empty list (r1 = 0, or every distance a NaN): KPOP_NO_CLASS, 0, 0, NaN.  The result is a function
 * of the distances alone: the same bits on every run.  Neither the r2 x r1 matrix nor a neighbour list longer than k a
 * row is formed; 12-20 bytes a query row cross the bus.  k in 1..128 (0: KPOP_ERR_INVALID, more: KPOP_ERR_UNSUPPORTED);
 * n_classes in 1..65,535 (more: KPOP_ERR_UNSUPPORTED).  The set's limits, slot and thread ownership hold as for every
 * call on a set.  The distances are the exact chain's on the vector pipe, one pass over the pairs (a second for the rows
 * whose tie group at the k-th distance is longer than the k slots hold).  MEASURED (k = 5, profiles/knn_vote.md): SLOWER
 * than kpop_dev_refset_distance_summary, which locates its neighbours on the matrix cores, at 256 x 1,000,000 x 64 (4.5
 * against 2.0 ms) and at 256 x 650,000 x 1,635 (44 against 11 ms); faster at 4,096 x 100,000 x 64 (5.8 against 6.7 ms) and
 * on a set of 600,000 identical rows (11.7 against 33.6 ms).                                                            */
#define KPOP_NO_CLASS 0xFFFFFFFFu
/* (lib/Matrix.ml:641-650 for the list; lib/Space.ml:182-205 for the distances.)  Host arrays; class_of[i] >= n_classes is
   KPOP_ERR_INVALID.  The query rows go through in chunks that keep the workspace bounded.  Synchronises.               */
int kpop_knn_vote(kpop_refset *rs, const uint32_t *class_of, uint32_t n_classes, const double *m2, uint32_t r2,
                  uint32_t k, uint32_t *out_class, uint32_t *out_votes, uint32_t *out_n, double *out_first_dist);
/* bytes of d_work for kpop_dev_knn_vote (the lists of lib/Matrix.ml:641-650, see the block above): the query side, 12 k
   bytes of lists a query row and segment of the set's columns (at most 128 segments, fewer the more query rows: about
   512 strips of rows x segments in all) and 8 n_classes bytes of tie tables a query row; does not grow with the set   */
uint64_t kpop_dev_knn_vote_workspace_bytes(const kpop_refset *rs, uint32_t r2, uint32_t k, uint32_t n_classes);
/* (lib/Matrix.ml:641-650; lib/Space.ml:182-205.)  Enqueues only: reads nothing back, allocates nothing.  d_class_of[r1] is
   TRUSTED; every table access is guarded: a row whose class is >= n_classes counts in d_out_n and votes for nobody.    */
int kpop_dev_knn_vote(kpop_refset *rs, const uint32_t *d_class_of, uint32_t n_classes, const double *d_m2, uint32_t r2,
                      uint32_t k, void *d_work, uint32_t *d_out_class, uint32_t *d_out_votes, uint32_t *d_out_n,
                      double *d_out_first_dist, void *stream);
/* unprepared convenience (lib/Matrix.ml:191-266 for the distances, :641-650 for the list): a temporary set over m1, then
   kpop_knn_vote                                                                                                        */
int kpop_distance_knn_vote(const double *m1, uint32_t r1, const uint32_t *class_of, uint32_t n_classes, const double *m2,
                           uint32_t r2, uint32_t n_dims, const double *metric, int kind, double p, int normalize,
                           uint32_t k, uint32_t *out_class, uint32_t *out_votes, uint32_t *out_n,
                           double *out_first_dist);

/* ------------------------------------------------- k-NN validation (leave-out votes of a labelled set, many k in one pass)
 * How good is a labelled set as a classifier, which k (the README leaves it open: "of course the number of neighbours
 * could be chosen to be different", README.md:770), and which rows disagree with their own neighbours (its classes are
 * "heterogeneous collections", README.md:1087)?  The reference answers by a hold-out run and awk (README.md:1077-1085).
 * Everything not said here is the block above's: the distance (lib/Space.ml:182-205 with the adaptors of
 * lib/Matrix.ml:243-250), the key order (d with -0 as +0, index), whole tie groups (lib/Matrix.ml:641-650), a NaN never a
 * neighbour, +inf a number, the vote's tie-break (README.md:773-775).
 * VOTES FOR MANY k (*_knn_ks_vote; RefSet.knn_vote_ks in Python): ks[n_ks] strictly ascending, each in 1..128, n_ks in 1..32; the outputs are
 * [n_ks][r2] row-major, and slice t is bit for bit what kpop_knn_vote returns for k = ks[t].  One pass over the pairs at
 * K = ks[n_ks-1] (and one for the rows whose tie group at the K-th distance is longer than the slots hold) serves every
 * t: the launches that do distance arithmetic do not depend on n_ks.
 * LEAVE-OUT VOTES (*_knn_validate): the query rows are the set's own rows.  Left out of row j's list: row j itself when
 * group_of == NULL (leave-one-out); otherwise every row i with group_of[i] == group_of[j], j among them (k-fold
 * cross-validation: group_of = the fold; "sequences of one outbreak do not vote for each other": group_of = the
 * outbreak).  By index or group, never by distance: a duplicate of j in another group stays, at distance 0.  d(j, i) is
 * the bits kpop_refset_distance_rowwise writes to out[j][i] under kpop_tune("distance_mfma", 0) with the set's rows as
 * the query: kpop_clusters_within's definition.  Per ks[t], [n_ks][rows] row-major: out_class, out_votes, out_n,
 * out_first_dist (may be NULL), and out_correct[t], the rows with out_class == class_of[row] (KPOP_NO_CLASS is never
 * correct).  A row with no list -- r1 = 1, every other distance a NaN, the whole set in its group -- gives
 * KPOP_NO_CLASS, 0, 0, NaN.  A function of the distances, classes and groups alone: the same bits on every run; no
 * kpop_tune setting is read.
 * ERRORS: ks empty, not strictly ascending or holding a 0: KPOP_ERR_INVALID; a k above 128 or n_ks > 32:
 * KPOP_ERR_UNSUPPORTED; n_classes as above.  MEASURED (profiles/knn_validate.md; 100,000 x 64, six k up to 31): the
 * validation takes 123.8 ms, one kpop_dev_knn_vote over the same rows at k = 31 takes 122.6 ms, six of them 692.8 ms.   */
/* (lib/Matrix.ml:641-650 for the list; lib/Space.ml:182-205 for the distances.)  Host arrays; class_of[i] >= n_classes is
   KPOP_ERR_INVALID.  The query rows go through in chunks that keep the workspace bounded.  Synchronises.               */
int kpop_knn_ks_vote(kpop_refset *rs, const uint32_t *class_of, uint32_t n_classes, const double *m2, uint32_t r2,
                     const uint32_t *ks, uint32_t n_ks, uint32_t *out_class, uint32_t *out_votes, uint32_t *out_n,
                     double *out_first_dist);
/* bytes of d_work for kpop_dev_knn_ks_vote (the lists of lib/Matrix.ml:641-650): kpop_dev_knn_vote_workspace_bytes at
   k = k_max, the largest k; does not grow with the set or with n_ks                                                    */
uint64_t kpop_dev_knn_ks_vote_workspace_bytes(const kpop_refset *rs, uint32_t r2, uint32_t k_max, uint32_t n_classes);
/* (lib/Matrix.ml:641-650; lib/Space.ml:182-205.)  Enqueues only: reads nothing back, allocates nothing.  ks is in HOST
   memory and is handed to the kernels by value; everything else is device memory.  d_class_of[r1] is TRUSTED, every table
   access guarded, as in kpop_dev_knn_vote.  d_out_*: [n_ks][r2]                                                        */
int kpop_dev_knn_ks_vote(kpop_refset *rs, const uint32_t *d_class_of, uint32_t n_classes, const double *d_m2, uint32_t r2,
                         const uint32_t *ks, uint32_t n_ks, void *d_work, uint32_t *d_out_class, uint32_t *d_out_votes,
                         uint32_t *d_out_n, double *d_out_first_dist, void *stream);
/* (lib/Matrix.ml:641-650 for the list; lib/Space.ml:182-205 for the distances; README.md:1077-1085 for the accuracy.)
   Host arrays, [n_ks][r1] and out_correct[n_ks]; class_of[i] >= n_classes is KPOP_ERR_INVALID; group_of NULL:
   leave-one-out.  The set's rows go through in ranges that keep the workspace bounded, out_correct summed over them;
   the query side of a range is the set's own divided copy: no second copy of the rows.  Synchronises.                  */
int kpop_knn_validate(kpop_refset *rs, const uint32_t *class_of, uint32_t n_classes, const uint32_t *group_of,
                      const uint32_t *ks, uint32_t n_ks, uint32_t *out_class, uint32_t *out_votes, uint32_t *out_n,
                      double *out_first_dist, uint64_t *out_correct);
/* bytes of d_work for kpop_dev_knn_validate over n_rows rows (the lists of lib/Matrix.ml:641-650): the vote's without a
   query side; does not grow with the set or with n_ks                                                                  */
uint64_t kpop_dev_knn_validate_workspace_bytes(const kpop_refset *rs, uint32_t n_rows, uint32_t k_max, uint32_t n_classes);
/* (lib/Matrix.ml:641-650; lib/Space.ml:182-205.)  Rows first_row .. first_row + n_rows of the set against the whole set
   (beyond r1: KPOP_ERR_INVALID).  Enqueues only: reads nothing back, allocates nothing.  ks in HOST memory, by value to
   the kernels.  d_class_of[r1] TRUSTED, every table access guarded; d_group_of[r1] or NULL.  d_out_*: [n_ks][n_rows];
   d_out_correct[n_ks] is WRITTEN for this range, not accumulated                                                       */
int kpop_dev_knn_validate(kpop_refset *rs, const uint32_t *d_class_of, uint32_t n_classes, const uint32_t *d_group_of,
                          uint32_t first_row, uint32_t n_rows, const uint32_t *ks, uint32_t n_ks, void *d_work,
                          uint32_t *d_out_class, uint32_t *d_out_votes, uint32_t *d_out_n, double *d_out_first_dist,
                          uint64_t *d_out_correct, void *stream);
/* unprepared convenience (lib/Matrix.ml:191-266 for the distances, m against itself; :641-650 for the list): a temporary
   set over m, then kpop_knn_validate                                                                                   */
int kpop_distance_knn_validate(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p,
                               int normalize, const uint32_t *class_of, uint32_t n_classes, const uint32_t *group_of,
                               const uint32_t *ks, uint32_t n_ks, uint32_t *out_class, uint32_t *out_votes,
                               uint32_t *out_n, double *out_first_dist, uint64_t *out_correct);

/* ------------------------------------------------- representatives at a distance (the greedy cover of a resident set)
 * Thinning (dereplication, leader clustering): keep one row per neighbourhood of radius max_distance, in row order, and
 * say which kept row stands for each dropped one.  d(j, i) is the reference chain's distance (lib/Space.ml:182-205 with
 * the adaptors of lib/Matrix.ml:243-250) -- the bits kpop_refset_distance_rowwise writes under
 * kpop_tune("distance_mfma", 0) when the set's own rows are the query -- whatever kpop_tune says; symmetric bit for bit;
 * a NaN distance is within nothing.  Row i is a REPRESENTATIVE iff no representative r < i has d(i, r) <= max_distance
 * (row 0 always is): the lexicographically first maximal independent set of kpop_clusters_within's graph.  For a
 * representative rep_of[i] = i and rep_dist[i] = +0; otherwise rep_of[i] is the representative r < i within max_distance
 * that is least under (d with -0 taken as +0, r) -- the nearest EARLIER one, ties to the smaller index, even when a later
 * representative is nearer -- and rep_dist[i] that distance, a zero written as +0.  rep_of[i] <= i,
 * rep_of[rep_of[i]] == rep_of[i], *n_reps the number of i with rep_of[i] == i; two representatives lie farther apart
 * than max_distance (or at a NaN), every other row within it of its own: these properties determine the result, the
 * same bits on every run.  It DEPENDS ON THE ROW ORDER, by design, and rows 0 .. n of it on no later row.
 * max_distance negative: every row stands for itself; +inf: a row is a representative iff its distance to every earlier
 * one is NaN; NaN: KPOP_ERR_INVALID.  r1 = 0: KPOP_OK and *n_reps = 0.  A row with a NaN in it stands for itself alone.
 * known_rows <= r1 (0: none) says that rep_of[0 .. known_rows) hold, on entry, what this call returned for those rows at
 * the same max_distance: they are not examined against each other, rep_dist[0 .. known_rows) is neither read nor
 * written, and the result is that of known_rows = 0, bit for bit -- after kpop_refset_append a re-thin costs new rows x
 * representatives.  known_rows = r1 examines nothing.  Semantics: INTEGRATION.md 6h; timings: profiles/representatives.md. */
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  rep_of: r1 entries, the first known_rows read and checked against the
   two invariants above (KPOP_ERR_INVALID), the others written; rep_dist: r1 entries or NULL.  Synchronises.            */
int kpop_representatives_within(kpop_refset *rs, double max_distance, uint32_t known_rows, uint32_t *rep_of,
                                double *rep_dist, uint32_t *n_reps);
/* bytes of d_work for kpop_dev_representatives_within (lib/Space.ml:182-205 over the set against itself, see the block
   above), for the set's r1 at the time of the call: the representatives' indices and a step's tables; no copy of rows  */
uint64_t kpop_dev_representatives_within_workspace_bytes(const kpop_refset *rs);
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Enqueues only, reads nothing back.  d_rep_of[r1] (the first known_rows
   TRUSTED to be an earlier result), d_rep_dist[r1] or NULL, d_n_reps[1].                                               */
int kpop_dev_representatives_within(kpop_refset *rs, double max_distance, uint32_t known_rows, void *d_work,
                                    uint32_t *d_rep_of, double *d_rep_dist, uint32_t *d_n_reps, void *stream);
/* unprepared convenience (lib/Matrix.ml:191-266 for the distances, m against itself): a temporary set over m, then
   kpop_representatives_within with known_rows = 0                                                                      */
int kpop_distance_representatives(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind,
                                  double p, int normalize, double max_distance, uint32_t *rep_of, double *rep_dist,
                                  uint32_t *n_reps);

/* ------------------------------------------------- DBSCAN on a resident set (core rows, border rows and noise)
 * The density-based cut of kpop_clusters_within's graph: a cluster is where at least min_pts rows sit within eps of each
 * other, a row on the rim belongs to the cluster it touches, everything else is noise -- one pair of stray rows between
 * two lineages no longer chains them into one.  d(j, i) is the reference chain's distance (lib/Space.ml:182-205 with the
 * adaptors of lib/Matrix.ml:243-250) -- the bits kpop_refset_distance_rowwise writes under kpop_tune("distance_mfma", 0)
 * when the set's own rows are the query -- whatever kpop_tune says; symmetric bit for bit, so only i < j is examined and
 * the pair i == j never; a NaN distance is within nothing.  degree[i] = 1 + #{ j != i : d(i, j) <= eps }: the row counts
 * itself, whatever its values are (a row with a NaN in it has degree 1).  Row i is a CORE row iff degree[i] >= min_pts.
 * THE CLUSTERS are the connected components of the graph restricted to the core rows; a core row's label is the smallest
 * core row index of its component, and core_of[i] = i.  A row that is not core and has a core row within eps is a BORDER
 * row: core_of[i] is the core row least under (d with -0 taken as +0, index) among those within eps -- the nearest, ties
 * to the smaller ROW INDEX, not to the smaller label -- and labels[i] = labels[core_of[i]].  A border row joins nothing:
 * two clusters that share only a border row stay two.  Every other row is NOISE: labels[i] = core_of[i] = KPOP_NOISE.
 * counts[0]: the clusters (core rows with labels[i] == i); counts[1]: the core rows; counts[2]: the noise rows.  For a
 * row that is not noise labels[labels[i]] == labels[i] and labels[i] is a core row; for a core row labels[i] <= i (a
 * border row's label may exceed its index).  Integer sums, canonical labels, the minimum of a strict total order: a
 * function of the distances alone, the same bits on every run.
 * eps NaN: KPOP_ERR_INVALID; eps negative: every degree is 1 (min_pts = 1: every row a cluster of its own; otherwise all
 * noise); +inf: every pair whose distance is a number, +inf included.  min_pts = 0: KPOP_ERR_INVALID; min_pts > r1: all
 * noise.  r1 = 0: KPOP_OK and the counts all zero.  min_pts = 1: the labels of kpop_clusters_within(eps), bit for bit,
 * and no noise; min_pts = 2: a component of two or more rows keeps that label and a singleton is noise; for eps >= 0 and
 * a row of finite values degree[i] is the length of row i's list in kpop_neighbours_within(the set's rows, eps).
 * THERE IS NO known_rows: a new row can turn old rows that were not core into core rows, so no earlier result is a valid
 * start; after kpop_refset_append the call is made again in full.  Neither the r1 x r1 matrix nor a neighbour list is
 * formed.  The set's limits, slot and thread ownership hold as for every call on a set.  Semantics: INTEGRATION.md 6i;
 * timings: profiles/dbscan.md. */
#define KPOP_NOISE 0xFFFFFFFFu
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Host arrays: labels[r1], core_of[r1] or NULL, degree[r1] or NULL,
   counts[3].  Synchronises.                                                                                            */
int kpop_dbscan(kpop_refset *rs, double eps, uint32_t min_pts, uint32_t *labels, uint32_t *core_of, uint32_t *degree,
                uint32_t *counts);
/* bytes of d_work for kpop_dev_dbscan (lib/Space.ml:182-205 over the set against itself, see the block above), for the
   set's r1 at the time of the call.  It grows with r1 and holds: the rows' hit counters (the degrees, 4 bytes a row), two
   tile bitmaps (a bit a tile of the triangle's grid each: the tiles with a hit, and those with a hit that has one core
   end) and the border rows' least key and core row (12 bytes a row); 1.8 MiB for 100,000 rows; no copy of rows         */
uint64_t kpop_dev_dbscan_workspace_bytes(const kpop_refset *rs);
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Enqueues only, reads nothing back, allocates nothing.  d_labels[r1],
   d_core_of[r1] or NULL, d_degree[r1] or NULL (the workspace holds the degrees either way), d_counts[3].              */
int kpop_dev_dbscan(kpop_refset *rs, double eps, uint32_t min_pts, void *d_work, uint32_t *d_labels,
                    uint32_t *d_core_of, uint32_t *d_degree, uint32_t *d_counts, void *stream);
/* unprepared convenience (lib/Matrix.ml:191-266 for the distances, m against itself): a temporary set over m, then
   kpop_dbscan                                                                                                          */
int kpop_distance_dbscan(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p,
                         int normalize, double eps, uint32_t min_pts, uint32_t *labels, uint32_t *core_of,
                         uint32_t *degree, uint32_t *counts);

/* ------------------------------------------------- mutual-reachability tree of a resident set (DBSCAN at every radius)
 * kpop_dbscan wants eps up front; this is its partner, as kpop_spanning_forest is kpop_clusters_within's: one forest for a
 * given min_pts, every eps by a cut -- the first stage of HDBSCAN*.  Distance, graph and NaN are the three blocks' above:
 * d(j, i) is the reference chain's distance (lib/Space.ml:182-205 with the adaptors of lib/Matrix.ml:243-250) -- the bits
 * kpop_refset_distance_rowwise writes under kpop_tune("distance_mfma", 0) when the set's own rows are the query --
 * symmetric bit for bit, the pair i == j never examined; no kpop_tune setting is read.
 * CORE DISTANCE, min_pts in 1 .. 129: core_dist[i] = +0 for min_pts = 1 (a row with a NaN in it too: its degree is 1);
 * otherwise the (min_pts - 1)-th element of the multiset { d(i, j) : j != i, d a number } (+inf is a number) in ascending
 * order, -0 taken as +0, a zero written as +0; the quiet NaN 0x7FF8000000000000 when the multiset has fewer elements
 * (min_pts > r1, a row with a NaN in it, a set full of them).  For every eps that is a number: core_dist[i] <= eps iff
 * kpop_dbscan's degree[i] >= min_pts.  min_pts = 0: KPOP_ERR_INVALID; min_pts > 129: KPOP_ERR_UNSUPPORTED.
 * MUTUAL REACHABILITY: mr(i, j) = max(d(i, j), core_dist[i], core_dist[j]), compared as doubles, a zero as +0.  An edge
 * i < j exists iff all three values are numbers and mr <= max_distance (+inf: every edge whose mr is a number, +inf
 * included; negative: none; NaN: KPOP_ERR_INVALID).  Edges are ordered by (mr, i, j) ascending -- a strict total order,
 * so the minimum spanning forest is UNIQUE, defined without reference to an algorithm, the same bits on every run, however
 * often weights tie (every edge out of row i within core_dist[i] weighs at least that).  *n_edges; edge_i[e] < edge_j[e]
 * with edge_dist[e] = mr, listed in that order, room r1 - 1 entries each (none for r1 <= 1); core_dist[r1] (may be
 * NULL); labels[r1] (may be NULL): the smallest row index of each component of the forest.  r1 = 0: KPOP_OK and
 * *n_edges = 0.  With min_pts = 1 the result is kpop_spanning_forest(rs, max_distance)'s, array for array.  A forest
 * capped at T is the prefix of the uncapped one up to the last edge with mr <= T.
 * THE CUT IS DBSCAN*: for any T <= max_distance, after uniting the ends of the edges with edge_dist <= T, a row with
 * core_dist[i] <= T -- a core row of kpop_dbscan(T, min_pts) -- has exactly kpop_dbscan's label, the smallest core row
 * index of its cluster, and every other row is a component of its own: border rows are NOT attached (DBSCAN*, the variant
 * HDBSCAN is built on).  THERE IS NO known_rows, for kpop_dbscan's reason: a new row can lower old rows' core distances.
 * Neither the r1 x r1 matrix nor a neighbour list longer than min_pts - 1 a row is formed.  The set's limits, slot and
 * thread ownership hold as for every call on a set.  Semantics: INTEGRATION.md 6j; timings: profiles/reachability.md.  */
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250, the order of lib/Matrix.ml:641-650 without the row itself.)  Host array
   core_dist[r1].  Synchronises.                                                                                        */
int kpop_core_distances(kpop_refset *rs, uint32_t min_pts, double *core_dist);
/* bytes of d_work for kpop_dev_core_distances (lib/Space.ml:182-205 over the set against itself, see the block above), for
   the set's r1 at the time of the call: the neighbour lists of one SLAB of 16,384 query rows (the last slab: what is left;
   the larger of the two), a row (12 k + 8) bytes a column segment (1 or 2 for a full slab) plus 12 k + 16, k = min_pts - 1
   -- 49 MiB at k = 128 however long the set; 256 for min_pts = 1 and min_pts > r1, which need no list; 0 for a min_pts
   the call refuses                                                                                                     */
uint64_t kpop_dev_core_distances_workspace_bytes(const kpop_refset *rs, uint32_t min_pts);
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Enqueues only, reads nothing back, allocates nothing.  d_core_dist[r1].  */
int kpop_dev_core_distances(kpop_refset *rs, uint32_t min_pts, void *d_work, double *d_core_dist, void *stream);
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Host arrays.  Synchronises.                                           */
int kpop_reachability_tree(kpop_refset *rs, uint32_t min_pts, double max_distance, uint32_t *n_edges, uint32_t *edge_i,
                           uint32_t *edge_j, double *edge_dist, double *core_dist, uint32_t *labels);
/* bytes of d_work for kpop_dev_reachability_tree (lib/Space.ml:182-205 over the set against itself, see the block above),
   for the set's r1 at the time of the call: 8 bytes a row for the core distances, then the larger of
   kpop_dev_core_distances_workspace_bytes and kpop_dev_spanning_forest_workspace_bytes (one after the other in one place) */
uint64_t kpop_dev_reachability_tree_workspace_bytes(const kpop_refset *rs, uint32_t min_pts);
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Enqueues only: the lists' two passes a slab, then ceil(log2 r1) rounds,
   each of which returns at once when the round before added no edge; nothing is read back, nothing allocated.
   d_n_edges[1], d_edge_i / d_edge_j / d_edge_dist[r1 - 1] (the first *d_n_edges written), d_core_dist[r1] or NULL,
   d_labels[r1] or NULL.                                                                                                */
int kpop_dev_reachability_tree(kpop_refset *rs, uint32_t min_pts, double max_distance, void *d_work, uint32_t *d_n_edges,
                               uint32_t *d_edge_i, uint32_t *d_edge_j, double *d_edge_dist, double *d_core_dist,
                               uint32_t *d_labels, void *stream);
/* unprepared convenience (lib/Matrix.ml:191-266 for the distances, m against itself): a temporary set over m, then
   kpop_reachability_tree                                                                                               */
int kpop_distance_reachability_tree(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind,
                                    double p, int normalize, uint32_t min_pts, double max_distance, uint32_t *n_edges,
                                    uint32_t *edge_i, uint32_t *edge_j, double *edge_dist, double *core_dist,
                                    uint32_t *labels);
/* pure host arithmetic, no GPU and no kpop_init: ANY list of edges i < j < r1 cut at T -- the edges with edge_dist <= T
   united (a NaN joins nothing), a row with core_dist[i] <= T given the smallest row index of its component, every other
   row KPOP_NOISE.  counts[0]: the components that hold such a row; counts[1]: those rows; counts[2]: the noise rows.  Over
   a forest of kpop_reachability_tree and T <= its max_distance: on every core row the label of kpop_dbscan(T, min_pts) over
   the reference chain's distances (lib/Space.ml:182-205; lib/Matrix.ml:243-250), counts[0] and counts[1] its counts[0] and
   counts[1]; its border rows are noise here.  KPOP_ERR_INVALID for a NaN T, a null array and an edge that is not
   i < j < r1.                                                                                                          */
int kpop_reachability_cut(uint32_t r1, uint32_t n_edges, const uint32_t *edge_i, const uint32_t *edge_j,
                          const double *edge_dist, const double *core_dist, double T, uint32_t *labels, uint32_t *counts);

/* ------------------------------------------------- silhouette and medoids of a labelled resident set, in one pass
 * The calls above PRODUCE row labels; this one judges a labelling without ground truth (Rousseeuw 1987) and names one real
 * row per class.  class_of[r1]: a class in [0, n_classes), or KPOP_NO_CLASS for a row that is LEFT OUT -- it is in no sum
 * and nothing is computed for it (KPOP_NOISE == KPOP_NO_CLASS: kpop_dbscan's noise rows leave themselves out).  d(j, i) is
 * the reference chain's distance (lib/Space.ml:182-205 with the adaptors of lib/Matrix.ml:243-250) -- the bits
 * kpop_refset_distance_rowwise writes under kpop_tune("distance_mfma", 0) when the set's own rows are the query; the pair
 * i == j is never examined; no kpop_tune setting is read.  With n_c the rows of class c, for a row j of class c:
 *   own_mean[j]     the sum of d(j, i) over the rows i != j of c, divided by n_c - 1; +0 when n_c == 1
 *   other_mean[j], other_class[j]   over the classes c' != c with n_c' > 0, the least (sum of d(j, i) over c') / n_c' and
 *                   that class; ties go to the smaller class number, a NaN mean is never the least; no such class (or
 *                   every such mean a NaN): the quiet NaN 0x7FF8000000000000 and KPOP_NO_CLASS
 *   silhouette[j]   (other_mean - own_mean) / max(own_mean, other_mean) as IEEE arithmetic gives it (a NaN operand, 0/0
 *                   and inf/inf give NaN), a zero written as +0; +0 when n_c == 1 (Rousseeuw's convention)
 * A row left out gets NaN, NaN, KPOP_NO_CLASS, NaN.  A NaN distance is not skipped: it poisons the sums it is in; the way
 * to keep a row with a NaN in it out is to leave it out.  For a class c: class_rows[c] = n_c; medoid[c] the member least
 * under (own_mean with -0 taken as +0, row index) among the members whose own_mean is a number, medoid_mean[c] that row's
 * own_mean, bits kept; an empty class, or one with no such member: KPOP_NO_CLASS and NaN.
 * THE SUMS are f64 sums in an order that is a fixed function of r1, n_dims and the members' row indices: no floating-point
 * atomic, nothing that depends on timing.  (a) The same bits on every run.  (b) The bits of own_mean, other_mean,
 * silhouette and medoid_mean do not change when the classes are renumbered; other_class and medoid move with the
 * renumbering.  (c) A sum has at most r1 non-negative terms: it lies within r1 2^-53 relative of the exact sum, and is
 * exact wherever all terms and partial sums are representable.
 * ERRORS: n_classes == 0: KPOP_ERR_INVALID; n_classes > 65,535: KPOP_ERR_UNSUPPORTED (kpop_knn_vote's limit); r1 = 0:
 * KPOP_OK.  Every output pointer may be NULL.  THERE IS NO known_rows: a new row changes every mean; after
 * kpop_refset_append the call is made again in full.  THE COST is the full rectangle, r1^2 pairs, twice
 * kpop_clusters_within's triangle: the symmetric half is not exploited (column-side sums that stay deterministic would need
 * a table of partial sums per tile).  Neither the r1 x r1 matrix nor an r1 x n_classes table is formed.  The set's limits,
 * slot and thread ownership hold as for every call on a set.  MEASURED (profiles/silhouette.md; 100,000 rows in 1,000
 * classes, beside kpop_dev_clusters_within at 0.3 in the same process): 156 ms against 49.7 at 64 dimensions, a ratio of
 * 3.14; 3.80 s against 1.07 at 1,635 dimensions, 3.55 -- by pair count 2; a column tile holds one class, and classes of
 * 38 to 204 rows fill 86.5 % of their tiles.  Semantics: INTEGRATION.md 6k. */
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Host arrays: class_of[r1]; own_mean, other_mean, other_class,
   silhouette [r1]; class_rows, medoid, medoid_mean [n_classes].  A class_of[i] >= n_classes that is not KPOP_NO_CLASS is
   KPOP_ERR_INVALID.  Synchronises.                                                                                     */
int kpop_silhouette(kpop_refset *rs, const uint32_t *class_of, uint32_t n_classes, double *own_mean, double *other_mean,
                    uint32_t *other_class, double *silhouette, uint32_t *class_rows, uint32_t *medoid,
                    double *medoid_mean);
/* bytes of d_work for kpop_dev_silhouette (lib/Space.ml:182-205 over the set against itself, see the block above), for the
   set's r1 at the time of the call: the rows grouped by class (the sort's keys and indices, its scratch), a row's own
   mean and 12 bytes for each of up to 16 column segments, the column tiles (16 bytes each, at most r1 / w + n_classes + 1
   of them) and 32 bytes a class -- O(r1 + n_classes), 10.6 MB for 100,000 rows in 1,000 classes; no copy of rows; 0 for
   an n_classes the call refuses                                                                                        */
uint64_t kpop_dev_silhouette_workspace_bytes(const kpop_refset *rs, uint32_t n_classes);
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Enqueues only, reads nothing back, allocates nothing.  d_class_of[r1] is
   TRUSTED and guarded: an entry >= n_classes counts as left out.  The outputs as above, on the device, each or NULL.    */
int kpop_dev_silhouette(kpop_refset *rs, const uint32_t *d_class_of, uint32_t n_classes, void *d_work, double *d_own_mean,
                        double *d_other_mean, uint32_t *d_other_class, double *d_silhouette, uint32_t *d_class_rows,
                        uint32_t *d_medoid, double *d_medoid_mean, void *stream);
/* unprepared convenience (lib/Matrix.ml:191-266 over lib/Space.ml:182-205 for the distances, m against itself): a
   temporary set over m, then kpop_silhouette                                                                           */
int kpop_distance_silhouette(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p,
                             int normalize, const uint32_t *class_of, uint32_t n_classes, double *own_mean,
                             double *other_mean, uint32_t *other_class, double *silhouette, uint32_t *class_rows,
                             uint32_t *medoid, double *medoid_mean);
/* pure host arithmetic, no GPU and no kpop_init: the mean silhouette (of kpop_silhouette over the reference chain's
   distances, lib/Space.ml:182-205, or any other) of each class, class_mean[n_classes], and of all the rows that are not
   left out, *overall_mean; both summed in ascending row order, which is the contract; an empty class, and no row at all,
   give NaN.  KPOP_ERR_INVALID for a null pointer, n_classes == 0 and a class_of[i] >= n_classes that is not
   KPOP_NO_CLASS; n_classes > 65,535: KPOP_ERR_UNSUPPORTED.                                                              */
int kpop_silhouette_summary(uint32_t r1, const uint32_t *class_of, uint32_t n_classes, const double *silhouette,
                            double *class_mean, double *overall_mean);

/* ------------------------------------------------- class linkage: the distances between every two classes, and their tree
 * The labelled-set calls above answer questions about rows; this one answers them about the CLASSES: which two touch and
 * through which two rows, how wide a class is, how far apart two classes are on average, and what tree they form (the
 * reference's README section 5.3, "Pseudo-phylogenetic trees", is empty).  class_of[r1]: a class in [0, n_classes), or
 * KPOP_NO_CLASS for a row that is LEFT OUT of everything.  d(i, j) is kpop_silhouette's distance: the reference chain's
 * (lib/Space.ml:182-205 with the adaptors of lib/Matrix.ml:243-250), the bits kpop_refset_distance_rowwise writes on the
 * vector pipe with the set's rows as the query, symmetric bit for bit; the pair i == j is never examined; no kpop_tune
 * setting is read.  P(a, b), a != b: the pairs of one row of a and one row of b; P(a, a): the pairs i < j of two rows of a.
 *   class_rows[a]     the rows of class a
 *   mean_dist[a][b]   the sum of d over P(a, b) divided by |P(a, b)|; P empty (an empty class, the diagonal of a class of
 *                     one row): the quiet NaN 0x7FF8000000000000; one NaN distance in P makes the mean a NaN
 *   min_dist, max_dist  the least and the greatest d over the pairs of P whose distance is a number, -0 as +0; no such
 *                     pair: the declared NaN
 *   min_i < min_j     the two rows of the least pair under the strict order (d with -0 as +0, i, j), i < j the natural row
 *                     indices (which of them lies in which class is class_of's to say); min_dist NaN: both KPOP_NO_CLASS
 * The five tables are [n_classes x n_classes], row-major, and SYMMETRIC bit for bit: every unordered class pair is computed
 * once and written to both halves.  max_dist[a][a] is the class's diameter, min_dist[a][a] and its pair the class's closest
 * two rows.  THE SAME BITS ON EVERY RUN: no floating-point atomic, nothing that depends on timing; a sum is taken in an
 * order that is a function of r1 and of the labelling alone (class_linkage.hip's header writes it down).  min_dist,
 * max_dist, min_i and min_j do not depend on any order: under a renumbering of the classes the tables are permuted and
 * nothing else changes.  mean_dist under a renumbering stays within (N + 2) 2^-53 relative of the exact mean, N = n_a n_b
 * (n_a^2 on the diagonal), but is NOT promised bit for bit: the class that supplies a strip's rows may change.
 * ERRORS: n_classes == 0: KPOP_ERR_INVALID; n_classes > 4,096: KPOP_ERR_UNSUPPORTED (the tables are n_classes^2 entries:
 * 134 MB each at 4,096); the workspace-bytes call returns 0 for both.  r1 = 0: KPOP_OK, every class_rows 0, every table
 * entry its NaN / KPOP_NO_CLASS.  No known_rows: after kpop_refset_append the call is made again in full.  Neither the
 * r1 x r1 matrix nor an r1 x n_classes table is formed.  MEASURED: profiles/class_linkage.md.                          */

/* the set on the handle.  Host arrays, each may be NULL: class_rows [n_classes]; the others [n_classes^2].  A class_of[i]
   >= n_classes that is not KPOP_NO_CLASS is KPOP_ERR_INVALID.  Synchronises.                                            */
int kpop_class_linkage(kpop_refset *rs, const uint32_t *class_of, uint32_t n_classes, uint32_t *class_rows,
                       double *mean_dist, double *min_dist, double *max_dist, uint32_t *min_i, uint32_t *min_j);
/* bytes of d_work for kpop_dev_class_linkage (lib/Space.ml:182-205 over the set against itself, see the block above), for
   the set's r1 at the time of the call: the grouping and (r1 / TJ + 1 + n_classes) n_classes partials of 32 bytes, TJ the
   tile shape's strip (64 rows, 256 from 65,536 rows on); 0 for an n_classes the call refuses                           */
uint64_t kpop_dev_class_linkage_workspace_bytes(const kpop_refset *rs, uint32_t n_classes);
/* enqueues only on `stream`: reads nothing back, allocates nothing.  d_class_of is TRUSTED and guarded: an entry that is
   no class counts as left out.  Every output pointer may be NULL (lib/Space.ml:182-205, see the block above)            */
int kpop_dev_class_linkage(kpop_refset *rs, const uint32_t *d_class_of, uint32_t n_classes, void *d_work,
                           uint32_t *d_class_rows, double *d_mean_dist, double *d_min_dist, double *d_max_dist,
                           uint32_t *d_min_i, uint32_t *d_min_j, void *stream);
/* without keeping a set (Matrix.get_distance_rowwise's operands, lib/Matrix.ml:191-266, m against itself): a temporary set
   over m, then kpop_class_linkage                                                                                        */
int kpop_distance_class_linkage(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p,
                                int normalize, const uint32_t *class_of, uint32_t n_classes, uint32_t *class_rows,
                                double *mean_dist, double *min_dist, double *max_dist, uint32_t *min_i, uint32_t *min_j);

#define KPOP_LINK_SINGLE 0   /* pass min_dist */
#define KPOP_LINK_COMPLETE 1 /* pass max_dist */
#define KPOP_LINK_AVERAGE 2  /* pass mean_dist: UPGMA, weighted by class_rows */
/* pure host arithmetic, no GPU and no kpop_init: the agglomeration of the classes under dist[n_classes^2] (a table of
   kpop_class_linkage over the reference chain's distances, lib/Space.ml:182-205, or any other), of which only the entries
   dist[a][b], a < b, of classes with rows are read.  The leaves are the classes with class_rows > 0, their node ids their
   class numbers; merge t makes node n_classes + t.  Each step merges the two live nodes least under (distance with -0 as
   +0, lower id, higher id): left[t] < right[t] their ids, height[t] that distance (-0 as +0), size[t] the rows under the
   new node.  The new node's distance to a third node z: single min(d_xz, d_yz), complete max, average
   (n_x d_xz + n_y d_yz) / (n_x + n_y) in exactly that order in f64, x the left node; a NaN operand gives a NaN.  A NaN is
   never the least: when no two live nodes have a number between them the call stops with *n_merges below leaves - 1, and
   the result is a forest.  All three linkages are reducible: the heights never decrease.  left, right, height, size:
   n_classes - 1 entries each.  KPOP_ERR_INVALID: a null pointer, n_classes == 0, another linkage; n_classes > 4,096:
   KPOP_ERR_UNSUPPORTED.                                                                                                  */
int kpop_class_tree(uint32_t n_classes, const uint32_t *class_rows, const double *dist, int linkage, uint32_t *n_merges,
                    uint32_t *left, uint32_t *right, double *height, uint32_t *size);

/* ------------------------------------------------- farthest-first traversal of a resident set (k diverse rows, every k)
 * kpop_representatives_within thins a set at a radius that is known; this is its partner when a COUNT is known, or
 * nothing: one ordering of the rows (Gonzalez 1985) whose every prefix is a cover of the set, its radius written beside
 * it.  d(j, i) is the reference chain's distance (lib/Space.ml:182-205 with the adaptors of lib/Matrix.ml:243-250) -- the
 * bits kpop_refset_distance_rowwise writes under kpop_tune("distance_mfma", 0) when the set's own rows are the query --
 * whatever kpop_tune says; symmetric bit for bit, the pair i == j never examined.
 * STATE: every row has a COVER DISTANCE, +inf at first, and a COVER ROW, KPOP_NOISE at first.  Picking row c marks it
 * picked; for every unpicked row x, d(x, c) replaces the cover distance iff it is a number and strictly less than it (-0
 * taken as +0), and the cover row becomes c.  A NaN distance covers nothing; a tie keeps the earlier pick.
 * ORDER: pick t < n_seeds is seeds[t].  Every later pick is the unpicked row greatest under (cover distance descending,
 * row index ascending): with no seeds the first pick is row 0.  Before a pick that is not a seed the traversal stops if
 * that row's cover distance is <= cover_radius (negative: never; +inf without seeds: at once; NaN: KPOP_ERR_INVALID); it
 * also stops at max_picks picks (above r1: r1).  A row with a NaN in it keeps +inf and is picked as soon as its index
 * comes up among the +inf rows.
 * RESULT: *n_picks; for pick t, pick[t] the row, pick_radius[t] its cover distance at the moment it was picked (+inf for
 * the first pick, a zero written as +0) and pick_parent[t] its cover row at that moment or KPOP_NOISE; for row i,
 * rep_of[i] = i and rep_dist[i] = +0 when it was picked, otherwise its cover row (KPOP_NOISE: none) and its cover
 * distance (+inf: none).  *n_passes: how often the call walked the whole set -- a fact about the run, not part of the
 * contract.  Every output pointer but n_picks may be NULL.  r1 = 0 or max_picks = 0: KPOP_OK and *n_picks = 0.
 * PROPERTIES: past the seeds and pick 0, pick_radius never increases; with cover_radius < 0 and the same seeds the result
 * at max_picks = k is the first k entries of the result at any larger max_picks, bit for bit; with seeds = pick[0 .. k)
 * of an earlier run the run reproduces pick, pick_radius and pick_parent from 0 on -- after kpop_refset_append the old
 * picks go in as seeds and the traversal goes on over the grown set; a run stopped at cover_radius = R >= 0 leaves every
 * row with rep_dist <= R (or +inf: a NaN) and every pick past the seeds with pick_radius > R, so that the picks lie
 * pairwise farther apart than R, a maximal independent set of kpop_clusters_within's graph at R; the first k picks are a
 * 2-approximation of the best k centres; rep_dist[i] is the least d(i, pick[t]) and rep_of[i] the pick at the first such
 * t.  A strict total order and no floating-point sum across rows: the same bits on every run.
 * ERRORS: a seed >= r1, a repeated seed, n_seeds > max_picks: KPOP_ERR_INVALID (the device form trusts the seeds'
 * values and holds them inside the set).  The set's limits, slot and thread ownership hold as for every call on a set.
 * Semantics: INTEGRATION.md 6l; timings: profiles/farthest_first.md. */
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Host arrays: seeds[n_seeds]; pick, pick_radius, pick_parent with room
   for min(max_picks, r1) entries, the first *n_picks written; rep_of[r1], rep_dist[r1].  Synchronises.                  */
int kpop_farthest_first(kpop_refset *rs, uint32_t max_picks, double cover_radius, const uint32_t *seeds,
                        uint32_t n_seeds, uint32_t *n_picks, uint32_t *pick, double *pick_radius, uint32_t *pick_parent,
                        uint32_t *rep_of, double *rep_dist, uint32_t *n_passes);
/* bytes of d_work for kpop_dev_farthest_first (lib/Space.ml:182-205 over the set against itself, see the block above),
   for the set's r1 at the time of the call: 12 bytes a row for the cover distances and rows, 16 bytes a pick, 24 KiB of
   buckets -- O(r1 + max_picks); no copy of rows                                                                        */
uint64_t kpop_dev_farthest_first_workspace_bytes(const kpop_refset *rs, uint32_t max_picks);
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Enqueues only, reads nothing back, allocates nothing: the seeds' groups,
   then min(max_picks, r1) - n_seeds + 1 passes, each of which returns at once after the traversal has stopped.
   d_seeds[n_seeds] TRUSTED to be distinct; d_pick, d_pick_radius, d_pick_parent [min(max_picks, r1)] each or NULL,
   d_rep_of[r1] or NULL, d_rep_dist[r1] or NULL, d_counts[2] = {n_picks, n_passes}.                                      */
int kpop_dev_farthest_first(kpop_refset *rs, uint32_t max_picks, double cover_radius, const uint32_t *d_seeds,
                            uint32_t n_seeds, void *d_work, uint32_t *d_pick, double *d_pick_radius,
                            uint32_t *d_pick_parent, uint32_t *d_rep_of, double *d_rep_dist, uint32_t *d_counts,
                            void *stream);
/* unprepared convenience (lib/Matrix.ml:191-266 for the distances, m against itself): a temporary set over m, then
   kpop_farthest_first                                                                                                  */
int kpop_distance_farthest_first(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind,
                                 double p, int normalize, uint32_t max_picks, double cover_radius, const uint32_t *seeds,
                                 uint32_t n_seeds, uint32_t *n_picks, uint32_t *pick, double *pick_radius,
                                 uint32_t *pick_parent, uint32_t *rep_of, double *rep_dist, uint32_t *n_passes);

/* ------------------------------------------------- k-medoids on a resident set (kmedoids.hip)
 * Clusters when a COUNT is known and no radius is: n_medoids groups, each around the real row that stands for it, every
 * other row filed under its nearest centre.  Alternating k-medoids (Voronoi iteration; Park & Jun 2009) on the set's r1
 * rows; d(j, i) is the distance of kpop_farthest_first and kpop_silhouette: the reference chain's bits, symmetric bit for
 * bit, the pair i == j never examined, no kpop_tune key read; all three kinds, normalised or not.
 * ASSIGNMENT of a labelling to a medoid list M[0 .. k): row M[c] has class c and dist +0 (a medoid always belongs to its
 * own position, also when it is a duplicate of an earlier medoid: no class is ever empty); every other row j gets the
 * class least under (d(j, M[c]) with -0 taken as +0, c ascending) over the c whose distance is a number, and dist[j] is
 * that distance; a row with no such c is LEFT OUT: class_of = KPOP_NO_CLASS, dist = +inf, own_mean = NaN, in no sum.
 * own_mean[j] is kpop_silhouette's for that labelling -- the sum of d(j, i) over the other rows of j's class divided by
 * n_c - 1, +0 when n_c == 1 -- WITH THE BITS kpop_silhouette writes for the same class_of.
 * UPDATE: M'[c] is the member of class c least under (own_mean with -0 as +0, row index) among the members whose own_mean
 * is a number (kpop_silhouette's medoid); a class with no such member keeps M[c].
 * THE LOOP:   L = assign(M = init); cost[0]; n_iter = 0
 *             for t = 0, 1, ...:  own_mean = within-class means of L;  M' = update
 *                                 if M' == M:       converged = 1, stop
 *                                 if t == max_iter: converged = 0, stop
 *                                 M = M';  L = assign(M);  n_iter += 1;  cost[n_iter]
 * RESULT, always consistent: class_of / dist are the assignment to medoid[], own_mean and class_rows are of that
 * labelling.  max_iter = 0 is the plain assignment to given rows (the nearest of ALL the representatives a caller
 * holds), converged saying whether they are a fixed point already.  cost[t] is the sum of dist over the rows not left
 * out, summed in an order that is a fixed function of r1, without a floating-point atomic: within r1 2^-53 relative of
 * the exact sum, exact where every partial sum is representable; the entries of cost[max_iter + 1] past n_iter are the
 * quiet NaN.
 * PROPERTIES: the same bits on every run; a run of a rounds followed by a run of b rounds from its medoid[] gives the
 * medoid, class_of, dist, own_mean, class_rows and converged of one run of a + b rounds, bit for bit, its cost the first
 * run's followed by the second's from index 1 -- after kpop_refset_append the old medoids go in as init; in exact
 * arithmetic cost never increases; kpop_silhouette(class_of, n_medoids) gives own_mean bit for bit, and its medoid is
 * medoid[] when converged, the next round's medoid[] otherwise; permuting init permutes medoid / class_rows and relabels
 * class_of, dist keeps its bits (own_mean too wherever no row is equidistant from two medoids).
 * ERRORS: n_medoids == 0, n_medoids > r1, a null init, and in the host forms an init[c] >= r1 or a repeated init row:
 * KPOP_ERR_INVALID (the device form trusts distinctness and holds every index inside the set); n_medoids > 65,535:
 * KPOP_ERR_UNSUPPORTED (the 16-bit class key).  Every output pointer may be NULL except n_iter and converged (d_counts).
 * Semantics: INTEGRATION.md 6m; timings: profiles/kmedoids.md. */
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Host arrays: init[n_medoids]; medoid, class_rows [n_medoids];
   class_of, dist, own_mean [r1]; cost[max_iter + 1].  Reads the done word back after every round and stops enqueuing
   once the loop has stopped.  Synchronises.                                                                            */
int kpop_kmedoids(kpop_refset *rs, uint32_t n_medoids, const uint32_t *init, uint32_t max_iter, uint32_t *medoid,
                  uint32_t *class_of, double *dist, double *own_mean, uint32_t *class_rows, double *cost,
                  uint32_t *n_iter, int *converged);
/* bytes of d_work for kpop_dev_kmedoids (lib/Space.ml:182-205 over the set against itself, see the block above), for the
   set's r1 at the time of the call: O(r1 + n_medoids + max_iter), no copy of a row; 0 for arguments the call refuses    */
uint64_t kpop_dev_kmedoids_workspace_bytes(const kpop_refset *rs, uint32_t n_medoids, uint32_t max_iter);
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Enqueues only, reads nothing back, allocates nothing: the worst case
   of max_iter + 1 rounds, whose kernels return at once after the loop has stopped (the scans and the sort of such a
   round run on unchanged data: O(r1) a round, no output altered).  d_init[n_medoids] TRUSTED to be distinct; d_medoid,
   d_class_rows [n_medoids], d_class_of, d_dist, d_own_mean [r1], d_cost[max_iter + 1], each or NULL;
   d_counts[2] = {n_iter, converged}.                                                                                    */
int kpop_dev_kmedoids(kpop_refset *rs, uint32_t n_medoids, const uint32_t *d_init, uint32_t max_iter, void *d_work,
                      uint32_t *d_medoid, uint32_t *d_class_of, double *d_dist, double *d_own_mean,
                      uint32_t *d_class_rows, double *d_cost, uint32_t *d_counts, void *stream);
/* unprepared convenience (lib/Matrix.ml:191-266 for the distances, m against itself): a temporary set over m, then
   kpop_kmedoids                                                                                                        */
int kpop_distance_kmedoids(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p,
                           int normalize, uint32_t n_medoids, const uint32_t *init, uint32_t max_iter, uint32_t *medoid,
                           uint32_t *class_of, double *dist, double *own_mean, uint32_t *class_rows, double *cost,
                           uint32_t *n_iter, int *converged);

/* ------------------------------------------------- local outlier factor of a resident set, and of query rows (lof.hip)
 * Does this row belong to the database at all?  kpop_knn_vote gives every query row a class however far it lies,
 * kpop_dbscan's noise needs one global eps, and a k-th neighbour's distance is not comparable between a tight lineage and
 * a loose one.  The local outlier factor (Breunig, Kriegel, Ng, Sander 2000) is a row's density relative to its
 * neighbours' densities: about 1 inside any lineage, well above 1 for a contaminated sample, a mislabelled assembly or the
 * first genome of a new lineage.  d(j, i) is the distance of every block above: the reference chain's (lib/Space.ml:182-205
 * with the adaptors of lib/Matrix.ml:243-250) -- the bits kpop_refset_distance_rowwise writes under
 * kpop_tune("distance_mfma", 0) -- symmetric bit for bit; no kpop_tune setting is read; a NaN distance is within nothing.
 * k in 1 .. 128: k = 0 KPOP_ERR_INVALID, k > 128 KPOP_ERR_UNSUPPORTED.
 * THE SET FORM scores every row j of the set against the OTHER rows; the pair i == j is never examined.
 *   kdist[j]   = kpop_core_distances(rs, k + 1)[j], bit for bit: the k-th least of the numbers among d(j, i), i != j; a
 *                zero is written as +0; the quiet NaN 0x7FF8000000000000 when there are fewer than k numbers.
 *   N(j)       = { i != j : d(j, i) <= kdist[j] }: the WHOLE tie group of the k-th distance, as the paper defines it, so
 *                the result does not depend on the row order.
 *   n_neigh[j] = |N(j)|: at least k; 0 when kdist[j] is a NaN.
 *   lrd[j]     = n_neigh[j] / S1(j), S1(j) the sum over N(j) of max(d(j, i), kdist[i]) -- the max compared as doubles, a
 *                zero taken as +0.  IEEE division: +inf when S1 = 0 (a row with at least k exact copies), 0 when S1 = +inf.
 *   lof[j]     = (S2(j) / n_neigh[j]) / lrd[j], S2(j) the sum over N(j) of lrd[i].  IEEE arithmetic with ONE declared
 *                exception: inf / inf is 1.0 -- a row inside a clump of copies is as dense as its neighbours.  So a finite
 *                lrd beside a clump gives +inf, and 0 / 0 gives a NaN.
 *   A row with n_neigh = 0 gets the quiet NaN for lrd and lof.  A NaN term poisons the sum it is in; every NaN written is
 *   the quiet NaN above, every zero +0.  Where a set holds more than k copies of a row, kpop_representatives_within(0)
 *   first (INTEGRATION.md 6n says why).
 * THE QUERY FORM (novelty) scores row q of m2 against the set AS IT STANDS; the set's rows are not re-scored.  set_kdist,
 * set_lrd [r1]: the set form's kdist and lrd at the same k.  kdist_q = the k-th least of the numbers among d(q, i) over ALL
 * i -- nothing is left out: a query equal to a set row has that row at distance 0; N(q) = { i : d(q, i) <= kdist_q };
 * lrd_q = |N| / (the sum over N of max(d(q, i), set_kdist[i])); lof_q = (the sum over N of set_lrd[i] / |N|) / lrd_q; the
 * conventions of the set form.  r1 < k: every row the NaN row (NaN, 0, NaN, NaN).  r2 = 0: KPOP_OK.
 * THE SUMS S1 and S2 are f64 sums in an order that is a fixed function of r1 (and r2), n_dims and k: within a thread the
 * columns ascend and a non-member adds +0, a row's lanes meet in a fixed tree, the column segments are added in segment
 * order.  No floating-point atomic: the same bits on every run.  Against an exact sum of n = n_neigh non-negative terms,
 * S is within n 2^-53 relative.
 * LIMITS: there is NO known_rows -- a new row can lower old rows' k-distances; after kpop_refset_append the set form is
 * called again in full.  Neither the matrix nor a neighbour list longer than k a row is formed; apart from the k-NN lists
 * of kpop_dev_core_distances the workspace is O(r1), or O(slab x segments) for a slab of 16,384 query rows.  Every output
 * pointer may be NULL.  The cost is three full rectangles of pairs: the lists, S1 and S2 (a NULL lof saves the third).
 * MEASURED (100,000 rows, k = 20, one MI355X): 348.7 ms at 64 dimensions and 7,997 ms at 1,635 -- 0.856 and 0.863 of
 * kpop_dev_core_distances(21) plus two kpop_dev_silhouette calls with one class, timed in the same process; 4,096 query
 * rows against the 64-dimensional set 19.3 ms.  Semantics: INTEGRATION.md 6n; registers and timings: profiles/lof.md.  */
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Host arrays [r1], each may be NULL.  r1 = 0: KPOP_OK.  Synchronises.   */
int kpop_lof(kpop_refset *rs, uint32_t k, double *kdist, uint32_t *n_neigh, double *lrd, double *lof);
/* bytes of d_work for kpop_dev_lof (lib/Space.ml:182-205 over the set against itself, see the block above), for the set's
   r1 at the time of the call: 16 bytes a row for kdist and lrd, 12 bytes a row and column segment (16 of them at most)
   for what a sweep leaves, then kpop_dev_core_distances_workspace_bytes(rs, k + 1); 0 for a k the call refuses          */
uint64_t kpop_dev_lof_workspace_bytes(const kpop_refset *rs, uint32_t k);
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Enqueues only, reads nothing back, allocates nothing.  d_kdist, d_lrd,
   d_lof (f64 [r1]), d_n_neigh (u32 [r1]), each or NULL: kdist and lrd, which the body needs itself, then live in d_work. */
int kpop_dev_lof(kpop_refset *rs, uint32_t k, void *d_work, double *d_kdist, uint32_t *d_n_neigh, double *d_lrd,
                 double *d_lof, void *stream);
/* unprepared convenience (lib/Matrix.ml:191-266 for the distances, m against itself): a temporary set over m, then
   kpop_lof                                                                                                             */
int kpop_distance_lof(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p,
                      int normalize, uint32_t k, double *kdist, uint32_t *n_neigh, double *lrd, double *lof);
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  The query form on host arrays: set_kdist, set_lrd [r1] (needed when
   r1 >= k), m2 [r2][n_dims]; kdist, lrd, lof (f64 [r2]), n_neigh (u32 [r2]), each may be NULL.  Synchronises.           */
int kpop_lof_score(kpop_refset *rs, uint32_t k, const double *set_kdist, const double *set_lrd, const double *m2,
                   uint32_t r2, double *kdist, uint32_t *n_neigh, double *lrd, double *lof);
/* bytes of d_work for kpop_dev_lof_score (lib/Space.ml:182-205, query rows against the set, see the block above): what
   kpop_dev_lof takes for a slab of min(r2, 16,384) query rows, the lists being kpop_dev_knn_vote's without a class or a
   tie table (with the slab's divided copy when the set normalises); it does not depend on r1.  0 for a k the call refuses */
uint64_t kpop_dev_lof_score_workspace_bytes(const kpop_refset *rs, uint32_t r2, uint32_t k);
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Enqueues only, reads nothing back, allocates nothing: the query rows in
   slabs of 16,384, a slab's lists, then its two sweeps.  d_set_kdist, d_set_lrd [r1]; d_m2 [r2][n_dims]; the outputs as
   in kpop_dev_lof, [r2].                                                                                                */
int kpop_dev_lof_score(kpop_refset *rs, uint32_t k, const double *d_set_kdist, const double *d_set_lrd, const double *d_m2,
                       uint32_t r2, void *d_work, double *d_kdist, uint32_t *d_n_neigh, double *d_lrd, double *d_lof,
                       void *stream);

/* ------------------------------------------------- density peaks of a resident set: nearest denser row, tree and cut
 * (density_peaks.hip)  Clusters when neither a radius nor a count is known and the lineages differ in tightness
 * (Rodriguez & Laio, Science 2014), and "the nearest row that ranks above me" for any score the caller holds: with
 * assembly quality as the score, delta > radius marks the rows with no better genome within the radius.  d(j, i) is the
 * distance of every block above: the reference chain's (lib/Space.ml:182-205 with the adaptors of lib/Matrix.ml:243-250)
 * -- the bits kpop_refset_distance_rowwise writes under kpop_tune("distance_mfma", 0) -- symmetric bit for bit; no
 * kpop_tune setting is read; the pair i == j is never examined; a NaN distance is no candidate; a zero is written as +0.
 * DENSITY: density[r1] (f64) is the caller's, or NULL: density[i] = (double) degree[i], kpop_dbscan's at eps (1 + the
 *   other rows within eps); eps is then required and a NaN eps is KPOP_ERR_INVALID.  With a density given eps is not read.
 *   A row whose density is a NaN is LEFT OUT: it is nobody's candidate, its delta is the quiet NaN 0x7FF8000000000000,
 *   its parent and its label are KPOP_NOISE.  -0 equals +0; +inf and -inf are numbers.
 * RANK: row i ranks above row j iff density[i] > density[j], or the densities are equal and i < j: a strict total order
 *   of the rows that are not left out.
 * PARENT, DELTA: among the rows i that rank above j and whose d(j, i) is a number, parent[j] is the least under
 *   (d with -0 as +0, i) -- ties of distance go to the smaller row index -- and delta[j] that distance.  None:
 *   parent[j] = j, delta[j] = +inf, a ROOT (the top of the order, a row with a NaN in it, r1 = 1).  A parent ranks above
 *   its child, so the parents form a forest; as the minimum of a strict order it is a function of the distances and the
 *   densities alone: the same bits on every run.
 * CUT: row j is a CENTRE iff it is a root, or delta[j] > min_delta && density[j] >= min_density.  labels[j] = j for a
 *   centre, otherwise labels[parent[j]]: the centre's row index, labels[labels[j]] == labels[j].  counts[0]: the
 *   centres, counts[1]: the roots, counts[2]: the rows left out.  A NaN threshold is KPOP_ERR_INVALID;
 *   min_density = -inf is no density bar; min_delta = +inf makes only the roots centres.
 * r1 = 0: KPOP_OK, the counts zero.  eps < 0: every degree is 1, every row ties, the rank is the row order.  There is NO
 * known_rows: a new row changes degrees; after kpop_refset_append the call is made again in full.  Neither the matrix
 * nor a neighbour list is formed; the workspace is O(r1).  The cost is the degree pass (a triangle, when no density is
 * given), a 64-bit radix sort of r1 keys, and ONE triangle of pairs in rank order: the row at position q of the rank
 * order meets only the positions below q.
 * MEASURED (100,000 rows, one MI355X): with a given density 54.5 ms at 64 dimensions and 1,315 ms at 1,635 -- 0.41 and 0.39
 * of kpop_dev_silhouette with one class, timed in the same process (0.5 by pair count); with the degree density 102.8 and
 * 2,377 ms, the difference one kpop_dev_clusters_within.  Semantics: INTEGRATION.md 6p; registers and timings:
 * profiles/density_peaks.md.                                                                                            */
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Host arrays: density [r1] or NULL; density_out, delta (f64 [r1]),
   parent, labels (u32 [r1]), counts (u32 [3]), each may be NULL.  Synchronises.                                         */
int kpop_density_peaks(kpop_refset *rs, double eps, const double *density, double min_density, double min_delta,
                       double *density_out, double *delta, uint32_t *parent, uint32_t *labels, uint32_t *counts);
/* bytes of d_work for kpop_dev_density_peaks (lib/Space.ml:182-205 over the set against itself, see the block above),
   for the set's r1 at the time of the call: O(r1) -- 12 bytes a row and column segment (16 of them), the sort's buffers,
   two label buffers, and kpop_dev_dbscan_workspace_bytes for the degrees                                               */
uint64_t kpop_dev_density_peaks_workspace_bytes(const kpop_refset *rs);
/* (lib/Space.ml:182-205; lib/Matrix.ml:243-250.)  Enqueues only, reads nothing back, allocates nothing.  d_density
   (f64 [r1]) or NULL; d_density_out, d_delta (f64 [r1]), d_parent, d_labels (u32 [r1]), d_counts (u32 [3]), each or
   NULL: what the body needs itself then lives in d_work.  NULL d_labels and d_counts: no cut is made.                   */
int kpop_dev_density_peaks(kpop_refset *rs, double eps, const double *d_density, double min_density, double min_delta,
                           void *d_work, double *d_density_out, double *d_delta, uint32_t *d_parent, uint32_t *d_labels,
                           uint32_t *d_counts, void *stream);
/* unprepared convenience (lib/Matrix.ml:191-266 for the distances, m against itself): a temporary set over m, then
   kpop_density_peaks                                                                                                   */
int kpop_distance_density_peaks(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p,
                                int normalize, double eps, const double *density, double min_density, double min_delta,
                                double *density_out, double *delta, uint32_t *parent, uint32_t *labels, uint32_t *counts);
/* The CUT alone, of the arrays a call above returned, at other thresholds: host arithmetic, no GPU and no kpop_init, so
   the thresholds can be chosen after a look at the decision graph (density, delta).  (No counterpart in the reference:
   the distances behind delta are lib/Space.ml:182-205's.)  KPOP_ERR_INVALID for a NaN threshold and for a parent that is
   neither KPOP_NOISE, the row itself, nor a row of the set ranking strictly above it -- the check that rules a cycle
   out; nothing is written then.  labels (u32 [r1]) and counts (u32 [3]) may each be NULL.                               */
int kpop_density_peaks_cut(uint32_t r1, const double *density, const double *delta, const uint32_t *parent,
                           double min_density, double min_delta, uint32_t *labels, uint32_t *counts);

/* ------------------------------------------------- k-mer database (KPopCountDB)
 * the operations of lib/KMerDB.ml that touch every count.  A database is the reference's
 * `storage: I32BAVector.t array` (lib/KMerDB.ml:54-63): n_cols spectra ("columns"), each a vector of n_rows int32
 * counts -- passed as one pointer per spectrum, exactly the shape an OCaml binding has in hand (Bigarray data
 * lives outside the OCaml heap and does not move).  Statistics are {non_zero, max, sum, sum_log} per vector
 * (Transformation.statistics_t, :73-79; `min` is always 0 there and unused).                                   */
#define KPOP_TRANSF_BINARY 0 /* lib/KMerDB.ml:88-92 (Transformation.t) */
#define KPOP_TRANSF_POWER 1
#define KPOP_TRANSF_CLR 2
#define KPOP_TRANSF_PSEUDO 3
#define KPOP_COMBINE_MEAN 0 /* lib/KMerDB.ml:616-626 (CombinationCriterion.t) */
#define KPOP_COMBINE_MEDIAN 1

/* Replaces stats_table_of_core_db, lib/KMerDB.ml:171-271: col_stats is n_cols x 4, row_stats n_rows x 4 (either
 * may be NULL).  A threshold below 1 is relative to the vector's own sum of count^power (:190-195).             */
int kpop_counter_stats(const int32_t *const *columns, uint32_t n_cols, uint64_t n_rows, double threshold,
                       double power, double *col_stats, double *row_stats);

/* Replaces the worker + consumer of add_combined_selected, lib/KMerDB.ml:661-722: combines the spectra
 * columns[sel[0..n_sel)] (visited in that order; the reference's order is its `found_cols`, :646-660) into
 * out[n_rows] = Int32.of_float(sum or median * n_sel of count * max_norm / norm) (:693-716).  col_sum[c] is the
 * linear statistic `sum` of column c (kpop_counter_stats with threshold 1, power 1).  *out_norm (may be NULL)
 * receives the accumulated norm the reference prints in verbose mode (:715,725).                                */
int kpop_counter_combine(const int32_t *const *columns, uint64_t n_rows, const uint32_t *sel, uint32_t n_sel,
                         const double *col_sum, int criterion, int32_t *out, double *out_norm);

/* Replaces the Transformation.compute loops of to_table / to_spectra, lib/KMerDB.ml:96-144,1040-1050,1140-1160,
 * 1203-1212: out[r*n_cols + c] (kmer_major = 1, the default table) or out[c*n_rows + r] (kmer_major = 0:
 * transposed table and spectra).  col_stats is n_cols x 4 from kpop_counter_stats with the same threshold/power. */
int kpop_counter_transform(const int32_t *const *columns, uint32_t n_cols, uint64_t n_rows, int which,
                           double threshold, double power, const double *col_stats, int kmer_major, double *out);

/* Replaces distill_kmers, lib/KMerDB.ml:812-976 (KPopCountDB -d): ranks the k-mers by how well they separate the
 * classes of the spectra.  classes[c] in [0, n_classes) is the class of column c.  For every k-mer, the absolute
 * differences of the normalised counts (count / linear column sum) of all pairs of spectra are binned by pair of
 * classes; mean, sample variance and coefficient of variation per bin; mean and median of each over the diagonal
 * ("Inner") and the off-diagonal ("Outer") bins; a straight line Outer ~ Inner over all k-mers per (quantity, mean |
 * median) and its residuals.  out is [KPOP_DISTILL_ROWS][n_rows] in the reference's row order (:960-965:
 * Inner/Outer/Residual x AvgMean, AvgMedian, VarMean, VarMedian, COVMean, COVMedian); fits (may be NULL) receives
 * {intercept, slope} of the six lines in that order.  The semantics are spelled out in INTEGRATION.md ("distill").
 * The same bits on every run.  KPOP_ERR_INVALID: a class index >= n_classes, an empty class, n_classes == 1 or
 * == n_cols ("Invalid_number_of_classes", :822-823).                                                             */
#define KPOP_DISTILL_ROWS 18
int kpop_counter_distill(const int32_t *const *columns, uint32_t n_cols, uint64_t n_rows, const uint32_t *classes,
                         uint32_t n_classes, double *out, double *fits);

/* device-resident forms: storage is [n_cols][ld] int32 with ld = kpop_dev_counter_ld(n_rows) */
uint64_t kpop_dev_counter_ld(uint64_t n_rows);
/* d_classes is on the device, fits_host (may be NULL) on the host; the k-mers go through in bands of what
   d_workspace (kpop_dev_counter_distill_workspace_bytes) holds, or of kpop_tune("distill_band", n) k-mers if that
   is fewer: the same bits either way.  Runs on `stream` and returns when it has finished (the fits come back to
   the host).                                                                                                     */
uint64_t kpop_dev_counter_distill_workspace_bytes(uint32_t n_cols, uint64_t n_rows, uint32_t n_classes);
int kpop_dev_counter_distill(const int32_t *d_storage, uint64_t ld, uint32_t n_cols, uint64_t n_rows,
                             const uint32_t *d_classes, uint32_t n_classes, void *d_workspace, double *d_out,
                             double *fits_host, void *stream);
/* development: under kpop_tune("distill_clock", 1) the last distill call on this slot drained its stream after
   every band and kept the milliseconds of its phases: out_ms[0] cells, [1] reduce, [2] fit                      */
int kpop_debug_distill_clocks(double *out_ms);
uint64_t kpop_dev_counter_workspace_bytes(uint32_t n_cols, uint64_t n_rows);
int kpop_dev_counter_stats(const int32_t *d_storage, uint64_t ld, uint32_t n_cols, uint64_t n_rows,
                           double threshold, double power, void *d_workspace, double *d_col_stats,
                           double *d_row_stats, void *stream);
/* d_sel / d_norm list the n_valid selected spectra whose norm is positive, in visiting order; d_workspace needs
   kpop_dev_counter_workspace_bytes(n_valid, n_rows) */
int kpop_dev_counter_combine(const int32_t *d_storage, uint64_t ld, uint64_t n_rows, const uint32_t *d_sel,
                             const double *d_norm, uint32_t n_valid, uint32_t n_sel, double max_norm,
                             int criterion, void *d_workspace, int32_t *d_out, double *d_out_norm, void *stream);
int kpop_dev_counter_transform(const int32_t *d_storage, uint64_t ld, uint32_t n_cols, uint64_t n_rows,
                               int which, double threshold, double power, const double *d_col_stats,
                               int kmer_major, double *d_out, void *stream);
/* test hook: d_fast[i] = a[i] / b[i] by the reciprocal + FMA route the combination kernels use, d_exact[i] by
   the hardware division; the two must be bit-identical */
int kpop_dev_division_probe(const double *d_a, const double *d_b, uint64_t n, double *d_fast, double *d_exact,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif
