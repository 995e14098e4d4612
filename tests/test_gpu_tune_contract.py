"""Every kpop_tune knob held to the effect tests/tune_contract.py states for it, value by value, on the kernels a setting selects and
no default dispatch reaches: the sixteen-deep gathers of the reads kernel and its non-temporal loads ("unroll", "nt", "ldspad"), the
streaming kernel at a caller's segment length and with non-temporal loads ("seg", "nt"), round 4's tile kernel in chunks of 32 and
of 64 sequences with the residual rows' kernel in both builds ("tilepipe", "tileg", "nt"), the priorities of the pipelined one
("pipeprio"), and what the rest of the table had no test for ("dense" 1, "distill_clock").

`want` is the oracle's twist of the oracle's counts (lib/Twister.ml:146-188).  "order" is max|got - want| <= RTOL * max(max|want|, 1),
the tolerance of tests/test_gpu_twist.py; "bits" is np.array_equal with the default's rows, the default reproducible (run twice) and
within the "order" bound itself.  Knobs are set through tune_contract.tuned alone, which puts them back whatever happens."""
import ctypes as C

import numpy as np
import pytest

from conftest import concat
from test_gpu_distill import bits, interleaved, poisson_db
from test_gpu_twist import RTOL, _one_organism
from tune_contract import KNOBS, tuned

pytestmark = pytest.mark.gpu

# mirrors kpop_amd/csrc/count_twist_plan.h (pick_R, kWaveMaxWindows, kTileMinSeqs, kSegWindows, and the segment length:
# default_seg_windows); tests/host/count_twist_plan_check.cpp holds the C++ side to the same formulas without a GPU
WAVE_MAX_WINDOWS, TILE_MIN_SEQS, SEG_WINDOWS_MAX = 512, 16, 16384
DENSE_IMAGE_MAX_ROWS = 36864  # count_twist.hip, kpop_count_twist ("const bool dense_image =")


def pick_R(max_windows):
    return 1 if max_windows <= 64 else 2 if max_windows <= 128 else 4 if max_windows <= 256 else 8


def default_seg_windows(d):
    d_pad = (d + 15) // 16 * 16
    return max(1024, min(SEG_WINDOWS_MAX, (3 << 19) // (d_pad * 8) // 64 * 64))


def assert_order(got, want, what):
    """max|got - want| <= RTOL * max(max|want|, 1); returns the left side over max(max|want|, 1)"""
    assert got.shape == want.shape and got.size
    err, scale = float(np.max(np.abs(got - want))), max(float(np.max(np.abs(want))), 1.0)
    assert err <= RTOL * scale, (what, err, RTOL * scale)
    return err / scale


def windows(seqs, k):
    return [max(len(s_) - k + 1, 0) for s_ in seqs]


# ---------------------------------------------------------------------------------------------------------------------------------
# A. the reads kernel: "unroll" x "nt" (x "ldspad")
# ---------------------------------------------------------------------------------------------------------------------------------
SPECIAL = (1, 15, 16, 17, 33)  # distinct known k-mers of the reads built for it: every alignment of the padded tail of the U = 16 loops


class Reads:
    """300 ragged reads over ACGTN in two batches -- the longest read under 64 windows (R = 1), and between 257 and 512 (R = 8) --, each
    with an empty read, one shorter than k, one of Ns and reads of exactly 1, 15, 16, 17 and 33 distinct k-mers, all of which the
    twister knows; of the other k-mers that occur it knows 95 %, in shuffled column order"""

    def __init__(self, oracle, k, seed):
        rng = np.random.RandomState(seed)
        self.k = k

        def distinct(m):  # m windows, m distinct k-mers (either strand counted once)
            while True:
                read = "".join(rng.choice(list("ACGT"), size=k + m - 1))
                if len(oracle.count_reads(*concat([read]), k)[0]) == m:
                    return read

        special = [distinct(m) for m in SPECIAL]

        def ragged(n, lo, hi):
            return ["".join(rng.choice(list("ACGTN"), size=int(rng.randint(lo, hi)), p=[.245] * 4 + [.02])) for _ in range(n)]

        fixed = ["", "ACGTACGTACGTACGTACGTAC"[:k - 1], "N" * 40] + special
        short = fixed + ragged(300 - len(fixed), k, k + 63)
        mixed = fixed + ragged(270 - len(fixed), k, k + 63) + ragged(30, k + 256, k + 400)
        self.batches = []
        for seqs in (short, mixed):
            order = rng.permutation(len(seqs))
            seqs = [seqs[i] for i in order]
            bases, offs = concat(seqs)
            self.batches.append((seqs, bases, offs, oracle.count_reads(bases, offs, k), [int(np.where(order == 3 + j)[0][0]) for j in range(len(SPECIAL))]))
        assert pick_R(max(windows(self.batches[0][0], k))) == 1 and 256 < max(windows(self.batches[1][0], k)) <= WAVE_MAX_WINDOWS
        sb, so = concat(special)
        must = np.unique(oracle.count_reads(sb, so, k)[0])
        seen = np.unique(np.concatenate([b[3][0] for b in self.batches]))
        cols = np.unique(np.concatenate([seen[rng.rand(len(seen)) < 0.95], must]))
        assert len(cols) < len(seen)  # (some k-mers that occur have no row)
        self.cols = cols[rng.permutation(len(cols))]
        for seqs, bases, offs, (h, c, o), where in self.batches:
            for m, r in zip(SPECIAL, where):
                mine = h[int(o[r]):int(o[r + 1])]
                assert len(mine) == m and np.isin(mine, self.cols).all(), (m, r)  # (the oracle's spectrum: distinct k-mers, all known)

    def want(self, oracle, T, b, normalize):
        h, c, o = self.batches[b][3]
        return oracle.twist(T, self.cols, h, c.astype(np.float64), o, normalize)


@pytest.fixture(scope="module")
def reads8(oracle):
    return Reads(oracle, 8, 8)


@pytest.fixture(scope="module")
def reads21(oracle):
    return Reads(oracle, 21, 21)


def _first_default(kpop, oracle, reads8):
    tw = kpop.Twister.load(oracle.synth_twister(77, 64, reads8.cols), reads8.cols, 8)
    return [tw.count_twist(b[1], b[2]) for b in reads8.batches]


@pytest.fixture(scope="module", autouse=True)
def first_default(kpop, oracle, reads8):
    """workload A at 64 dimensions under the defaults, before any test of this file has set a knob"""
    return _first_default(kpop, oracle, reads8)


def check_reads_settings(oracle, reads, T, tw, run, what):
    for b in range(len(reads.batches)):
        for normalize in (True, False):
            want = reads.want(oracle, T, b, normalize)
            base, again = run(tw, b, normalize), run(tw, b, normalize)
            assert np.array_equal(base, again), (what, b, normalize)
            assert_order(base, want, (what, b, normalize))
            for row, seq in zip(base, reads.batches[b][0]):
                if len(seq) < reads.k or set(seq) <= {"N"}:
                    assert not row.any(), seq  # (no window: a row of zeros)
            got = {}
            for unroll in KNOBS["unroll"]["values"]:
                for nt in (0, 1):
                    with tuned(unroll=unroll, nt=nt):
                        got["unroll", unroll, "nt", nt] = run(tw, b, normalize)
            with tuned(nt=2):
                got["nt", 2] = run(tw, b, normalize)
            for pad in KNOBS["ldspad"]["values"]:
                with tuned(ldspad=pad):
                    got["ldspad", pad] = run(tw, b, normalize)
            for setting, rows in got.items():
                assert np.array_equal(rows, base), (what, b, normalize, setting, float(np.max(np.abs(rows - base))))


@pytest.mark.parametrize("d", [9, 24, 64, 65, 100])
def test_reads_kernel_gives_the_same_bits_at_every_unroll_nt_and_ldspad(kpop, oracle, reads8, d):
    """count_twist_wave_kernel<R, uint32_t, U, NT> for R = 1 and 8: the packed gather at 16 and 32 lanes a row (9, 24), one full block
    (64), wave_gather_rows_tail at one lane of eight (65) and a second ordinary block of 36 (100)"""
    T = oracle.synth_twister(77, d, reads8.cols)
    tw = kpop.Twister.load(T, reads8.cols, 8)
    assert tw.info()["direct_bytes"] == 0
    check_reads_settings(oracle, reads8, T, tw, lambda tw, b, normalize: tw.count_twist(reads8.batches[b][1], reads8.batches[b][2], normalize=normalize), d)
    tw.free()


def test_reads_kernel_from_packed_words_gives_the_same_bits_at_every_nt(kpop, oracle, reads8):
    """kpop_count_twist_packed: count_twist_wave_kernel<.., 8, NT, PACKED> (built at U = 8 only: "unroll" is not read), and the bytes' rows"""
    from kpop_amd import api
    T = oracle.synth_twister(77, 64, reads8.cols)
    tw = kpop.Twister.load(T, reads8.cols, 8)
    packed = [api.pack_bases(b[1]) for b in reads8.batches]
    check_reads_settings(oracle, reads8, T, tw, lambda tw, b, normalize: tw.count_twist_packed(packed[b][0], packed[b][1], reads8.batches[b][2], normalize=normalize), "packed")
    for b in range(2):
        assert np.array_equal(tw.count_twist_packed(packed[b][0], packed[b][1], reads8.batches[b][2]), tw.count_twist(reads8.batches[b][1], reads8.batches[b][2]))
    tw.free()


def test_reads_kernel_with_64_bit_keys_gives_the_same_bits_at_every_unroll_and_nt(kpop, oracle, reads21):
    """k = 21: count_twist_wave_kernel<R, uint64_t, U, NT>"""
    T = oracle.synth_twister(78, 64, reads21.cols)
    tw = kpop.Twister.load(T, reads21.cols, 21)
    check_reads_settings(oracle, reads21, T, tw, lambda tw, b, normalize: tw.count_twist(reads21.batches[b][1], reads21.batches[b][2], normalize=normalize), "k21")
    tw.free()


@pytest.mark.parametrize("d", [9, 24])
def test_reads_kernel_with_rows_at_their_hashes_gives_the_same_bits_at_every_unroll_and_nt(kpop, oracle, reads8, d):
    """a twister loaded under "direct" 1: wave_gather_rows_direct<U, NT>, and -- 5 % of the k-mers that occur have no row -- its second
    pass without them"""
    T = oracle.synth_twister(79, d, reads8.cols)
    with tuned(direct=1):
        tw = kpop.Twister.load(T, reads8.cols, 8)
    assert tw.info()["direct_bytes"] > 0
    check_reads_settings(oracle, reads8, T, tw, lambda tw, b, normalize: tw.count_twist(reads8.batches[b][1], reads8.batches[b][2], normalize=normalize), ("direct", d))
    tw.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# B. the streaming kernel: "seg" x "nt"
# ---------------------------------------------------------------------------------------------------------------------------------
LONGEST = 40000


class Sequences:
    """twelve sequences, eight of them of more than 512 windows (fewer than the tile route bothers with): 600 to 40,000 bases put
    together from pieces of one 4,000-base text with a few substitutions and Ns (so that the twister stays small), "A" * 2000, three
    reads and an empty one"""

    def __init__(self, oracle, k, seed):
        rng = np.random.RandomState(seed)
        text = rng.choice(list("ACGT"), size=4000)

        def pieces(n):
            out = []
            while sum(len(p) for p in out) < n:
                at = int(rng.randint(0, len(text) - 200))
                out.append(text[at:at + int(rng.randint(200, 1500))].copy())
            m = np.concatenate(out)[:n]
            hit = rng.rand(n) < 0.002
            m[hit] = rng.choice(list("ACGTN"), size=int(hit.sum()), p=[.24, .24, .24, .24, .04])
            return "".join(m)

        self.seqs = [pieces(1500), "".join(rng.choice(list("ACGT"), size=150)), pieces(LONGEST), "", pieces(600), "A" * 2000, pieces(12000),
                     "".join(rng.choice(list("ACGTN"), size=97)), pieces(5000), pieces(2600), "ACGTTGCA" * 10, pieces(800)]
        self.k, self.longest = k, 2
        w = windows(self.seqs, k)
        assert len(self.seqs) == 12 and sum(x > WAVE_MAX_WINDOWS for x in w) < TILE_MIN_SEQS and max(w) == w[self.longest] == LONGEST - k + 1
        self.bases, self.offs = concat(self.seqs)
        self.h, self.c, self.o = oracle.count_reads(self.bases, self.offs, k)
        seen = np.unique(self.h)
        cols = seen[rng.rand(len(seen)) < 0.95]
        self.cols = cols[rng.permutation(len(cols))]


@pytest.fixture(scope="module")
def sequences11(oracle):
    return Sequences(oracle, 11, 11)


@pytest.fixture(scope="module")
def sequences17(oracle):
    return Sequences(oracle, 17, 17)


def check_stream_settings(kpop, oracle, S, d):
    T = oracle.synth_twister(80, d, S.cols)
    tw = kpop.Twister.load(T, S.cols, S.k)
    W = LONGEST - S.k + 1
    n_seg = {seg: -(-W // (seg or default_seg_windows(d))) for seg in KNOBS["seg"]["values"]}
    assert n_seg[64] == 625 and n_seg[16384] == 3 and n_seg[0] not in (625, 3), n_seg  # (by default 7 at 24 dimensions, 14 at 64, 24 at 100, 40 at 300)
    worst = {}
    for normalize in (True, False):
        want = oracle.twist(T, S.cols, S.h, S.c.astype(np.float64), S.o, normalize)
        base, again = tw.count_twist(S.bases, S.offs, normalize=normalize), tw.count_twist(S.bases, S.offs, normalize=normalize)
        assert np.array_equal(base, again)
        assert_order(base, want, ("default", d, normalize))
        assert not base[3].any()
        got = {}
        for seg in KNOBS["seg"]["values"]:
            for nt in (0, 1):
                with tuned(seg=seg, nt=nt):
                    got[seg, nt] = tw.count_twist(S.bases, S.offs, normalize=normalize)
            worst[seg] = max(worst.get(seg, 0.0), assert_order(got[seg, 0], want, ("seg", seg, d, normalize)))
            assert np.array_equal(got[seg, 1], got[seg, 0]), ("nt", seg, d, normalize)
        assert np.array_equal(got[0, 0], base)
        # (another segmentation did run: the longest sequence's partial sums are cut elsewhere)
        assert not np.array_equal(got[64, 0][S.longest], base[S.longest]) and not np.array_equal(got[16384, 0][S.longest], base[S.longest])
    print("seg: k=%d d=%d max|got - want| / max(max|want|, 1): %s" % (S.k, d, "  ".join("%d: %.2e" % (s_, e) for s_, e in sorted(worst.items()))))
    tw.free()


@pytest.mark.parametrize("d", [24, 64, 100, 300])
def test_streaming_kernel_at_every_segment_length_and_nt(kpop, oracle, sequences11, d):
    """count_twist_stream_kernel<uint32_t, NT, B>: one, two and four blocks of dimensions a pass, 300 = 256 + 44 in two launches; segments of 64
    windows (a wavefront of the four has work), 1,024, 16,384 and the default's.  "nt" gives the same bits at the same "seg", "seg" 0 the
    default's, any other the oracle's rows within the tolerance"""
    check_stream_settings(kpop, oracle, sequences11, d)


def test_streaming_kernel_with_64_bit_keys_at_every_segment_length_and_nt(kpop, oracle, sequences17):
    """k = 17: count_twist_stream_kernel<uint64_t, NT, 1>"""
    check_stream_settings(kpop, oracle, sequences17, 24)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. the tile routes: "tilepipe" x "tileg" x "nt" x "pipeprio"
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def organism(oracle):
    """70 assemblies of one organism -- a full chunk of 64 and one of 6; of 32: two full ones and one of 6 --, strangers and reads"""
    rng = np.random.RandomState(70)
    k = 11
    seqs = _one_organism(rng, 70, 3000, 0.003)
    assert sum(x > WAVE_MAX_WINDOWS for x in windows(seqs, k)) >= 70 + TILE_MIN_SEQS // 2
    bases, offs = concat(seqs)
    h, c, o = oracle.count_reads(bases, offs, k)
    cols = np.unique(h)
    cols = cols[rng.rand(len(cols)) < 0.95]
    assert len(cols) > DENSE_IMAGE_MAX_ROWS  # (kpop_count_twist must not take the dense image: that route reads none of these knobs)
    return k, bases, offs, (h, c, o), cols[rng.permutation(len(cols))]


@pytest.mark.parametrize("d", [40, 64, 72, 130])
def test_tile_routes_at_every_tilepipe_tileg_nt_and_pipeprio(kpop, oracle, organism, d):
    """up to 64 dimensions the exchanging kernel of tile_pipe.h, beyond its three-stage form; under "tilepipe" 0 count_twist_tile_kernel<uint32_t, G>
    for G = 64 and 32 -- beyond 64 dimensions with tile_residual_kernel<NT> behind it.  "tilepipe" and "tileg" change the order of additions,
    "nt" gives the same bits at the same "tileg", "pipeprio" the same bits at every value, and "tileg" is not read while "tilepipe" is 1"""
    k, bases, offs, (h, c, o), cols = organism
    T = oracle.synth_twister(81, d, cols)
    tw = kpop.Twister.load(T, cols, k)
    worst = {}
    for normalize in (True, False):
        want = oracle.twist(T, cols, h, c.astype(np.float64), o, normalize)
        run = lambda: tw.count_twist(bases, offs, normalize=normalize)
        base, again = run(), run()
        assert np.array_equal(base, again)
        assert_order(base, want, ("default", d, normalize))
        with tuned(dense=0):
            plain = run()
        assert_order(plain, want, ("dense=0", d, normalize))
        assert not np.array_equal(base, plain)  # (another order of additions: the tile route did run)
        with tuned(dense=2, tilepipe=1, tileg=32):
            assert np.array_equal(run(), base)
        r4 = {}
        for tileg in KNOBS["tileg"]["values"]:
            for nt in (0, 1):
                with tuned(tilepipe=0, tileg=tileg, nt=nt):
                    r4[tileg, nt] = run()
            worst[tileg] = max(worst.get(tileg, 0.0), assert_order(r4[tileg, 0], want, ("tilepipe=0", tileg, d, normalize)))
            assert np.array_equal(r4[tileg, 1], r4[tileg, 0]), ("nt", tileg, d, normalize)
            assert not np.array_equal(r4[tileg, 0], plain)  # (round 4's kernel did run)
        assert not np.array_equal(r4[32, 0], r4[64, 0])  # (other seeds, another consensus set: the chunks of 32 did run)
        if d in (64, 130):
            for prio in KNOBS["pipeprio"]["values"]:
                with tuned(pipeprio=prio):
                    assert np.array_equal(run(), base), (prio, d, normalize)
    print("tileg (tilepipe=0): d=%d max|got - want| / max(max|want|, 1): %s" % (d, "  ".join("%d: %.2e" % (g, e) for g, e in sorted(worst.items()))))
    tw.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# D. the rest of the table: the values no other file sets
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,shuffled", [(9, False), (200, False), (9, True)])
def test_kpop_twist_always_through_the_dense_contraction(kpop, oracle, d, shuffled):
    """"dense" 1: kpop_twist takes the contraction on the matrix cores whatever the batch -- 40 spectra, where the default (2) and 0 both keep the
    line-by-line kernel: lines in ascending order up to 160 dimensions through the fused kernel, beyond it or in any other order through the dense image"""
    rng = np.random.RandomState(d)
    k = 7
    bases, offs = concat(["".join(rng.choice(list("ACGTN"), size=int(n), p=[.2475] * 4 + [.01])) for n in rng.randint(k, 4000, size=38)] + ["", "ACG"])
    h, c, o = oracle.count_reads(bases, offs, k)
    if shuffled:
        for r in range(len(o) - 1):
            p = rng.permutation(int(o[r + 1] - o[r])) + int(o[r])
            h[int(o[r]):int(o[r + 1])], c[int(o[r]):int(o[r + 1])] = h[p], c[p]
    cols = oracle.enumerate_kmers(k)
    cols = cols[rng.rand(len(cols)) < 0.9]
    T = oracle.synth_twister(82, d, cols)
    tw = kpop.Twister.load(T, cols, k)
    for normalize in (True, False):
        want = oracle.twist(T, cols, h, c.astype(np.float64), o, normalize)
        res = {}
        for mode in KNOBS["dense"]["values"]:
            with tuned(dense=mode):
                res[mode] = tw.twist(h, c.astype(np.float64), o, normalize=normalize)
            assert_order(res[mode], want, ("dense", mode, d, shuffled, normalize))
        assert np.array_equal(res[0], res[2]) and not np.array_equal(res[1], res[0])
        assert not res[1][-1].any() and not res[1][-2].any()
    tw.free()


def test_distill_with_its_phase_clocks_gives_the_same_bits(kpop):
    """"distill_clock" 1 drains the stream after every band and keeps three times (kpop_debug_distill_clocks): no result changes"""
    from kpop_amd import _lib
    counts, classes = poisson_db(41, 26, 5000, 4.0), interleaved(26, 3)
    want, want_fits = kpop.counter_distill(list(counts), classes)
    ms = (C.c_double * 3)(-1.0, -1.0, -1.0)
    with tuned(distill_clock=1):
        got, got_fits = kpop.counter_distill(list(counts), classes)
        assert _lib.load().kpop_debug_distill_clocks(ms) == 0
    with tuned(distill_clock=0):
        off, off_fits = kpop.counter_distill(list(counts), classes)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(np.asarray(got_fits)), bits(np.asarray(want_fits)))
    assert np.array_equal(bits(off), bits(want)) and np.array_equal(bits(np.asarray(off_fits)), bits(np.asarray(want_fits)))
    assert all(t >= 0.0 for t in ms) and sum(ms) > 0.0, list(ms)


def test_the_defaults_hold_after_every_tuned_block(kpop, oracle, reads8, first_default):
    """there is no getter: the last test of the file runs workload A under whatever the knobs now are, and must find the rows the file's first
    call found under the defaults"""
    for got, was in zip(_first_default(kpop, oracle, reads8), first_default):
        assert np.array_equal(got, was)
