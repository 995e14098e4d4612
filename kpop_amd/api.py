"""Host-side mirror of the reference's hot-path interface, over the C ABI.

Names follow the reference (PaoloRibeca/KPop):
  count_reads        KMerCounter.compute            bin/KPopCount.ml:26-63
  Twister            Twister.t + add_twisted_...    lib/Twister.ml:22-25,58-206
  metric_compute     Space.Distance.Metric.compute  lib/Space.ml:88-105
  distance_rowwise   Matrix.get_distance_rowwise    lib/Matrix.ml:191-266
  distance_summary   Matrix.summarize_rowwise       lib/Matrix.ml:691-766

Everything here is plumbing (numpy <-> pointers); the arithmetic runs in the
HIP kernels of libkpop_hip.so.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import KPopError, check  # noqa: F401

DNA_DS, DNA_SS, PROTEIN = 0, 1, 2
EUCLIDEAN, COSINE, MINKOWSKI = 0, 1, 2
METRIC_FLAT, METRIC_POWERS = 0, 1

_DISTANCES = {"euclidean": EUCLIDEAN, "cosine": COSINE, "minkowski": MINKOWSKI}


def _p(a, ty):
    return a.ctypes.data_as(C.POINTER(ty))


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _nz(a, dt):
    """ctypes needs a valid pointer even for empty arrays."""
    return a if a.size else np.zeros(1, dtype=dt)


_CTYPE = {np.dtype(np.float64): C.c_double, np.dtype(np.uint32): C.c_uint32, np.dtype(np.uint64): C.c_uint64}


def _ptr(a):
    """the array as the typed pointer the C ABI takes (an empty one: a valid pointer all the same)"""
    return _p(_nz(a, a.dtype), _CTYPE[a.dtype])


def _pointers(res):
    return [_ptr(x) for x in res]


def init(device=0):
    check(_lib.load().kpop_init(int(device)))


def init_devices(devices):
    """Several GPUs in one process: devices[i] becomes device slot i (kpop_init_devices)."""
    arr = (C.c_int * len(devices))(*[int(d) for d in devices])
    check(_lib.load().kpop_init_devices(arr, len(devices)))


def use_device(slot):
    """The calling thread's device slot (thread-local, like hipSetDevice)."""
    check(_lib.load().kpop_use_device(int(slot)))


def device_slots():
    return int(_lib.load().kpop_device_slots())


def pack_bases(bases, threads=0):
    """one byte a base -> (codes, invalid): 16 bases a uint32 of 2-bit codes (A0 C1 G2 T3, either case), one bit a base that is none of
    ACGTacgt (32 a uint32) -- kpop_pack_bases; 2.25 bits a base for the *_packed entry points"""
    bases = _c(bases, np.uint8)
    n = bases.size
    lib = _lib.load()
    codes = np.zeros(max(int(lib.kpop_packed_code_words(n)), 1), dtype=np.uint32)
    invalid = np.zeros(max(int(lib.kpop_packed_mask_words(n)), 1), dtype=np.uint32)
    check(lib.kpop_pack_bases(_nz(bases, np.uint8).ctypes.data, n, codes.ctypes.data, invalid.ctypes.data, int(threads)))
    return codes, invalid


def dev_unpack_bases(d_codes, d_invalid, n_bases, d_bases, stream=0):
    check(_lib.load().kpop_dev_unpack_bases(d_codes, d_invalid, int(n_bases), d_bases, stream))


def dev_count_twist_packed(tw, d_codes, d_invalid, d_offsets, n_reads, n_bases, max_len, d_out, content=DNA_DS, normalize=True, stream=0):
    check(_lib.load().kpop_dev_count_twist_packed(tw.handle, d_codes, d_invalid, d_offsets, int(n_reads), int(n_bases), int(max_len), int(content),
                                                  1 if normalize else 0, d_out, stream))


def tune(key, value):
    """Performance knobs for A/B runs (kpop_tune, include/kpop_hip.h).  Most leave every bit of the results alone; "seg", "dense", "tilepipe",
    "tileg", "tilecap_mb" and "direct" change the order of additions (1e-12 of the result's scale), "distance_mfma" and the "summary*" family
    choose among the matrix cores' approximations; the header says which knob is which, tests/tune_contract.py keeps the table."""
    check(_lib.load().kpop_tune(key.encode(), int(value)))


def debug_counters(n=16):
    """the development phase clocks of kpop_debug_counters (read and cleared)"""
    out = (C.c_uint64 * 16)()
    check(_lib.load().kpop_debug_counters(out, int(n)))
    return [int(x) for x in out[:n]]


def summary_fallbacks():
    """query rows the large-reference summaries left to their exact fall-back since the last call (counted under tune("summary_audit", 1))"""
    out = C.c_uint64(0)
    check(_lib.load().kpop_debug_summary_fallbacks(C.byref(out)))
    return int(out.value)


def device_count():
    n = _lib.load().kpop_device_count()
    if n < 0:
        check(n)
    return n


def parse_distance(name):
    """Space.Distance.of_string, lib/Space.ml:208-225: 'euclidean' | 'cosine' | 'minkowski(p)'."""
    if name in ("euclidean", "cosine"):
        return _DISTANCES[name], 2.0
    if name.startswith("minkowski(") and name.endswith(")"):
        try:
            p = float(name[len("minkowski("):-1])
        except ValueError:
            raise ValueError("Unknown_distance %r" % name)
        if p < 0:
            raise ValueError("Negative_power %r" % p)
        return MINKOWSKI, p
    raise ValueError("Unknown_distance %r" % name)


# ------------------------------------------------------------------ count
def count_reads(bases, offsets, k, content=DNA_DS, per_read=True, capacity=None):
    """-> (hash u64[], count u32[], offsets u64[]) CSR of per-read spectra (-L) or one spectrum (-l)."""
    bases = _c(bases, np.uint8)
    offsets = _c(offsets, np.uint64)
    n = len(offsets) - 1
    if capacity is None:
        capacity = int(offsets[-1] - offsets[0]) + 1 if n > 0 else 1
    oh = np.empty(capacity, dtype=np.uint64)
    oc = np.empty(capacity, dtype=np.uint32)
    oo = np.zeros(n + 1 if per_read else 2, dtype=np.uint64)
    bb = _nz(bases, np.uint8)
    check(_lib.load().kpop_count_reads(_p(bb, C.c_uint8), _p(offsets, C.c_uint64), n, int(k), int(content),
                                       1 if per_read else 0, _p(oh, C.c_uint64), _p(oc, C.c_uint32),
                                       _p(oo, C.c_uint64), capacity))
    t = int(oo[-1])
    return oh[:t].copy(), oc[:t].copy(), oo


# ---------------------------------------------------------------- twister
class Twister:
    """Device-resident twister (lib/Twister.ml:22-25 + the name->column table of :71-76)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def load(cls, T_dims_major, col_hash, k):
        T = _c(T_dims_major, np.float64)
        if T.ndim != 2:
            raise ValueError("twister must be n_dims x n_cols")
        n_dims, n_cols = T.shape
        col_hash = _c(col_hash, np.uint64)
        if len(col_hash) != n_cols:
            raise ValueError("col_hash length %d <> n_cols %d" % (len(col_hash), n_cols))
        h = C.c_void_p()
        check(_lib.load().kpop_twister_load(_p(_nz(T, np.float64), C.c_double), n_cols, n_dims,
                                            _p(_nz(col_hash, np.uint64), C.c_uint64), int(k), C.byref(h)))
        return cls(h)

    @classmethod
    def synth(cls, seed, k, n_dims, content=DNA_DS, hash_range=None, acc_dim=False):
        """Synthetic twister generated on the device; hash_range=(lo, hi) keeps only that slice of k-mer rows and
        acc_dim appends the all-ones dimension of a k-mer-row shard (kpop_amd/shard.py)."""
        h = C.c_void_p()
        if hash_range is None and not acc_dim:
            check(_lib.load().kpop_twister_synth(int(seed), int(k), int(content), int(n_dims), C.byref(h)))
        else:
            lo, hi = hash_range if hash_range is not None else (0, 1 << (2 * int(k)))
            check(_lib.load().kpop_twister_synth_slice(int(seed), int(k), int(content), int(n_dims), int(lo), int(hi),
                                                       1 if acc_dim else 0, C.byref(h)))
        return cls(h)

    @classmethod
    def load_slice(cls, T_dims_major, col_hash, k, hash_range):
        """The k-mer-row shard of a real twister: the columns with hash in [lo, hi), plus the all-ones dimension."""
        T = _c(T_dims_major, np.float64)
        col_hash = _c(col_hash, np.uint64)
        keep = (col_hash >= np.uint64(hash_range[0])) & (col_hash < np.uint64(hash_range[1]))
        Ts = np.vstack([T[:, keep], np.ones((1, int(keep.sum())))])
        return cls.load(Ts, col_hash[keep], k)

    @property
    def handle(self):
        return self._h

    def info(self):
        n_cols, n_dims, k, nbytes = C.c_uint64(), C.c_uint32(), C.c_int(), C.c_uint64()
        check(_lib.load().kpop_twister_info(self._h, C.byref(n_cols), C.byref(n_dims), C.byref(k),
                                            C.byref(nbytes)))
        direct = C.c_uint64()
        check(_lib.load().kpop_twister_direct_bytes(self._h, C.byref(direct)))
        return {"n_cols": n_cols.value, "n_dims": n_dims.value, "k": k.value, "device_bytes": nbytes.value, "direct_bytes": direct.value}

    def twist(self, hash_, value, offsets, normalize=True):
        """Spectra (CSR of hash,value lines) -> twisted rows; lib/Twister.ml:146-188."""
        hash_ = _c(hash_, np.uint64)
        value = _c(value, np.float64)
        offsets = _c(offsets, np.uint64)
        n = len(offsets) - 1
        out = np.zeros((n, self.info()["n_dims"]), dtype=np.float64)
        check(_lib.load().kpop_twist(self._h, _p(_nz(hash_, np.uint64), C.c_uint64),
                                     _p(_nz(value, np.float64), C.c_double), _p(offsets, C.c_uint64), n,
                                     1 if normalize else 0, _p(_nz(out, np.float64), C.c_double)))
        return out

    def count_twist(self, bases, offsets, content=DNA_DS, normalize=True):
        """Reads -> twisted rows, count and twist fused on the device."""
        bases = _c(bases, np.uint8)
        offsets = _c(offsets, np.uint64)
        n = len(offsets) - 1
        out = np.zeros((n, self.info()["n_dims"]), dtype=np.float64)
        check(_lib.load().kpop_count_twist(self._h, _p(_nz(bases, np.uint8), C.c_uint8),
                                           _p(offsets, C.c_uint64), n, int(content), 1 if normalize else 0,
                                           _p(_nz(out, np.float64), C.c_double)))
        return out

    def count_twist_packed(self, codes, invalid, offsets, content=DNA_DS, normalize=True):
        """The same from the packed form (pack_bases): 2.25 bits a base over the bus, the same rows bit for bit."""
        codes = _c(codes, np.uint32)
        invalid = _c(invalid, np.uint32)
        offsets = _c(offsets, np.uint64)
        n = len(offsets) - 1
        out = np.zeros((n, self.info()["n_dims"]), dtype=np.float64)
        check(_lib.load().kpop_count_twist_packed(self._h, _nz(codes, np.uint32).ctypes.data, _nz(invalid, np.uint32).ctypes.data, _p(offsets, C.c_uint64), n,
                                                  int(content), 1 if normalize else 0, _p(_nz(out, np.float64), C.c_double)))
        return out

    def spectra_twist(self, bases, offsets, k, content=DNA_DS, normalize=True):
        """Reads -> the rows count_reads(k) + twist would give, bit for bit, spectra kept on the device (any length)."""
        bases = _c(bases, np.uint8)
        offsets = _c(offsets, np.uint64)
        n = len(offsets) - 1
        out = np.zeros((n, self.info()["n_dims"]), dtype=np.float64)
        check(_lib.load().kpop_spectra_twist(self._h, _p(_nz(bases, np.uint8), C.c_uint8), _p(offsets, C.c_uint64), n, int(k),
                                             int(content), 1 if normalize else 0, _p(_nz(out, np.float64), C.c_double)))
        return out

    def set_count_k(self, k):
        check(_lib.load().kpop_twister_set_count_k(self._h, int(k)))

    def free(self):
        if self._h is not None and self._h.value:
            _lib.load().kpop_twister_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ------------------------------------------------------- streaming pipeline
OUT_TWISTED, OUT_DISTANCES, OUT_SUMMARY = 1, 2, 4


class _HostBlock:
    """One kpop_host_alloc'ed block, freed when the last array over it goes."""

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        check(_lib.load().kpop_host_alloc(C.byref(self.ptr), int(max(nbytes, 1))))
        self.nbytes = int(max(nbytes, 1))

    def __del__(self):
        try:
            if self.ptr and self.ptr.value:
                _lib.load().kpop_host_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


def host_empty(shape, dtype):
    """numpy array over page-locked host memory (kpop_host_alloc): what the streaming pipeline copies to and from at
    the bus rate.  An OCaml binding does the same with Ctypes.bigarray_of_ptr."""
    dt = np.dtype(dtype)
    shape = (shape,) if np.isscalar(shape) else tuple(int(x) for x in shape)
    n = int(np.prod(shape)) if shape else 1
    blk = _HostBlock(n * dt.itemsize)
    buf = (C.c_char * blk.nbytes).from_address(blk.ptr.value)
    buf._kpop_block = blk  # the array's base is buf: the block lives as long as any view of it
    return np.frombuffer(buf, dtype=dt, count=n).reshape(shape)


class Pipeline:
    """Reads in host memory -> twisted rows / distances to `classes` / per-read summary, streamed through the GPU in
    chunks on three streams (kpop_pipeline_*): the README.md:606 + :641/:656 chain as one call."""

    def __init__(self, tw, classes=None, metric=None, outputs=OUT_TWISTED | OUT_DISTANCES, content=DNA_DS,
                 normalize_counts=True, kind=EUCLIDEAN, p=2.0, normalize_distances=True, keep_at_most=2,
                 max_neighbours=8, chunk_reads=0, depth=0, chunk_bases=0, record_timeline=False):
        self.tw = tw
        self.n_dims = tw.info()["n_dims"]
        self.outputs = int(outputs)
        self.max_neighbours = int(max_neighbours)
        cfg = _lib.PipelineConfig()
        cfg.struct_size = C.sizeof(_lib.PipelineConfig)
        cfg.content, cfg.normalize_counts = int(content), 1 if normalize_counts else 0
        cfg.kind, cfg.p, cfg.normalize_distances = int(kind), float(p), 1 if normalize_distances else 0
        cfg.outputs, cfg.keep_at_most, cfg.max_neighbours = self.outputs, int(keep_at_most or 0), self.max_neighbours
        cfg.chunk_reads, cfg.depth, cfg.chunk_bases = int(chunk_reads), int(depth), int(chunk_bases)
        cfg.record_timeline = 1 if record_timeline else 0
        self.n_classes = 0
        cp = mp = None
        if classes is not None:
            classes = _c(classes, np.float64)
            metric = _c(metric, np.float64)
            if classes.ndim != 2 or classes.shape[1] != self.n_dims or len(metric) != self.n_dims:
                raise ValueError("Incompatible_geometries")  # lib/Matrix.ml:193-194
            self.n_classes = classes.shape[0]
            cp, mp = _p(classes, C.c_double), _p(metric, C.c_double)
        self._h = C.c_void_p()
        check(_lib.load().kpop_pipeline_create(tw.handle, cp, self.n_classes, mp, C.byref(cfg), C.byref(self._h)))
        self._pending = {}

    def alloc_outputs(self, n_reads, pinned=True):
        """dict of output arrays for a batch of n_reads (page-locked unless pinned=False)"""
        mk = host_empty if pinned else (lambda shape, dt: np.empty(shape, dtype=dt))
        n, o = max(int(n_reads), 1), {}
        if self.outputs & OUT_TWISTED:
            o["twisted"] = mk((n, self.n_dims), np.float64)[:n_reads]
        if self.outputs & OUT_DISTANCES:
            o["distances"] = mk((n, self.n_classes), np.float64)[:n_reads]
        if self.outputs & OUT_SUMMARY:
            mn = max(self.max_neighbours, 1)
            o["stats"] = mk((n, 4), np.float64)[:n_reads]
            o["n_neighbours"] = mk((n,), np.uint32)[:n_reads]
            o["nb_index"] = mk((n, mn), np.uint32)[:n_reads, :self.max_neighbours]
            o["nb_distance"] = mk((n, mn), np.float64)[:n_reads, :self.max_neighbours]
            o["nb_z"] = mk((n, mn), np.float64)[:n_reads, :self.max_neighbours]
        return o

    def submit(self, bases, offsets, out):
        """enqueue one batch; bases (uint8), offsets (uint64, n+1) and the arrays of `out` must stay alive and untouched
        until collect(ticket).  -> ticket"""
        if bases.dtype != np.uint8 or offsets.dtype != np.uint64 or not bases.flags.c_contiguous or not offsets.flags.c_contiguous:
            raise ValueError("bases must be contiguous uint8 and offsets contiguous uint64")
        n = len(offsets) - 1
        po = _lib.PipelineOutputs()
        for name in ("twisted", "distances", "stats", "n_neighbours", "nb_index", "nb_distance", "nb_z"):
            a = out.get(name)
            if a is not None:
                if not a.flags.c_contiguous:
                    raise ValueError("output %s is not contiguous" % name)
                setattr(po, name, a.ctypes.data)
        tk = C.c_uint64()
        check(_lib.load().kpop_pipeline_submit(self._h, bases.ctypes.data, offsets.ctypes.data, n, C.byref(po), C.byref(tk)))
        self._pending[tk.value] = (bases, offsets, out)
        return tk.value

    def submit_packed(self, codes, invalid, offsets, out):
        """submit() with the batch in the packed form (pack_bases): what goes up the bus is 2.25 bits a base"""
        for a, dt in ((codes, np.uint32), (invalid, np.uint32), (offsets, np.uint64)):
            if a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError("codes / invalid must be contiguous uint32 and offsets contiguous uint64")
        n = len(offsets) - 1
        po = _lib.PipelineOutputs()
        for name in ("twisted", "distances", "stats", "n_neighbours", "nb_index", "nb_distance", "nb_z"):
            a = out.get(name)
            if a is not None:
                if not a.flags.c_contiguous:
                    raise ValueError("output %s is not contiguous" % name)
                setattr(po, name, a.ctypes.data)
        tk = C.c_uint64()
        check(_lib.load().kpop_pipeline_submit_packed(self._h, codes.ctypes.data, invalid.ctypes.data, offsets.ctypes.data, n, C.byref(po), C.byref(tk)))
        self._pending[tk.value] = (codes, invalid, offsets, out)
        return tk.value

    def collect(self, ticket):
        check(_lib.load().kpop_pipeline_collect(self._h, int(ticket)))
        for t in [t for t in self._pending if t <= ticket]:
            del self._pending[t]

    def run(self, bases, offsets, out=None, pinned_outputs=True):
        """one batch, start to finish -> dict of output arrays"""
        bases = _c(bases, np.uint8)
        offsets = _c(offsets, np.uint64)
        if out is None:
            out = self.alloc_outputs(len(offsets) - 1, pinned=pinned_outputs)
        self.collect(self.submit(bases, offsets, out))
        return out

    def timeline(self, max_chunks=256):
        """[chunks, 6] ms from the first upload's start: upload start/end, kernels start/end, download start/end of every
        chunk of the last submit (record_timeline pipelines, after collect)"""
        ms = np.zeros((max_chunks, 6))
        n = C.c_uint32()
        check(_lib.load().kpop_pipeline_timeline(self._h, int(max_chunks), _p(ms, C.c_double), C.byref(n)))
        return ms[:n.value]

    def stats(self):
        ch, pin, dep = C.c_uint32(), C.c_int(), C.c_uint32()
        check(_lib.load().kpop_pipeline_stats(self._h, C.byref(ch), C.byref(pin), C.byref(dep)))
        return {"chunks": ch.value, "pinned": bool(pin.value), "depth": dep.value}

    def close(self):
        if self._h is not None and self._h.value:
            _lib.load().kpop_pipeline_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------ several GPUs
def shard_bounds(n_items, rank, world):
    """kpop_shard_bounds: rows [lo, hi) of n_items owned by `rank` of `world` (host arithmetic, no GPU)"""
    lo, hi = C.c_uint64(), C.c_uint64()
    check(_lib.load().kpop_shard_bounds(int(n_items), int(rank), int(world), C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


class Sharded:
    """One batch over every device slot of kpop_init_devices, from inside the library (kpop_sharded_*): one streaming
    pipeline and one host thread per device; replaces `-T` and the fork()ed workers of lib/Twister.ml:90-196."""

    def __init__(self, tw, classes=None, metric=None, outputs=OUT_TWISTED | OUT_DISTANCES, content=DNA_DS,
                 normalize_counts=True, kind=EUCLIDEAN, p=2.0, normalize_distances=True, keep_at_most=2,
                 max_neighbours=8, chunk_reads=0, depth=0, chunk_bases=0):
        self.tw = tw
        self.n_dims = tw.info()["n_dims"]
        self.outputs, self.max_neighbours = int(outputs), int(max_neighbours)
        cfg = _lib.PipelineConfig()
        cfg.struct_size = C.sizeof(_lib.PipelineConfig)
        cfg.content, cfg.normalize_counts = int(content), 1 if normalize_counts else 0
        cfg.kind, cfg.p, cfg.normalize_distances = int(kind), float(p), 1 if normalize_distances else 0
        cfg.outputs, cfg.keep_at_most, cfg.max_neighbours = self.outputs, int(keep_at_most or 0), self.max_neighbours
        cfg.chunk_reads, cfg.depth, cfg.chunk_bases = int(chunk_reads), int(depth), int(chunk_bases)
        self.n_classes = 0
        cp = mp = None
        if metric is not None:
            metric = _c(metric, np.float64)
            mp = _p(metric, C.c_double)
        if classes is not None:
            classes = _c(classes, np.float64)
            if classes.ndim != 2 or classes.shape[1] != self.n_dims or metric is None or len(metric) != self.n_dims:
                raise ValueError("Incompatible_geometries")
            self.n_classes = classes.shape[0]
            cp = _p(classes, C.c_double)
        self._h = C.c_void_p()
        check(_lib.load().kpop_sharded_create(tw.handle, cp, self.n_classes, mp, C.byref(cfg), C.byref(self._h)))
        self.slots = int(_lib.load().kpop_sharded_slots(self._h))

    alloc_outputs = Pipeline.alloc_outputs

    def run(self, bases, offsets, out=None, pinned_outputs=True):
        """host memory -> host memory over all devices; rows of shard s are written by device s"""
        bases = _c(bases, np.uint8)
        offsets = _c(offsets, np.uint64)
        n = len(offsets) - 1
        if out is None:
            out = self.alloc_outputs(n, pinned=pinned_outputs)
        po = _lib.PipelineOutputs()
        for name in ("twisted", "distances", "stats", "n_neighbours", "nb_index", "nb_distance", "nb_z"):
            a = out.get(name)
            if a is not None:
                setattr(po, name, a.ctypes.data)
        check(_lib.load().kpop_sharded_run(self._h, bases.ctypes.data, offsets.ctypes.data, n, C.byref(po)))
        return out

    def resident_step(self, d_bases, d_offsets, n_reads, n_bases, max_len, chunks=4, gather=True):
        """device-resident config-4 step; d_bases / d_offsets: one device pointer per slot (in that slot's HBM)"""
        n = self.slots
        pb = (C.c_void_p * n)(*[int(x) for x in d_bases])
        po = (C.c_void_p * n)(*[int(x) for x in d_offsets])
        nr = (C.c_uint32 * n)(*[int(x) for x in n_reads])
        nb = (C.c_uint64 * n)(*[int(x) for x in n_bases])
        check(_lib.load().kpop_sharded_resident_step(self._h, pb, po, nr, nb, int(max_len), int(chunks), 1 if gather else 0))

    def resident_buffers(self, slot):
        full, dist = C.c_void_p(), C.c_void_p()
        first, rows = C.c_uint64(), C.c_uint64()
        check(_lib.load().kpop_sharded_resident_buffers(self._h, int(slot), C.byref(full), C.byref(first), C.byref(rows), C.byref(dist)))
        return full.value, first.value, rows.value, dist.value

    def timings(self, slot):
        a, b = C.c_double(), C.c_double()
        check(_lib.load().kpop_sharded_timings(self._h, int(slot), C.byref(a), C.byref(b)))
        return {"ms_compute": a.value, "ms_exposed_comm": b.value}

    def chunk_timings(self, slot, max_chunks=64):
        """ms of the fused count->twist launches of the last resident step on that slot, chunk by chunk (HIP events)"""
        ms = (C.c_double * int(max_chunks))()
        n = C.c_int()
        check(_lib.load().kpop_sharded_chunk_timings(self._h, int(slot), ms, int(max_chunks), C.byref(n)))
        return [float(ms[i]) for i in range(n.value)]

    def all_vs_all_summary(self, queries_per_slot=0, keep_at_most=2, max_neighbours=8, capacity=None):
        """after resident_step(gather=True) -> (query global ids, stats, n, idx, dist, z), one row per query"""
        cap = int(capacity if capacity is not None else max(1, queries_per_slot) * self.slots)
        mn = max(int(max_neighbours), 1)
        q = np.zeros(cap, dtype=np.uint64)
        stats = np.zeros((cap, 4))
        n = np.zeros(cap, dtype=np.uint32)
        idx = np.zeros((cap, mn), dtype=np.uint32)
        dd = np.zeros((cap, mn))
        z = np.zeros((cap, mn))
        got = C.c_uint64()
        check(_lib.load().kpop_sharded_all_vs_all_summary(self._h, int(queries_per_slot), int(keep_at_most or 0), int(max_neighbours), cap,
                                                          C.byref(got), _p(q, C.c_uint64), _p(stats, C.c_double), _p(n, C.c_uint32),
                                                          _p(idx, C.c_uint32), _p(dd, C.c_double), _p(z, C.c_double)))
        g = got.value
        return q[:g], stats[:g], n[:g], idx[:g], dd[:g], z[:g]

    def close(self):
        if self._h is not None and self._h.value:
            _lib.load().kpop_sharded_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sharded_distance_rowwise(m1, m2, metric, kind=EUCLIDEAN, p=2.0, normalize=True):
    """distance_rowwise with the rows of m2 cut over the device slots"""
    m1, m2, metric = _c(m1, np.float64), _c(m2, np.float64), _c(metric, np.float64)
    r1, d = m1.shape
    r2 = m2.shape[0]
    out = np.zeros((r2, r1))
    check(_lib.load().kpop_sharded_distance_rowwise(_p(_nz(m1, np.float64), C.c_double), r1, _p(_nz(m2, np.float64), C.c_double), r2, d,
                                                    _p(metric, C.c_double), int(kind), float(p), 1 if normalize else 0,
                                                    _p(_nz(out, np.float64), C.c_double)))
    return out


def sharded_distance_summary(m1, m2, metric, kind=EUCLIDEAN, p=2.0, normalize=True, keep_at_most=2, max_neighbours=8):
    """distance_summary with the rows of m2 cut over the device slots"""
    m1, m2, metric = _c(m1, np.float64), _c(m2, np.float64), _c(metric, np.float64)
    r1, d = m1.shape
    r2 = m2.shape[0]
    mn = max(int(max_neighbours), 1)
    stats = np.zeros((r2, 4))
    n = np.zeros(r2, dtype=np.uint32)
    idx = np.zeros((r2, mn), dtype=np.uint32)
    dist = np.zeros((r2, mn))
    z = np.zeros((r2, mn))
    check(_lib.load().kpop_sharded_distance_summary(_p(_nz(m1, np.float64), C.c_double), r1, _p(_nz(m2, np.float64), C.c_double), r2, d,
                                                    _p(metric, C.c_double), int(kind), float(p), 1 if normalize else 0, int(keep_at_most or 0),
                                                    mn, _p(_nz(stats, np.float64), C.c_double), _p(_nz(n, np.uint32), C.c_uint32),
                                                    _p(_nz(idx, np.uint32), C.c_uint32), _p(_nz(dist, np.float64), C.c_double),
                                                    _p(_nz(z, np.float64), C.c_double)))
    return stats, n, idx, dist, z


# ------------------------------------------------------ twister generation
def ca(counts, normalize=True):
    """Correspondence analysis of a k-mers x spectra table (the R stage of src/KPopTwist:93-116).
    -> twisted (J x nd), inertia (nd), twister (nd x I, dims-major)."""
    counts = _c(counts, np.float64)
    I, J = counts.shape
    nd = min(I, J) - 1
    twisted = np.zeros((J, max(nd, 1)), dtype=np.float64)
    inertia = np.zeros(max(nd, 1), dtype=np.float64)
    twister = np.zeros((max(nd, 1), I), dtype=np.float64)
    n_out = C.c_uint32()
    check(_lib.load().kpop_ca(_p(counts, C.c_double), I, J, 1 if normalize else 0, C.byref(n_out),
                              _p(twisted, C.c_double), _p(inertia, C.c_double), _p(twister, C.c_double)))
    return twisted[:, :nd], inertia[:nd], twister[:nd]


def debug_ca():
    """what the eigen-solver did in this thread's last ca() / dev_ca() (kpop_debug_ca): the route taken and its convergence"""
    out = (C.c_uint64 * 8)()
    check(_lib.load().kpop_debug_ca(out))
    return {"blocked": int(out[0]), "on_factor": int(out[1]), "dead": int(out[2]), "kernel": int(out[3]), "sweeps": int(out[4]),
            "converged": int(out[5]), "cosine": float(np.array([out[6]], dtype=np.uint64).view(np.float64)[0]), "closing": int(out[7])}


def dev_ca_workspace_bytes(n_kmers, n_spectra):
    return int(_lib.load().kpop_dev_ca_workspace_bytes(int(n_kmers), int(n_spectra)))


def dev_ca(d_counts, n_kmers, n_spectra, d_work, d_twisted, d_inertia, d_twister, normalize=True, stream=None):
    """kpop_ca on device pointers (kpop_dev_ca); returns n_dims"""
    n_out = C.c_uint32()
    check(_lib.load().kpop_dev_ca(d_counts, int(n_kmers), int(n_spectra), 1 if normalize else 0, d_work, C.byref(n_out),
                                  d_twisted, d_inertia, d_twister, stream))
    return int(n_out.value)


# ---------------------------------------------------------- k-mer database
TRANSF_BINARY, TRANSF_POWER, TRANSF_CLR, TRANSF_PSEUDO = 0, 1, 2, 3
COMBINE_MEAN, COMBINE_MEDIAN = 0, 1
_TRANSFORMS = {"binary": TRANSF_BINARY, "power": TRANSF_POWER, "pow": TRANSF_POWER, "clr": TRANSF_CLR,
               "CLR": TRANSF_CLR, "pseudocounts": TRANSF_PSEUDO, "pseudo": TRANSF_PSEUDO}  # lib/KMerDB.ml:152-163


def _columns(columns):
    """list of int32 vectors (one per spectrum, the reference's storage) -> (kept arrays, void* array, n_rows)"""
    cols = [_c(v, np.int32) for v in columns]
    n_rows = cols[0].size if cols else 0
    for v in cols:
        if v.ndim != 1 or v.size != n_rows:
            raise ValueError("every spectrum must be a vector of n_rows counts")
    ptrs = (C.c_void_p * max(len(cols), 1))(*[v.ctypes.data for v in cols])
    return cols, ptrs, n_rows


def counter_stats(columns, threshold=1.0, power=1.0, rows=True):
    """stats_table_of_core_db (lib/KMerDB.ml:171-271) -> (col_stats n_cols x 4, row_stats n_rows x 4 | None);
    statistics are non_zero, max, sum, sum_log."""
    cols, ptrs, n_rows = _columns(columns)
    cs = np.zeros((len(cols), 4), dtype=np.float64)
    rs = np.zeros((n_rows, 4), dtype=np.float64) if rows else None
    check(_lib.load().kpop_counter_stats(ptrs, len(cols), n_rows, float(threshold), float(power),
                                         _p(_nz(cs, np.float64), C.c_double),
                                         _p(_nz(rs, np.float64), C.c_double) if rows else None))
    return cs, rs


def counter_combine(columns, sel, col_sum, criterion=COMBINE_MEAN):
    """add_combined_selected (lib/KMerDB.ml:628-736) -> (int32 combined spectrum, norm)"""
    cols, ptrs, n_rows = _columns(columns)
    sel = _c(sel, np.uint32)
    col_sum = _c(col_sum, np.float64)
    out = np.zeros(n_rows, dtype=np.int32)
    norm = C.c_double()
    check(_lib.load().kpop_counter_combine(ptrs, n_rows, _p(_nz(sel, np.uint32), C.c_uint32), sel.size,
                                           _p(_nz(col_sum, np.float64), C.c_double), int(criterion),
                                           _nz(out, np.int32).ctypes.data if n_rows else None, C.byref(norm)))
    return out, norm.value


def counter_transform(columns, col_stats, which=TRANSF_POWER, threshold=1.0, power=1.0, kmer_major=True):
    """Transformation.compute over a whole table (lib/KMerDB.ml:96-144) -> f64 [n_rows, n_cols] (kmer_major) or
    [n_cols, n_rows]"""
    cols, ptrs, n_rows = _columns(columns)
    if isinstance(which, str):
        which = _TRANSFORMS[which]
    col_stats = _c(col_stats, np.float64)
    out = np.zeros((n_rows, len(cols)) if kmer_major else (len(cols), n_rows), dtype=np.float64)
    check(_lib.load().kpop_counter_transform(ptrs, len(cols), n_rows, int(which), float(threshold), float(power),
                                             _p(_nz(col_stats, np.float64), C.c_double), 1 if kmer_major else 0,
                                             _p(_nz(out, np.float64), C.c_double)))
    return out


# rows of counter_distill's result, in the reference's order (lib/KMerDB.ml:960-965)
DISTILL_ROW_NAMES = tuple("%s%s%s" % (part, quantity, across) for quantity in ("Avg", "Var", "COV")
                          for across in ("Mean", "Median") for part in ("Inner", "Outer", "Residual"))


def counter_distill(columns, classes, n_classes=None):
    """distill_kmers (lib/KMerDB.ml:812-976; semantics declared in INTEGRATION.md) -> (out [18, n_rows] in the order of
    DISTILL_ROW_NAMES, fits [6, 2]: intercept and slope of the lines behind the six Residual rows).  classes[c] is the
    class index of spectrum c; n_classes defaults to max(classes) + 1."""
    cols, ptrs, n_rows = _columns(columns)
    classes = _c(classes, np.uint32)
    if classes.ndim != 1 or classes.size != len(cols):
        raise ValueError("one class index per spectrum")
    if n_classes is None:
        n_classes = int(classes.max()) + 1 if classes.size else 0
    out = np.zeros((len(DISTILL_ROW_NAMES), n_rows), dtype=np.float64)
    fits = np.zeros((6, 2), dtype=np.float64)
    check(_lib.load().kpop_counter_distill(ptrs, len(cols), n_rows, _p(_nz(classes, np.uint32), C.c_uint32), int(n_classes),
                                           _p(_nz(out, np.float64), C.c_double), _p(fits, C.c_double)))
    return out, fits


# ----------------------------------------------------------------- metric
def metric_compute(inertia, kind=METRIC_POWERS, power_int=1.0, threshold=1.0, power_ext=2.0):
    """Default = powers(1,1,2), bin/KPopTwistDB.ml:92."""
    inertia = _c(inertia, np.float64)
    out = np.empty(len(inertia), dtype=np.float64)
    check(_lib.load().kpop_metric_compute(int(kind), _p(_nz(inertia, np.float64), C.c_double), len(inertia),
                                          power_int, threshold, power_ext, _p(_nz(out, np.float64), C.c_double)))
    return out


# --------------------------------------------------------------- distance
def _set_geometry(m, metric, kind, p, normalize):
    """a first operand and its distance as a kpop_distance_* call takes them -> (the seven leading arguments m, rows, n_dims, metric, kind,
    p, normalize; rows)"""
    m, metric = _c(m, np.float64), _c(metric, np.float64)
    if m.ndim != 2 or m.shape[1] != len(metric):
        raise ValueError("Incompatible_geometries")  # lib/Matrix.ml:193-194
    return [_ptr(m), m.shape[0], len(metric), _ptr(metric), int(kind), float(p), 1 if normalize else 0], m.shape[0]


def _query_rows(m2, n_dims):
    """a second operand against n_dims dimensions"""
    m2 = _c(m2, np.float64)
    if m2.ndim != 2 or m2.shape[1] != n_dims:
        raise ValueError("Incompatible_geometries")  # lib/Matrix.ml:193-194
    return m2


def _summary_call(fn, lead, r1, r2, keep_at_most, max_neighbours):
    if max_neighbours is None:
        max_neighbours = r1 if not keep_at_most else min(r1, max(keep_at_most * 4, 8))
    max_neighbours = max(int(max_neighbours), 1)
    res = (np.zeros((r2, 4), dtype=np.float64), np.zeros(r2, dtype=np.uint32), np.zeros((r2, max_neighbours), dtype=np.uint32),
           np.zeros((r2, max_neighbours), dtype=np.float64), np.zeros((r2, max_neighbours), dtype=np.float64))
    check(fn(*lead, int(keep_at_most or 0), max_neighbours, *_pointers(res)))
    return res


def distance_rowwise(m1, m2, metric, kind=EUCLIDEAN, p=2.0, normalize=True):
    """-> r2 x r1 matrix, rows = m2 (the file operand), cols = m1 (the register); lib/Matrix.ml:253,264-266."""
    m1 = _c(m1, np.float64)
    m2 = _c(m2, np.float64)
    metric = _c(metric, np.float64)
    if m1.shape[1] != m2.shape[1] or m1.shape[1] != len(metric):
        raise ValueError("Incompatible_geometries")  # lib/Matrix.ml:193-194
    r1, d = m1.shape
    r2 = m2.shape[0]
    out = np.zeros((r2, r1), dtype=np.float64)
    check(_lib.load().kpop_distance_rowwise(_ptr(m1), r1, _ptr(m2), r2, d, _ptr(metric), int(kind), float(p), 1 if normalize else 0, _ptr(out)))
    return out


def distance_summary(m1, m2, metric, kind=EUCLIDEAN, p=2.0, normalize=True, keep_at_most=2,
                     max_neighbours=None):
    """-> stats (r2 x 4: mean, sd, median, MAD), n (r2), idx/dist/z (r2 x max_neighbours)."""
    m1 = _c(m1, np.float64)
    m2 = _c(m2, np.float64)
    metric = _c(metric, np.float64)
    if m1.shape[1] != m2.shape[1] or m1.shape[1] != len(metric):
        raise ValueError("Incompatible_geometries")  # lib/Matrix.ml:698-699
    r1, d = m1.shape
    r2 = m2.shape[0]
    return _summary_call(_lib.load().kpop_distance_summary, [_ptr(m1), r1, _ptr(m2), r2, d, _p(metric, C.c_double), int(kind), float(p), 1 if normalize else 0],
                         r1, r2, keep_at_most, max_neighbours)


class RefSet:
    """A first operand that stays on the device, prepared once and queried many times (kpop_refset, include/kpop_hip.h): the
    register of Matrix.get_distance_rowwise / summarize_rowwise (lib/Matrix.ml:191-266, :691-766) when it is queried repeatedly.
    Every call returns what distance_rowwise / distance_summary return for the same rows, bit for bit."""

    def __init__(self, m1, metric, kind=EUCLIDEAN, p=2.0, normalize=True, capacity=None):
        metric = _c(metric, np.float64)
        m1 = _c(m1, np.float64)
        if m1.ndim != 2:
            m1 = m1.reshape(0, len(metric))
        if m1.shape[1] != len(metric):
            raise ValueError("Incompatible_geometries")  # lib/Matrix.ml:193-194
        self._h = None
        self._keep = None
        h = C.c_void_p()
        check(_lib.load().kpop_refset_create(_p(_nz(m1, np.float64), C.c_double), m1.shape[0], m1.shape[1], _p(_nz(metric, np.float64), C.c_double),
                                             int(kind), float(p), 1 if normalize else 0, int(capacity or 0), C.byref(h)))
        self._h = h

    @classmethod
    def wrap(cls, d_m1, r1, n_dims, d_metric, kind=EUCLIDEAN, p=2.0, normalize=True, stream=0, keep=None):
        """Rows and metric already on the device (pointers), borrowed: the caller keeps them alive and unchanged (`keep`: objects
        to hold on to for the life of the set, such as the tensors the pointers came from).  No append."""
        self = cls.__new__(cls)
        self._h = None
        self._keep = keep
        h = C.c_void_p()
        check(_lib.load().kpop_dev_refset_wrap(d_m1, int(r1), int(n_dims), d_metric, int(kind), float(p), 1 if normalize else 0, stream, C.byref(h)))
        self._h = h
        return self

    @property
    def handle(self):
        return self._h

    def info(self):
        r1, d, cap, nbytes = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        check(_lib.load().kpop_refset_info(self._h, C.byref(r1), C.byref(d), C.byref(cap), C.byref(nbytes)))
        return {"r1": r1.value, "n_dims": d.value, "capacity": cap.value, "device_bytes": nbytes.value}

    def append(self, rows):
        rows = _c(rows, np.float64)
        d = self.info()["n_dims"]
        if rows.ndim != 2 or rows.shape[1] != d:
            raise ValueError("Incompatible_geometries")
        check(_lib.load().kpop_refset_append(self._h, _p(_nz(rows, np.float64), C.c_double), rows.shape[0]))

    def distance_rowwise(self, m2):
        """-> r2 x r1 matrix, as distance_rowwise(m1, m2, ...)"""
        i = self.info()
        m2 = _query_rows(m2, i["n_dims"])
        out = np.zeros((m2.shape[0], i["r1"]), dtype=np.float64)
        check(_lib.load().kpop_refset_distance_rowwise(self._h, _ptr(m2), m2.shape[0], _ptr(out)))
        return out

    def distance_summary(self, m2, keep_at_most=2, max_neighbours=None):
        """-> stats, n, idx, dist, z, as distance_summary(m1, m2, ...)"""
        i = self.info()
        m2 = _query_rows(m2, i["n_dims"])
        return _summary_call(_lib.load().kpop_refset_distance_summary, [self._h, _ptr(m2), m2.shape[0]], i["r1"], m2.shape[0], keep_at_most, max_neighbours)

    def within(self, m2, max_distance, capacity=None):
        """Every row of the set within max_distance of each row of m2 -> (offsets[r2 + 1] u64, idx u32, dist f64), CSR; a row's list
        ascending by (distance, index): the neighbour list of distance_summary (lib/Matrix.ml:632-690) cut at a distance instead of a
        count.  capacity=None: one call counts, a second fills arrays of exactly that size; a capacity that turns out too small raises
        KPopError with code ERR_CAPACITY (kpop_neighbours_within, include/kpop_hip.h)."""
        m2 = _query_rows(m2, self.info()["n_dims"])
        r2 = m2.shape[0]
        fn = _lib.load().kpop_neighbours_within
        if capacity is None:
            offsets = np.zeros(r2 + 1, dtype=np.uint64)
            check(fn(self._h, _ptr(m2), r2, float(max_distance), 0, _ptr(offsets), None, None))
            capacity = int(offsets[r2])
            if capacity == 0:  # (nothing to fill: the offsets are all there is)
                return offsets, np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float64)
        return _within_call(fn, [self._h, _ptr(m2), r2, float(max_distance)], r2, capacity)

    def clusters(self, max_distance, known=None):
        """The connected components of the graph that joins rows i < j iff d(j, i) <= max_distance -> (labels u32 [r1], n_clusters):
        labels[i] is the smallest row index of row i's component, the same bits on every run.  known: the labels an earlier call
        returned at the same max_distance, for the first len(known) rows (the set has grown since: append); pairs of two such rows are
        not examined, the result is the from-scratch one (kpop_clusters_within, include/kpop_hip.h)."""
        r1 = self.info()["r1"]
        labels = np.zeros(max(r1, 1), dtype=np.uint32)
        known_rows = 0
        if known is not None:
            known = np.asarray(known)
            if known.ndim != 1 or len(known) > r1:
                raise ValueError("known: the labels of the first rows of the set, at most %d" % r1)
            known_rows = len(known)
            labels[:known_rows] = known
        return _clusters_call(_lib.load().kpop_clusters_within, [self._h, float(max_distance), known_rows], r1, labels)

    def representatives(self, max_distance, known=None):
        """The greedy cover of the set in row order -> (rep_of u32 [r1], rep_dist f64 [r1], n_reps): row i is a representative iff no
        representative below it lies within max_distance; rep_of[i] is i for a representative and otherwise the nearest representative
        BELOW row i (ties to the smaller index), rep_dist[i] its distance.  The same bits on every run; the result depends on the row
        order, and its first n rows on no later row.  known: the rep_of an earlier call returned at the same max_distance for the first
        len(known) rows (the set has grown since: append), or the whole tuple it returned; those rows are not examined against each
        other, the result is the from-scratch one.  rep_dist of the known rows is not computed again: it is taken from the tuple, and
        NaN where only rep_of was given (kpop_representatives_within, include/kpop_hip.h)."""
        r1 = self.info()["r1"]
        rep_of = np.zeros(max(r1, 1), dtype=np.uint32)
        rep_dist = np.zeros(max(r1, 1), dtype=np.float64)
        known_rows = 0
        if known is not None:
            known_dist = None
            if isinstance(known, tuple):
                known, known_dist = known[0], np.asarray(known[1])
            known = np.asarray(known)
            if known.ndim != 1 or len(known) > r1 or (known_dist is not None and known_dist.shape != known.shape):
                raise ValueError("known: the rep_of of the first rows of the set, at most %d" % r1)
            known_rows = len(known)
            rep_of[:known_rows] = known
            rep_dist[:known_rows] = np.nan if known_dist is None else known_dist
        return _representatives_call(_lib.load().kpop_representatives_within, [self._h, float(max_distance), known_rows], r1, rep_of, rep_dist)

    def dbscan(self, eps, min_pts):
        """DBSCAN of the set -> (labels u32 [r1], core_of u32 [r1], degree u32 [r1], counts u32 [3]).  degree[i] = 1 + the rows within
        eps of row i; row i is a core row iff degree[i] >= min_pts; the clusters are the connected components of the core rows, a core
        row's label the smallest core row index of its component and core_of[i] = i; a row that is not core and has a core row within
        eps is a border row: core_of[i] its nearest core row (ties to the smaller row index), labels[i] that row's label, and it joins
        nothing; every other row is noise: labels[i] = core_of[i] = NOISE.  counts: the clusters, the core rows, the noise rows.  The
        same bits on every run.  No earlier result is a valid start: after append the call is made again in full (kpop_dbscan,
        include/kpop_hip.h)."""
        return _dbscan_call(_lib.load().kpop_dbscan, [self._h, float(eps), _min_pts(min_pts)], self.info()["r1"])

    def silhouette(self, class_of, n_classes=None):
        """The silhouette and the medoids of the set under a labelling -> Silhouette(own_mean f64 [r1], other_mean f64 [r1], other_class
        u32 [r1], silhouette f64 [r1], class_rows u32 [n_classes], medoid u32 [n_classes], medoid_mean f64 [n_classes]).  class_of[i] is a
        class in [0, n_classes) or NO_CLASS (== NOISE): the row is left out of every sum and gets NaN, NaN, NO_CLASS, NaN.  own_mean: the
        mean distance to the other rows of the row's class (+0 alone); other_mean, other_class: the least mean distance to another class
        and that class (ties to the smaller class); silhouette: (other - own) / max(own, other), +0 for a row alone in its class; medoid:
        the member of a class with the least own_mean (ties to the smaller row), medoid_mean that mean.  The same bits on every run and
        under any renumbering of the classes.  n_classes None: one more than the largest class.  No earlier result is a valid start:
        after append the call is made again in full (kpop_silhouette, include/kpop_hip.h)."""
        return _silhouette_call(_lib.load().kpop_silhouette, [self._h], self.info()["r1"], class_of, n_classes)

    def class_linkage(self, class_of, n_classes=None):
        """The distances between every two classes of the set under a labelling -> ClassLinkage(class_rows u32 [n_classes], mean_dist,
        min_dist, max_dist f64 [n_classes, n_classes], min_i, min_j u32 [n_classes, n_classes]).  class_of[i] is a class in [0, n_classes)
        or NO_CLASS: the row is left out of everything.  Over the pairs of one row of a and one row of b (on the diagonal: the pairs i < j
        of two rows of a): the mean, the least and the greatest distance, and the two rows min_i < min_j of the least pair under
        (d, i, j); no pair (an empty class, the diagonal of a class of one row): NaN and NO_CLASS.  max_dist[a, a] is a class's diameter.
        All five tables are symmetric bit for bit; the same bits on every run; under a renumbering of the classes min_dist, max_dist,
        min_i and min_j are permuted and nothing else, mean_dist stays within its rounding.  n_classes None: one more than the largest
        class; at most 4,096.  No earlier result is a valid start: after append the call is made again in full (kpop_class_linkage,
        include/kpop_hip.h).  class_tree makes the classes' tree of a table."""
        return _class_linkage_call(_lib.load().kpop_class_linkage, [self._h], self.info()["r1"], class_of, n_classes)

    def farthest_first(self, max_picks=None, cover_radius=-1.0, seeds=None):
        """The farthest-first traversal of the set -> FarthestFirst(pick u32 [n], pick_radius f64 [n], pick_parent u32 [n], rep_of u32 [r1],
        rep_dist f64 [r1], n_passes).  Every row has a cover distance (+inf at first) and a cover row (NOISE at first); a pick lowers the
        cover distance of every unpicked row that lies strictly nearer to it (a NaN covers nothing, a tie keeps the earlier pick).  The
        seeds are picked first, in their order; every later pick is the unpicked row with the greatest cover distance, ties to the smaller
        row (without seeds the first pick is row 0).  It stops at max_picks picks (None: every row), or before a pick that is not a seed
        and whose cover distance is <= cover_radius (negative: never).  pick_radius[t], pick_parent[t]: the cover distance and row of
        pick t when it was picked; rep_of, rep_dist: a picked row itself at +0, any other row its cover row and distance.  Every prefix
        of the picks is a cover of the set at the radius written beside the next pick; seeds=pick[:k] of an earlier run, or that run's
        whole tuple, reproduces it and goes on -- also after append.  The same bits on every run; n_passes is a fact about the run
        (kpop_farthest_first, include/kpop_hip.h)."""
        return _farthest_first_call(_lib.load().kpop_farthest_first, [self._h], self.info()["r1"], max_picks, cover_radius, seeds)

    def kmedoids(self, medoids, max_iter=100):
        """Alternating k-medoids (Voronoi iteration) on the set -> KMedoids(medoid u32 [k], class_of u32 [r1], dist f64 [r1], own_mean f64
        [r1], class_rows u32 [k], cost f64 [n_iter + 1], n_iter, converged).  medoids: the k distinct rows to start from -- an index array;
        a FarthestFirst tuple, whose picks are used; or an int k, meaning self.farthest_first(max_picks=k).pick: the k-centre seeding, a
        2-approximation of the best k centres and the same rows on every run.  Assignment: a medoid has its own position as class and dist
        +0, every other row the nearest medoid (ties to the earlier position; a row with no distance that is a number is left out: NO_CLASS,
        +inf, NaN).  Update: a class's new medoid is its member with the least own_mean (ties to the smaller row), own_mean being
        silhouette's for class_of, bit for bit.  The rounds stop when no medoid moves (converged) or after max_iter re-assignments;
        max_iter=0 is the plain assignment to the given rows.  What is returned is consistent: class_of / dist are the assignment to
        medoid, own_mean and class_rows are of that labelling; cost[t] is the sum of dist after t re-assignments.  medoids=an earlier run's
        medoid goes on where that run stopped -- also after append.  The same bits on every run (kpop_kmedoids, include/kpop_hip.h)."""
        if isinstance(medoids, (int, np.integer)) and not isinstance(medoids, bool):
            medoids = self.farthest_first(max_picks=int(medoids)).pick
        return _kmedoids_call(_lib.load().kpop_kmedoids, [self._h], self.info()["r1"], medoids, max_iter)

    def lof(self, k=20):
        """The local outlier factor of every row of the set against the other rows -> Lof(kdist f64 [r1], n_neigh u32 [r1], lrd f64 [r1],
        lof f64 [r1]).  kdist: core_distances(k + 1), bit for bit; the neighbourhood of row j is every other row within kdist[j], the whole
        tie group of the k-th distance; lrd = n_neigh / the sum of max(d(j, i), kdist[i]) over it; lof = (the mean of lrd[i] over it) /
        lrd[j]: about 1 inside a lineage, well above 1 for a row that belongs nowhere.  A clump of more than k copies has lrd +inf and lof
        1.0 (inf / inf is 1.0), a row beside it lof +inf; a row with fewer than k numeric distances gets NaN, 0, NaN, NaN.  k in 1 .. 128.
        The same bits on every run.  No earlier result is a valid start: after append the call is made again in full (kpop_lof,
        include/kpop_hip.h)."""
        return _lof_call(_lib.load().kpop_lof, [self._h, _min_pts(k)], self.info()["r1"])

    def lof_score(self, m2, k, kdist, lrd):
        """The novelty score of the rows of m2 against the set as it stands -> Lof, one entry a row of m2.  kdist, lrd: what self.lof(k)
        returned (the arrays or the whole tuple's fields), at the same k.  Nothing is left out: a query equal to a set row has that row at
        distance 0.  The set's rows are not re-scored (kpop_lof_score, include/kpop_hip.h)."""
        i = self.info()
        m2 = _query_rows(m2, i["n_dims"])
        kdist, lrd = _c(kdist, np.float64), _c(lrd, np.float64)
        if kdist.shape != (i["r1"],) or lrd.shape != (i["r1"],):
            raise ValueError("kdist, lrd: the set form's arrays, one entry for each of the set's %d rows" % i["r1"])
        return _lof_call(_lib.load().kpop_lof_score, [self._h, _min_pts(k), _ptr(kdist), _ptr(lrd), _ptr(m2), m2.shape[0]], m2.shape[0])

    def density_peaks(self, eps=None, density=None, min_density=float("-inf"), min_delta=None):
        """Density peaks (Rodriguez & Laio 2014): for every row the distance delta to, and the index parent of, the nearest row that ranks
        above it -> DensityPeaks(density f64 [r1], delta f64 [r1], parent u32 [r1], labels u32 [r1], counts u32 [3]).  density: one score a
        row (assembly quality, lof().lrd, ...), or None: dbscan(eps, .)'s degree as doubles.  Row i ranks above row j iff its density is
        higher, or equal and i < j; a row without anybody above it at a numeric distance is a ROOT (parent itself, delta +inf); a row
        whose density is a NaN is left out (delta NaN, parent and label NOISE).  min_delta given: a row is a CENTRE iff it is a root or
        delta > min_delta and density >= min_density; labels[j] is the centre's row index that j reaches along its parents, counts =
        (centres, roots, rows left out).  min_delta None: labels and counts are None -- look at (density, delta), then density_peaks_cut.
        The same bits on every run.  After append the call is made again in full (kpop_density_peaks, include/kpop_hip.h)."""
        return _density_peaks_call(_lib.load().kpop_density_peaks, [self._h], self.info()["r1"], eps, density, min_density, min_delta)

    def spanning_forest(self, max_distance=float("inf")):
        """The single-linkage tree of the set: the minimum spanning forest of the graph that joins rows i < j iff d(j, i) <= max_distance,
        under the order (d, i, j) -> (edge_i u32, edge_j u32, edge_dist f64, labels u32 [r1]).  The order is strict, so the forest is
        unique: the same bits on every run, the edges listed ascending.  labels are clusters(max_distance)'s; forest_cut of the edges
        at any T <= max_distance gives clusters(T) (kpop_spanning_forest, include/kpop_hip.h)."""
        return _forest_call(_lib.load().kpop_spanning_forest, [self._h, float(max_distance)], self.info()["r1"], core=False)

    def core_distances(self, min_pts):
        """Every row's core distance -> f64 [r1]: +0 for min_pts = 1, otherwise the distance to its (min_pts - 1)-th nearest OTHER row
        (NaN distances are not counted, +inf is), NaN where a row has fewer.  core_distances(min_pts) <= eps iff dbscan(eps, min_pts)'s
        degree >= min_pts.  min_pts in 1 .. 129 (kpop_core_distances, include/kpop_hip.h)."""
        r1 = self.info()["r1"]
        core = np.zeros(max(r1, 1), dtype=np.float64)
        check(_lib.load().kpop_core_distances(self._h, _min_pts(min_pts), _p(core, C.c_double)))
        return core[:r1]

    def reachability_forest(self, min_pts, max_distance=float("inf")):
        """The mutual-reachability forest of the set: DBSCAN at every radius -> (edge_i u32, edge_j u32, edge_dist f64, core_dist f64 [r1],
        labels u32 [r1]).  An edge i < j weighs max(d(i, j), core_dist[i], core_dist[j]) and exists iff the three are numbers and the
        weight is within max_distance; the result is the minimum spanning forest under the strict order (weight, i, j): unique, the same
        bits on every run, the edges listed ascending; labels the smallest row index of each component.  min_pts = 1 gives
        spanning_forest(max_distance).  reachability_cut of the edges at any T <= max_distance gives dbscan(T, min_pts)'s labels on the
        core rows, every other row alone (DBSCAN*: border rows are not attached).  No earlier result is a valid start after append
        (kpop_reachability_tree, include/kpop_hip.h)."""
        return _forest_call(_lib.load().kpop_reachability_tree, [self._h, _min_pts(min_pts), float(max_distance)], self.info()["r1"], core=True)

    def knn_vote(self, m2, class_of, k=5, n_classes=None):
        """The k-NN classifier of the reference's README on the device -> (cls u32, votes u32, n u32, first f64), one entry a row of m2.
        class_of: a class in [0, n_classes) for every row of the set (n_classes=None: the largest class + 1).  A row's list is its k
        nearest rows of the set by (distance, index) plus every further row at the k-th distance (lib/Matrix.ml:641-650); n its length,
        cls the class with the most members in it -- among equals the one whose nearest member comes first --, votes its count, first that
        member's distance.  An empty list gives NO_CLASS, 0, 0, NaN (kpop_knn_vote, include/kpop_hip.h)."""
        i = self.info()
        m2 = _query_rows(m2, i["n_dims"])
        class_of, n_classes = _classes(class_of, i["r1"], n_classes)
        return _knn_call(_lib.load().kpop_knn_vote, [self._h, _ptr(class_of), n_classes, _ptr(m2), m2.shape[0], int(k)], (m2.shape[0],))

    def knn_vote_ks(self, m2, class_of, ks, n_classes=None):
        """knn_vote at every k of ks (strictly ascending, each in 1..128, at most 32 of them) from ONE pass over the pairs ->
        (cls, votes, n, first), each [len(ks)][rows of m2]; slice t is knn_vote(m2, class_of, k=ks[t]) bit for bit (kpop_knn_ks_vote,
        include/kpop_hip.h)."""
        i = self.info()
        m2 = _query_rows(m2, i["n_dims"])
        class_of, n_classes = _classes(class_of, i["r1"], n_classes)
        ks = _ks(ks)
        return _knn_call(_lib.load().kpop_knn_ks_vote, [self._h, _ptr(class_of), n_classes, _ptr(m2), m2.shape[0], _ptr(ks), len(ks)], (len(ks), m2.shape[0]))

    def knn_validate(self, class_of, ks=(1, 3, 5), group_of=None, n_classes=None):
        """The set as its own test: every row classified by its neighbours among the OTHER rows, at every k of ks, from one pass over the
        pairs -> (cls, votes, n, first, correct): the first four [len(ks)][r1] as knn_vote_ks gives them, correct[t] (u64) the rows whose
        class at ks[t] is their own.  group_of=None leaves out the row itself (leave-one-out); otherwise every row of the row's group is
        left out of its list (the fold of a cross-validation, an outbreak) -- by index or group, never by distance: a duplicate in another
        group stays.  A row with no list gives NO_CLASS, 0, 0, NaN and is never correct (kpop_knn_validate, include/kpop_hip.h)."""
        return _knn_validate_call(_lib.load().kpop_knn_validate, [self._h], self.info()["r1"], class_of, n_classes, group_of, ks)

    def free(self):
        if self._h is not None and self._h.value:
            check(_lib.load().kpop_refset_free(self._h))
            self._h = None
            self._keep = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def embeddings(m, metric, kind=EUCLIDEAN, p=2.0, normalize=True):
    """Base.get_embeddings (lib/Matrix.ml:78-128): principal coordinates from twisted rows."""
    m = _c(m, np.float64)
    metric = _c(metric, np.float64)
    out = np.zeros_like(m)
    check(_lib.load().kpop_embeddings(_p(_nz(m, np.float64), C.c_double), m.shape[0], m.shape[1], _p(metric, C.c_double), int(kind),
                                      float(p), 1 if normalize else 0, _p(_nz(out, np.float64), C.c_double)))
    return out


def splits_gaps(emb, max_splits=10000):
    """Matrix.get_splits ... Gaps (lib/Matrix.ml:524-600) -> (gap, dim, idx) of the largest gaps and perm [n_dims, rows];
    split s = perm[dim[s], :idx[s] + 1]"""
    emb = _c(emb, np.float64)
    rows, d = emb.shape
    gap = np.zeros(max(max_splits, 1), dtype=np.float64)
    dim = np.zeros(max(max_splits, 1), dtype=np.uint32)
    idx = np.zeros(max(max_splits, 1), dtype=np.uint32)
    perm = np.zeros((max(d, 1), max(rows, 1)), dtype=np.uint32)
    n = C.c_uint32()
    check(_lib.load().kpop_splits_gaps(_p(_nz(emb, np.float64), C.c_double), rows, d, int(max_splits), C.byref(n), _p(gap, C.c_double),
                                       _p(dim, C.c_uint32), _p(idx, C.c_uint32), _p(perm, C.c_uint32)))
    return gap[:n.value], dim[:n.value], idx[:n.value], perm[:d, :rows]


def summarize_distances(dist, keep_at_most=2, max_neighbours=None):
    """Matrix.summarize_distance (lib/Matrix.ml:767-810) on an existing r2 x r1 distance matrix."""
    dist = _c(dist, np.float64)
    r2, r1 = dist.shape
    return _summary_call(_lib.load().kpop_summarize_distances, [_ptr(dist), r2, r1], r1, r2, keep_at_most, max_neighbours)


# ------------------------------------------------- device-resident entry points
def dev_synth_reads(seed, n_reads, read_len, d_bases, d_offsets, first_read=0, stream=0):
    check(_lib.load().kpop_dev_synth_reads(int(seed), int(n_reads), int(read_len), int(first_read), d_bases,
                                           d_offsets, stream))


def dev_count_reads_scratch_bytes(n_reads, max_len, k):
    return int(_lib.load().kpop_dev_count_reads_scratch_bytes(int(n_reads), int(max_len), int(k)))


def dev_count_reads(d_bases, d_offsets, n_reads, max_len, k, d_scratch, d_out_hash, d_out_count, d_out_offsets,
                    content=DNA_DS, stream=0):
    check(_lib.load().kpop_dev_count_reads(d_bases, d_offsets, int(n_reads), int(max_len), int(k), int(content), d_scratch,
                                           d_out_hash, d_out_count, d_out_offsets, stream))


def dev_count_twist(tw, d_bases, d_offsets, n_reads, n_bases, max_len, d_out, content=DNA_DS, normalize=True,
                    stream=0):
    check(_lib.load().kpop_dev_count_twist(tw.handle, d_bases, d_offsets, int(n_reads), int(n_bases), int(max_len),
                                           int(content), 1 if normalize else 0, d_out, stream))


def dev_twist(tw, d_hash, d_value, d_offsets, n_spectra, max_lines, d_out, normalize=True, stream=0):
    check(_lib.load().kpop_dev_twist(tw.handle, d_hash, d_value, d_offsets, int(n_spectra), int(max_lines),
                                     1 if normalize else 0, d_out, stream))


def dev_twist_dense_workspace_bytes(tw, n_spectra):
    return int(_lib.load().kpop_dev_twist_dense_workspace_bytes(tw.handle, int(n_spectra)))


def dev_twist_dense(tw, d_hash, d_value, d_offsets, n_spectra, d_work, d_out, normalize=True, stream=0):
    """the twist as X[n_spectra x n_kmers] * T on the f64 matrix cores (kpop_dev_twist_dense)"""
    check(_lib.load().kpop_dev_twist_dense(tw.handle, d_hash, d_value, d_offsets, int(n_spectra), 1 if normalize else 0, d_work,
                                           d_out, stream))


def dev_count_twist_dense_workspace_bytes(tw, n_reads):
    return int(_lib.load().kpop_dev_count_twist_dense_workspace_bytes(tw.handle, int(n_reads)))


def dev_count_twist_dense(tw, d_bases, d_offsets, n_reads, d_work, d_out, content=DNA_DS, normalize=True, stream=0):
    """sequences -> twisted rows through the dense u32 image of their counts and the f64 matrix cores (small k, assemblies)"""
    check(_lib.load().kpop_dev_count_twist_dense(tw.handle, d_bases, d_offsets, int(n_reads), int(content), 1 if normalize else 0, d_work,
                                                 d_out, stream))


def dev_twist_dense_sorted(tw, d_hash, d_value, d_offsets, n_spectra, d_work, d_out, normalize=True, stream=0):
    """kpop_dev_twist_dense_sorted: lines ascending by hash, densified inside the contraction (no X in HBM)"""
    check(_lib.load().kpop_dev_twist_dense_sorted(tw.handle, d_hash, d_value, d_offsets, int(n_spectra), 1 if normalize else 0, d_work,
                                                  d_out, stream))


def dev_distance_workspace_bytes(r1, r2, n_dims):
    return int(_lib.load().kpop_dev_distance_workspace_bytes(int(r1), int(r2), int(n_dims)))


def dev_distance_rowwise(d_m1, r1, d_m2, r2, n_dims, d_metric, d_work, d_out, kind=EUCLIDEAN, p=2.0,
                         normalize=True, stream=0):
    check(_lib.load().kpop_dev_distance_rowwise(d_m1, int(r1), d_m2, int(r2), int(n_dims), d_metric, int(kind),
                                                float(p), 1 if normalize else 0, d_work, d_out, stream))


def dev_distance_summary(d_m1, r1, d_m2, r2, n_dims, d_metric, d_work, d_stats, d_n, d_idx, d_dist, d_z,
                         keep_at_most=2, max_neighbours=8, kind=EUCLIDEAN, p=2.0, normalize=True, stream=0):
    check(_lib.load().kpop_dev_distance_summary(d_m1, int(r1), d_m2, int(r2), int(n_dims), d_metric, int(kind),
                                                float(p), 1 if normalize else 0, int(keep_at_most or 0),
                                                int(max_neighbours), d_work, d_stats, d_n, d_idx, d_dist, d_z, stream))


def dev_refset_workspace_bytes(rs, r2):
    """the size of d_work for r2 query rows against the set: the query side alone, whatever the set's size"""
    return int(_lib.load().kpop_dev_refset_workspace_bytes(rs.handle, int(r2)))


def dev_refset_distance_rowwise(rs, d_m2, r2, d_work, d_out, stream=0):
    check(_lib.load().kpop_dev_refset_distance_rowwise(rs.handle, d_m2, int(r2), d_work, d_out, stream))


def dev_refset_distance_summary(rs, d_m2, r2, d_work, d_stats, d_n, d_idx, d_dist, d_z, keep_at_most=2, max_neighbours=8, stream=0):
    check(_lib.load().kpop_dev_refset_distance_summary(rs.handle, d_m2, int(r2), int(keep_at_most or 0), int(max_neighbours), d_work, d_stats, d_n,
                                                       d_idx, d_dist, d_z, stream))


NO_CLASS = 0xFFFFFFFF  # KPOP_NO_CLASS: the class of a query row with an empty list


def _classes(class_of, r1, n_classes):
    """the labels of a set's rows as the C ABI takes them"""
    class_of = np.asarray(class_of)
    if class_of.ndim != 1 or len(class_of) != r1:
        raise ValueError("class_of: one class for each of the set's %d rows" % r1)
    if len(class_of) and (class_of.min() < 0 or class_of.max() > 0xFFFFFFFF):
        raise ValueError("class_of: classes are uint32")
    class_of = _c(class_of, np.uint32)
    if n_classes is None:
        n_classes = int(class_of.max()) + 1 if len(class_of) else 1
    return class_of, int(n_classes)


def dev_knn_vote_workspace_bytes(rs, r2, k, n_classes):
    """the size of d_work for dev_knn_vote: by r2, k and n_classes; it does not grow with the set"""
    return int(_lib.load().kpop_dev_knn_vote_workspace_bytes(rs.handle, int(r2), int(k), int(n_classes)))


def dev_knn_vote(rs, d_class_of, n_classes, d_m2, r2, k, d_work, d_cls, d_votes, d_n, d_first=None, stream=0):
    """enqueue only: d_cls / d_votes / d_n (u32 [r2]) and d_first (f64 [r2], or None) as RefSet.knn_vote returns them; d_class_of
    (u32, one a row of the set) is trusted"""
    check(_lib.load().kpop_dev_knn_vote(rs.handle, d_class_of, int(n_classes), d_m2, int(r2), int(k), d_work, d_cls, d_votes, d_n, d_first, stream))


def _knn_call(fn, lead, shape, *more):
    """cls, votes, n, first of a vote: one entry a query row, or one a k and query row.  more: the outputs that follow them"""
    res = (np.zeros(shape, dtype=np.uint32), np.zeros(shape, dtype=np.uint32), np.zeros(shape, dtype=np.uint32), np.zeros(shape, dtype=np.float64))
    check(fn(*lead, *_pointers(res + more)))
    return res


def distance_knn_vote(m1, class_of, m2, metric, k=5, kind=EUCLIDEAN, p=2.0, normalize=True, n_classes=None):
    """RefSet(m1, ...).knn_vote(m2, class_of, k) without keeping the set: one call of kpop_distance_knn_vote"""
    lead, r1 = _set_geometry(m1, metric, kind, p, normalize)
    m2 = _query_rows(m2, lead[2])
    class_of, n_classes = _classes(class_of, r1, n_classes)
    return _knn_call(_lib.load().kpop_distance_knn_vote, lead[:2] + [_ptr(class_of), n_classes, _ptr(m2), m2.shape[0]] + lead[2:] + [int(k)], (m2.shape[0],))


def _ks(ks):
    """a ladder of k as the C ABI takes it (the library checks it: strictly ascending, 1..128, at most 32)"""
    ks = np.asarray(ks)
    if ks.ndim != 1 or (len(ks) and (ks.min() < 0 or ks.max() > 0xFFFFFFFF)):
        raise ValueError("ks: a list of k, each a uint32")
    return _c(ks, np.uint32)


def _groups(group_of, r1):
    if group_of is None:
        return None
    group_of = np.asarray(group_of)
    if group_of.ndim != 1 or len(group_of) != r1:
        raise ValueError("group_of: one group for each of the set's %d rows" % r1)
    if len(group_of) and (group_of.min() < 0 or group_of.max() > 0xFFFFFFFF):
        raise ValueError("group_of: groups are uint32")
    return _c(group_of, np.uint32)


def dev_knn_vote_ks_workspace_bytes(rs, r2, k_max, n_classes):
    """the size of d_work for dev_knn_vote_ks: dev_knn_vote's at the largest k; it grows neither with the set nor with len(ks)"""
    return int(_lib.load().kpop_dev_knn_ks_vote_workspace_bytes(rs.handle, int(r2), int(k_max), int(n_classes)))


def dev_knn_vote_ks(rs, d_class_of, n_classes, d_m2, r2, ks, d_work, d_cls, d_votes, d_n, d_first=None, stream=0):
    """enqueue only: d_cls / d_votes / d_n (u32 [len(ks)][r2]) and d_first (f64, or None) as RefSet.knn_vote_ks returns them; ks is a
    host sequence (it goes to the kernels by value), d_class_of (u32, one a row of the set) is trusted"""
    ks = _ks(ks)
    check(_lib.load().kpop_dev_knn_ks_vote(rs.handle, d_class_of, int(n_classes), d_m2, int(r2), _p(_nz(ks, np.uint32), C.c_uint32), len(ks), d_work, d_cls,
                                           d_votes, d_n, d_first, stream))


def dev_knn_validate_workspace_bytes(rs, n_rows, k_max, n_classes):
    """the size of d_work for dev_knn_validate over n_rows rows: it grows neither with the set nor with len(ks)"""
    return int(_lib.load().kpop_dev_knn_validate_workspace_bytes(rs.handle, int(n_rows), int(k_max), int(n_classes)))


def dev_knn_validate(rs, d_class_of, n_classes, d_group_of, first_row, n_rows, ks, d_work, d_cls, d_votes, d_n, d_first, d_correct, stream=0):
    """enqueue only: rows first_row .. first_row + n_rows of the set against the whole set; d_cls / d_votes / d_n (u32 [len(ks)][n_rows]),
    d_first (f64, or None) and d_correct (u64 [len(ks)], written for this range, not accumulated) as RefSet.knn_validate returns them;
    d_group_of (u32, one a row of the set) or None: leave-one-out; ks is a host sequence"""
    ks = _ks(ks)
    check(_lib.load().kpop_dev_knn_validate(rs.handle, d_class_of, int(n_classes), d_group_of, int(first_row), int(n_rows), _p(_nz(ks, np.uint32), C.c_uint32),
                                            len(ks), d_work, d_cls, d_votes, d_n, d_first, d_correct, stream))


def _knn_validate_call(fn, lead, r1, class_of, n_classes, group_of, ks):
    class_of, n_classes = _classes(class_of, r1, n_classes)
    group_of = _groups(group_of, r1)
    ks = _ks(ks)
    correct = np.zeros(max(len(ks), 1), dtype=np.uint64)
    res = _knn_call(fn, lead + [_ptr(class_of), n_classes, None if group_of is None else _ptr(group_of), _ptr(ks), len(ks)], (len(ks), r1), correct)
    return res + (correct[:len(ks)],)


def distance_knn_validate(m, class_of, metric, ks=(1, 3, 5), group_of=None, kind=EUCLIDEAN, p=2.0, normalize=True, n_classes=None):
    """RefSet(m, ...).knn_validate(class_of, ks, group_of) without keeping the set: one call of kpop_distance_knn_validate"""
    lead, r1 = _set_geometry(m, metric, kind, p, normalize)
    return _knn_validate_call(_lib.load().kpop_distance_knn_validate, lead, r1, class_of, n_classes, group_of, ks)


def confusion_matrix(class_of, predicted, n_classes):
    """host bookkeeping (numpy): M[c][q] = the rows of class c that were given class q, with one more column, M[c][n_classes], for
    NO_CLASS; the diagonal's sum is knn_validate's `correct` of that slice"""
    class_of, predicted = np.asarray(class_of, dtype=np.int64), np.asarray(predicted, dtype=np.int64)
    n_classes = int(n_classes)
    if class_of.shape != predicted.shape or class_of.ndim != 1:
        raise ValueError("confusion_matrix: one prediction for each row")
    if len(class_of) and (class_of.min() < 0 or class_of.max() >= n_classes):
        raise ValueError("confusion_matrix: a class is not below n_classes")
    col = np.where(predicted == NO_CLASS, n_classes, predicted)
    if len(col) and (col.min() < 0 or col.max() > n_classes):
        raise ValueError("confusion_matrix: a prediction is neither a class nor NO_CLASS")
    out = np.zeros((n_classes, n_classes + 1), dtype=np.int64)
    np.add.at(out, (class_of, col), 1)
    return out


def dev_neighbours_within_workspace_bytes(rs, r2, capacity):
    """the size of d_work for r2 query rows and lists of `capacity` entries in all: it does not grow with the set"""
    return int(_lib.load().kpop_dev_neighbours_within_workspace_bytes(rs.handle, int(r2), int(capacity)))


def dev_neighbours_within(rs, d_m2, r2, max_distance, capacity, d_work, d_offsets, d_idx, d_dist, stream=0):
    """enqueue only: d_offsets[r2 + 1] (u64) is always complete, d_idx (u32) / d_dist (f64) are written when d_offsets[r2] <= capacity;
    d_idx = d_dist = None counts only"""
    check(_lib.load().kpop_dev_neighbours_within(rs.handle, d_m2, int(r2), float(max_distance), int(capacity), d_work, d_offsets, d_idx, d_dist, stream))


def _within_call(fn, lead, r2, capacity):
    capacity = int(capacity)
    offsets = np.zeros(r2 + 1, dtype=np.uint64)
    idx = np.zeros(max(capacity, 1), dtype=np.uint32)
    dist = np.zeros(max(capacity, 1), dtype=np.float64)
    check(fn(*lead, capacity, _ptr(offsets), _ptr(idx), _ptr(dist)))
    total = int(offsets[r2])
    return offsets, idx[:total], dist[:total]


def distance_within(m1, m2, metric, max_distance, kind=EUCLIDEAN, p=2.0, normalize=True, capacity=None):
    """RefSet(m1, ...).within(m2, max_distance) without keeping the set; with a capacity, one call of kpop_distance_within"""
    if capacity is None:
        rs = RefSet(_c(m1, np.float64), _c(metric, np.float64), kind=kind, p=p, normalize=normalize)
        try:
            return rs.within(m2, max_distance)
        finally:
            rs.free()
    lead, r1 = _set_geometry(m1, metric, kind, p, normalize)
    m2 = _query_rows(m2, lead[2])
    return _within_call(_lib.load().kpop_distance_within, lead[:2] + [_ptr(m2), m2.shape[0]] + lead[2:] + [float(max_distance)], m2.shape[0], capacity)


def dev_clusters_within_workspace_bytes(rs):
    """the size of d_work for dev_clusters_within: a constant, whatever the set's size"""
    return int(_lib.load().kpop_dev_clusters_within_workspace_bytes(rs.handle))


def dev_clusters_within(rs, max_distance, d_work, d_labels, d_n_clusters, known_rows=0, stream=0):
    """enqueue only: d_labels[r1] (u32; the first known_rows an earlier result at the same max_distance, trusted), d_n_clusters[1] (u32)"""
    check(_lib.load().kpop_dev_clusters_within(rs.handle, float(max_distance), int(known_rows), d_work, d_labels, d_n_clusters, stream))


def _clusters_call(fn, lead, r1, labels):
    n = C.c_uint32()
    check(fn(*lead, _ptr(labels), C.byref(n)))
    return labels[:r1], int(n.value)


def distance_clusters(m, metric, kind=EUCLIDEAN, p=2.0, normalize=True, max_distance=0.0):
    """RefSet(m, ...).clusters(max_distance) without keeping the set: one call of kpop_distance_clusters -> (labels u32 [rows], n_clusters)"""
    lead, rows = _set_geometry(m, metric, kind, p, normalize)
    return _clusters_call(_lib.load().kpop_distance_clusters, lead + [float(max_distance)], rows, np.zeros(max(rows, 1), dtype=np.uint32))


def dev_representatives_within_workspace_bytes(rs):
    """the size of d_work for dev_representatives_within, for the set's r1 at the time of the call"""
    return int(_lib.load().kpop_dev_representatives_within_workspace_bytes(rs.handle))


def dev_representatives_within(rs, max_distance, d_work, d_rep_of, d_rep_dist, d_n_reps, known_rows=0, stream=0):
    """enqueue only: d_rep_of[r1] (u32; the first known_rows an earlier result at the same max_distance, trusted), d_rep_dist[r1] (f64, or
    None), d_n_reps[1] (u32)"""
    check(_lib.load().kpop_dev_representatives_within(rs.handle, float(max_distance), int(known_rows), d_work, d_rep_of, d_rep_dist, d_n_reps, stream))


def _representatives_call(fn, lead, r1, rep_of, rep_dist):
    n = C.c_uint32()
    check(fn(*lead, _ptr(rep_of), _ptr(rep_dist), C.byref(n)))
    return rep_of[:r1], rep_dist[:r1], int(n.value)


def distance_representatives(m, metric, kind=EUCLIDEAN, p=2.0, normalize=True, max_distance=0.0):
    """RefSet(m, ...).representatives(max_distance) without keeping the set: one call of kpop_distance_representatives ->
    (rep_of u32 [rows], rep_dist f64 [rows], n_reps)"""
    lead, rows = _set_geometry(m, metric, kind, p, normalize)
    return _representatives_call(_lib.load().kpop_distance_representatives, lead + [float(max_distance)], rows, np.zeros(max(rows, 1), dtype=np.uint32),
                                 np.zeros(max(rows, 1), dtype=np.float64))


NOISE = 0xFFFFFFFF  # KPOP_NOISE: the label and the core row of a row that is neither a core row nor within eps of one


def _min_pts(min_pts):
    """a count a uint32 holds (zero goes through: the library says what is wrong with it)"""
    min_pts = int(min_pts)
    if not 0 <= min_pts <= 0xFFFFFFFF:
        raise ValueError("min_pts: a count of rows")
    return min_pts


def dev_dbscan_workspace_bytes(rs):
    """the size of d_work for dev_dbscan, for the set's r1 at the time of the call"""
    return int(_lib.load().kpop_dev_dbscan_workspace_bytes(rs.handle))


def dev_dbscan(rs, eps, min_pts, d_work, d_labels, d_core_of, d_degree, d_counts, stream=0):
    """enqueue only: d_labels[r1] (u32), d_core_of[r1] (u32, or None), d_degree[r1] (u32, or None), d_counts[3] (u32)"""
    check(_lib.load().kpop_dev_dbscan(rs.handle, float(eps), _min_pts(min_pts), d_work, d_labels, d_core_of, d_degree, d_counts, stream))


def _dbscan_call(fn, lead, r1):
    labels, core_of, degree = (np.zeros(max(r1, 1), dtype=np.uint32) for _ in range(3))
    counts = np.zeros(3, dtype=np.uint32)
    check(fn(*lead, _ptr(labels), _ptr(core_of), _ptr(degree), _ptr(counts)))
    return labels[:r1], core_of[:r1], degree[:r1], counts


def distance_dbscan(m, metric, kind=EUCLIDEAN, p=2.0, normalize=True, eps=0.0, min_pts=1):
    """RefSet(m, ...).dbscan(eps, min_pts) without keeping the set: one call of kpop_distance_dbscan ->
    (labels u32 [rows], core_of u32 [rows], degree u32 [rows], counts u32 [3])"""
    lead, rows = _set_geometry(m, metric, kind, p, normalize)
    return _dbscan_call(_lib.load().kpop_distance_dbscan, lead + [float(eps), _min_pts(min_pts)], rows)


def dev_spanning_forest_workspace_bytes(rs):
    """the size of d_work for dev_spanning_forest, for the set's r1 at the time of the call"""
    return int(_lib.load().kpop_dev_spanning_forest_workspace_bytes(rs.handle))


def dev_spanning_forest(rs, max_distance, d_work, d_n_edges, d_edge_i, d_edge_j, d_edge_dist, d_labels=None, stream=0):
    """enqueue only: d_n_edges[1] (u32), d_edge_i / d_edge_j (u32) and d_edge_dist (f64) of r1 - 1 entries each, the first
    *d_n_edges written; d_labels[r1] (u32) or None"""
    check(_lib.load().kpop_dev_spanning_forest(rs.handle, float(max_distance), d_work, d_n_edges, d_edge_i, d_edge_j, d_edge_dist, d_labels, stream))


def _forest_call(fn, lead, r1, core):
    """the edges of a forest, cut at their count, then the rows' core distances (core: the mutual-reachability forest) and labels"""
    room = max(r1 - 1, 1)
    edges = (np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.float64))
    rows = ((np.zeros(max(r1, 1), dtype=np.float64),) if core else ()) + (np.zeros(max(r1, 1), dtype=np.uint32),)
    n = C.c_uint32()
    check(fn(*lead, C.byref(n), *_pointers(edges + rows)))
    n = int(n.value)
    return tuple(x[:n] for x in edges) + tuple(x[:r1] for x in rows)


def distance_spanning_forest(m, metric, kind=EUCLIDEAN, p=2.0, normalize=True, max_distance=float("inf")):
    """RefSet(m, ...).spanning_forest(max_distance) without keeping the set: one call of kpop_distance_spanning_forest
    -> (edge_i, edge_j, edge_dist, labels)"""
    lead, rows = _set_geometry(m, metric, kind, p, normalize)
    return _forest_call(_lib.load().kpop_distance_spanning_forest, lead + [float(max_distance)], rows, core=False)


def forest_cut(r1, edge_i, edge_j, edge_dist, T):
    """The connected components of a list of edges cut at T (the edges with edge_dist <= T united) -> (labels u32 [r1], n_clusters),
    labels[i] the smallest row index of row i's component.  Host arithmetic alone: no GPU, no init.  Over a spanning_forest and
    T <= its max_distance: RefSet.clusters(T), exactly (kpop_forest_cut, include/kpop_hip.h)."""
    ei = np.ascontiguousarray(edge_i, dtype=np.uint32)
    ej = np.ascontiguousarray(edge_j, dtype=np.uint32)
    ed = np.ascontiguousarray(edge_dist, dtype=np.float64)
    if not (ei.ndim == ej.ndim == ed.ndim == 1 and len(ei) == len(ej) == len(ed)):
        raise ValueError("edge_i, edge_j and edge_dist: three lists of one length")
    r1, n_edges = int(r1), len(ei)
    labels = np.zeros(max(r1, 1), dtype=np.uint32)
    n = C.c_uint32()
    check(_lib.load().kpop_forest_cut(r1, n_edges, _p(_nz(ei, np.uint32), C.c_uint32), _p(_nz(ej, np.uint32), C.c_uint32),
                                      _p(_nz(ed, np.float64), C.c_double), float(T), _p(labels, C.c_uint32), C.byref(n)))
    return labels[:r1], int(n.value)


def dev_core_distances_workspace_bytes(rs, min_pts):
    """the size of d_work for dev_core_distances, for the set's r1 at the time of the call: the lists of one slab of rows"""
    return int(_lib.load().kpop_dev_core_distances_workspace_bytes(rs.handle, _min_pts(min_pts)))


def dev_core_distances(rs, min_pts, d_work, d_core_dist, stream=0):
    """enqueue only: d_core_dist[r1] (f64)"""
    check(_lib.load().kpop_dev_core_distances(rs.handle, _min_pts(min_pts), d_work, d_core_dist, stream))


def dev_reachability_forest_workspace_bytes(rs, min_pts):
    """the size of d_work for dev_reachability_forest, for the set's r1 at the time of the call"""
    return int(_lib.load().kpop_dev_reachability_tree_workspace_bytes(rs.handle, _min_pts(min_pts)))


def dev_reachability_forest(rs, min_pts, max_distance, d_work, d_n_edges, d_edge_i, d_edge_j, d_edge_dist, d_core_dist=None, d_labels=None, stream=0):
    """enqueue only: d_n_edges[1] (u32), d_edge_i / d_edge_j (u32) and d_edge_dist (f64) of r1 - 1 entries each, the first
    *d_n_edges written; d_core_dist[r1] (f64) or None; d_labels[r1] (u32) or None"""
    check(_lib.load().kpop_dev_reachability_tree(rs.handle, _min_pts(min_pts), float(max_distance), d_work, d_n_edges, d_edge_i, d_edge_j, d_edge_dist,
                                                 d_core_dist, d_labels, stream))


def distance_reachability_forest(m, metric, kind=EUCLIDEAN, p=2.0, normalize=True, min_pts=1, max_distance=float("inf")):
    """RefSet(m, ...).reachability_forest(min_pts, max_distance) without keeping the set: one call of kpop_distance_reachability_tree
    -> (edge_i, edge_j, edge_dist, core_dist, labels)"""
    lead, rows = _set_geometry(m, metric, kind, p, normalize)
    return _forest_call(_lib.load().kpop_distance_reachability_tree, lead + [_min_pts(min_pts), float(max_distance)], rows, core=True)


def reachability_cut(r1, edge_i, edge_j, edge_dist, core_dist, T):
    """A list of edges cut at T (the edges with edge_dist <= T united) -> (labels u32 [r1], counts u32 [3]): a row with core_dist <= T gets
    the smallest row index of its component, every other row NOISE; counts: the components with such a row, those rows, the noise rows.
    Host arithmetic alone: no GPU, no init.  Over a reachability_forest and T <= its max_distance: RefSet.dbscan(T, min_pts)'s labels on
    every core row and its counts[0], counts[1]; its border rows are noise here (kpop_reachability_cut, include/kpop_hip.h)."""
    ei = np.ascontiguousarray(edge_i, dtype=np.uint32)
    ej = np.ascontiguousarray(edge_j, dtype=np.uint32)
    ed = np.ascontiguousarray(edge_dist, dtype=np.float64)
    core = np.ascontiguousarray(core_dist, dtype=np.float64)
    if not (ei.ndim == ej.ndim == ed.ndim == 1 and len(ei) == len(ej) == len(ed)):
        raise ValueError("edge_i, edge_j and edge_dist: three lists of one length")
    r1, n_edges = int(r1), len(ei)
    if core.shape != (r1,):
        raise ValueError("core_dist: a core distance for each of the %d rows" % r1)
    labels = np.zeros(max(r1, 1), dtype=np.uint32)
    counts = np.zeros(3, dtype=np.uint32)
    check(_lib.load().kpop_reachability_cut(r1, n_edges, _p(_nz(ei, np.uint32), C.c_uint32), _p(_nz(ej, np.uint32), C.c_uint32),
                                            _p(_nz(ed, np.float64), C.c_double), _p(_nz(core, np.float64), C.c_double), float(T), _p(labels, C.c_uint32),
                                            _p(counts, C.c_uint32)))
    return labels[:r1], counts


Silhouette = collections.namedtuple("Silhouette", "own_mean other_mean other_class silhouette class_rows medoid medoid_mean")


def _left_out_classes(class_of, r1, n_classes):
    """_classes where NO_CLASS leaves a row out: it does not count towards the number of classes"""
    class_of = np.asarray(class_of)
    if class_of.ndim != 1 or len(class_of) != r1:
        raise ValueError("class_of: one class, or NO_CLASS, for each of the set's %d rows" % r1)
    if len(class_of) and (class_of.min() < 0 or class_of.max() > 0xFFFFFFFF):
        raise ValueError("class_of: classes are uint32")
    class_of = _c(class_of, np.uint32)
    if n_classes is None:
        kept = class_of[class_of != NO_CLASS]
        n_classes = int(kept.max()) + 1 if len(kept) else 1
    n_classes = int(n_classes)
    if not 0 <= n_classes <= 0xFFFFFFFF:
        raise ValueError("n_classes: a count of classes")
    return class_of, n_classes


def _silhouette_call(fn, lead, r1, class_of, n_classes):
    class_of, n_classes = _left_out_classes(class_of, r1, n_classes)
    rows, classes = max(r1, 1), max(min(n_classes, 65536), 1)  # (the library refuses more classes before it writes)
    res = (np.zeros(rows, dtype=np.float64), np.zeros(rows, dtype=np.float64), np.zeros(rows, dtype=np.uint32), np.zeros(rows, dtype=np.float64),
           np.zeros(classes, dtype=np.uint32), np.zeros(classes, dtype=np.uint32), np.zeros(classes, dtype=np.float64))
    check(fn(*lead, _ptr(class_of), n_classes, *_pointers(res)))
    return Silhouette(*[x[:r1] for x in res[:4]], *[x[:n_classes] for x in res[4:]])


def dev_silhouette_workspace_bytes(rs, n_classes):
    """the size of d_work for dev_silhouette, for the set's r1 at the time of the call; 0 for an n_classes the call refuses"""
    return int(_lib.load().kpop_dev_silhouette_workspace_bytes(rs.handle, int(n_classes)))


def dev_silhouette(rs, d_class_of, n_classes, d_work, d_own_mean=None, d_other_mean=None, d_other_class=None, d_silhouette=None, d_class_rows=None,
                   d_medoid=None, d_medoid_mean=None, stream=0):
    """enqueue only: d_own_mean / d_other_mean / d_silhouette (f64 [r1]), d_other_class (u32 [r1]), d_class_rows / d_medoid (u32 [n_classes]),
    d_medoid_mean (f64 [n_classes]) as RefSet.silhouette returns them, each or None; d_class_of (u32, one a row of the set) is trusted:
    an entry that is no class counts as left out"""
    check(_lib.load().kpop_dev_silhouette(rs.handle, d_class_of, int(n_classes), d_work, d_own_mean, d_other_mean, d_other_class, d_silhouette, d_class_rows,
                                          d_medoid, d_medoid_mean, stream))


def distance_silhouette(m, metric, class_of, kind=EUCLIDEAN, p=2.0, normalize=True, n_classes=None):
    """RefSet(m, ...).silhouette(class_of, n_classes) without keeping the set: one call of kpop_distance_silhouette -> Silhouette"""
    lead, rows = _set_geometry(m, metric, kind, p, normalize)
    return _silhouette_call(_lib.load().kpop_distance_silhouette, lead, rows, class_of, n_classes)


def silhouette_summary(class_of, silhouette, n_classes=None):
    """The mean silhouette of each class and of all the rows that are not left out -> (class_mean f64 [n_classes], overall_mean), both summed
    in ascending row order; an empty class gives NaN.  Host arithmetic alone: no GPU, no init (kpop_silhouette_summary, include/kpop_hip.h)."""
    silhouette = _c(silhouette, np.float64)
    if silhouette.ndim != 1:
        raise ValueError("silhouette: one value a row")
    class_of, n_classes = _left_out_classes(class_of, len(silhouette), n_classes)
    class_mean = np.zeros(max(min(n_classes, 65536), 1), dtype=np.float64)
    overall = C.c_double()
    check(_lib.load().kpop_silhouette_summary(len(silhouette), _p(_nz(class_of, np.uint32), C.c_uint32), n_classes, _p(_nz(silhouette, np.float64), C.c_double),
                                              _p(class_mean, C.c_double), C.byref(overall)))
    return class_mean[:n_classes], float(overall.value)


ClassLinkage = collections.namedtuple("ClassLinkage", "class_rows mean_dist min_dist max_dist min_i min_j")
ClassTree = collections.namedtuple("ClassTree", "left right height size")
LINK_SINGLE, LINK_COMPLETE, LINK_AVERAGE = 0, 1, 2
LINK_MAX_CLASSES = 4096


def _class_linkage_call(fn, lead, r1, class_of, n_classes):
    class_of, n_classes = _left_out_classes(class_of, r1, n_classes)
    nc = n_classes if 1 <= n_classes <= LINK_MAX_CLASSES else 1  # (the library refuses any other number of classes before it writes)
    res = (np.zeros(nc, dtype=np.uint32), np.zeros((nc, nc), dtype=np.float64), np.zeros((nc, nc), dtype=np.float64), np.zeros((nc, nc), dtype=np.float64),
           np.zeros((nc, nc), dtype=np.uint32), np.zeros((nc, nc), dtype=np.uint32))
    check(fn(*lead, _ptr(class_of), n_classes, *_pointers(res)))
    return ClassLinkage(*res)


def dev_class_linkage_workspace_bytes(rs, n_classes):
    """the size of d_work for dev_class_linkage, for the set's r1 at the time of the call; 0 for an n_classes the call refuses"""
    return int(_lib.load().kpop_dev_class_linkage_workspace_bytes(rs.handle, int(n_classes)))


def dev_class_linkage(rs, d_class_of, n_classes, d_work, d_class_rows=None, d_mean_dist=None, d_min_dist=None, d_max_dist=None, d_min_i=None, d_min_j=None,
                      stream=0):
    """enqueue only: d_class_rows (u32 [n_classes]), d_mean_dist / d_min_dist / d_max_dist (f64 [n_classes^2]), d_min_i / d_min_j (u32
    [n_classes^2]) as RefSet.class_linkage returns them, each or None; d_class_of (u32, one a row of the set) is trusted: an entry that is
    no class counts as left out"""
    check(_lib.load().kpop_dev_class_linkage(rs.handle, d_class_of, int(n_classes), d_work, d_class_rows, d_mean_dist, d_min_dist, d_max_dist, d_min_i, d_min_j,
                                             stream))


def distance_class_linkage(m, metric, class_of, kind=EUCLIDEAN, p=2.0, normalize=True, n_classes=None):
    """RefSet(m, ...).class_linkage(class_of, n_classes) without keeping the set: one call of kpop_distance_class_linkage -> ClassLinkage"""
    lead, rows = _set_geometry(m, metric, kind, p, normalize)
    return _class_linkage_call(_lib.load().kpop_distance_class_linkage, lead, rows, class_of, n_classes)


def class_tree(class_rows, dist, linkage):
    """The agglomeration of the classes under a table of RefSet.class_linkage -> ClassTree(left u32 [n], right u32 [n], height f64 [n], size
    u32 [n]), n the merges.  linkage: LINK_SINGLE (pass min_dist), LINK_COMPLETE (max_dist) or LINK_AVERAGE (mean_dist: UPGMA weighted by
    class_rows).  The leaves are the classes with rows, their ids their class numbers; merge t makes node n_classes + t of the two live
    nodes least under (distance, lower id, higher id): left < right, height that distance, size the rows under the new node.  A NaN is
    never the least: where no two live nodes have a number between them the merges stop and the result is a forest.  Host arithmetic
    alone: no GPU, no init (kpop_class_tree, include/kpop_hip.h)."""
    class_rows = np.asarray(class_rows)
    if class_rows.ndim != 1 or (len(class_rows) and (class_rows.min() < 0 or class_rows.max() > 0xFFFFFFFF)):
        raise ValueError("class_rows: one count of rows a class")
    class_rows = _c(class_rows, np.uint32)
    n_classes = len(class_rows)
    dist = _c(dist, np.float64)
    if dist.shape != (n_classes, n_classes):
        raise ValueError("dist: a table of %d x %d distances" % (n_classes, n_classes))
    n = n_classes - 1 if 2 <= n_classes <= LINK_MAX_CLASSES else 1  # (as above; one entry so that every pointer is valid)
    left, right, size = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    height = np.zeros(n, dtype=np.float64)
    n_merges = C.c_uint32()
    check(_lib.load().kpop_class_tree(n_classes, _p(_nz(class_rows, np.uint32), C.c_uint32), _p(_nz(dist, np.float64), C.c_double), int(linkage),
                                      C.byref(n_merges), _p(left, C.c_uint32), _p(right, C.c_uint32), _p(height, C.c_double), _p(size, C.c_uint32)))
    k = int(n_merges.value)
    return ClassTree(left[:k], right[:k], height[:k], size[:k])


def class_tree_newick(tree, n_classes, names=None):
    """The Newick strings of a ClassTree, one a root in ascending node id: a leaf is names[class] (its class number without names), a branch's
    length the height of the parent minus the height of the child (a leaf lies at height 0), written with repr's shortest digits.  Leaves
    that no merge names are not written (class_tree does not say which classes have rows).  Plain Python: no library call."""
    n_classes = int(n_classes)
    left, right, height = [int(v) for v in tree.left], [int(v) for v in tree.right], [float(v) for v in tree.height]
    if not len(left) == len(right) == len(height):
        raise ValueError("tree: left, right and height of one length")
    if names is not None and len(names) < n_classes:
        raise ValueError("names: one a class")
    child = set(left) | set(right)
    for t, (a, b) in enumerate(zip(left, right)):
        if not (0 <= a < b < n_classes + t):
            raise ValueError("tree: merge %d joins nodes %d and %d" % (t, a, b))

    def node_height(v):
        return 0.0 if v < n_classes else height[v - n_classes]

    def label(v):
        return str(v) if names is None else str(names[v])

    out = []
    for root in range(n_classes, n_classes + len(left)):
        if root in child:
            continue
        # (an explicit stack: a chain of 4,095 merges is deeper than Python's recursion limit)
        text, stack = {}, [(root, False)]
        while stack:
            v, seen = stack.pop()
            if v < n_classes:
                text[v] = label(v)
            elif not seen:
                stack.extend([(v, True), (left[v - n_classes], False), (right[v - n_classes], False)])
            else:
                a, b = left[v - n_classes], right[v - n_classes]
                text[v] = "(%s:%r,%s:%r)" % (text.pop(a), node_height(v) - node_height(a), text.pop(b), node_height(v) - node_height(b))
        out.append(text[root] + ";")
    return out


FarthestFirst = collections.namedtuple("FarthestFirst", "pick pick_radius pick_parent rep_of rep_dist n_passes")


def _farthest_first_arguments(rows, max_picks, seeds):
    """max_picks None: every row; seeds None: none, a FarthestFirst: its picks"""
    max_picks = rows if max_picks is None else int(max_picks)
    if not 0 <= max_picks <= 0xFFFFFFFF:
        raise ValueError("max_picks: a count of rows")
    if isinstance(seeds, FarthestFirst):
        seeds = seeds.pick
    seeds = np.zeros(0, dtype=np.uint32) if seeds is None else np.asarray(seeds)
    if seeds.ndim != 1 or (len(seeds) and (seeds.min() < 0 or seeds.max() > 0xFFFFFFFF)):
        raise ValueError("seeds: row indices")
    return max_picks, _c(seeds, np.uint32)


def _farthest_first_call(fn, lead, rows, max_picks, cover_radius, seeds):
    max_picks, seeds = _farthest_first_arguments(rows, max_picks, seeds)
    k, n = max(min(max_picks, rows), 1), max(rows, 1)
    res = (np.zeros(k, dtype=np.uint32), np.zeros(k, dtype=np.float64), np.zeros(k, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.float64))
    picks, passes = C.c_uint32(), C.c_uint32()
    check(fn(*lead, max_picks, float(cover_radius), _ptr(seeds), len(seeds), C.byref(picks), *_pointers(res), C.byref(passes)))
    picks = int(picks.value)
    return FarthestFirst(res[0][:picks], res[1][:picks], res[2][:picks], res[3][:rows], res[4][:rows], int(passes.value))


def dev_farthest_first_workspace_bytes(rs, max_picks):
    """the size of d_work for dev_farthest_first, for the set's r1 at the time of the call"""
    return int(_lib.load().kpop_dev_farthest_first_workspace_bytes(rs.handle, int(max_picks)))


def dev_farthest_first(rs, max_picks, cover_radius, d_work, d_counts, d_pick=None, d_pick_radius=None, d_pick_parent=None, d_rep_of=None, d_rep_dist=None,
                       d_seeds=None, n_seeds=0, stream=0):
    """enqueue only: d_counts[2] (u32: n_picks, n_passes); d_pick / d_pick_parent (u32) and d_pick_radius (f64) with room for min(max_picks, r1)
    entries, d_rep_of (u32 [r1]), d_rep_dist (f64 [r1]), each or None; d_seeds (u32 [n_seeds]) is trusted to hold distinct rows"""
    check(_lib.load().kpop_dev_farthest_first(rs.handle, int(max_picks), float(cover_radius), d_seeds, int(n_seeds), d_work, d_pick, d_pick_radius,
                                              d_pick_parent, d_rep_of, d_rep_dist, d_counts, stream))


def distance_farthest_first(m, metric, kind=EUCLIDEAN, p=2.0, normalize=True, max_picks=None, cover_radius=-1.0, seeds=None):
    """RefSet(m, ...).farthest_first(max_picks, cover_radius, seeds) without keeping the set: one call of kpop_distance_farthest_first ->
    FarthestFirst"""
    lead, rows = _set_geometry(m, metric, kind, p, normalize)
    return _farthest_first_call(_lib.load().kpop_distance_farthest_first, lead, rows, max_picks, cover_radius, seeds)


KMedoids = collections.namedtuple("KMedoids", "medoid class_of dist own_mean class_rows cost n_iter converged")


def _kmedoids_arguments(medoids, max_iter):
    """medoids: row indices, or a FarthestFirst: its picks"""
    if isinstance(medoids, FarthestFirst):
        medoids = medoids.pick
    medoids = np.asarray(medoids)
    if medoids.ndim != 1 or (len(medoids) and (medoids.min() < 0 or medoids.max() > 0xFFFFFFFF)):
        raise ValueError("medoids: row indices")
    max_iter = int(max_iter)
    if not 0 <= max_iter < 0xFFFFFFFF:
        raise ValueError("max_iter: a count of rounds")
    return _c(medoids, np.uint32), max_iter


def _kmedoids_call(fn, lead, rows, medoids, max_iter):
    init, max_iter = _kmedoids_arguments(medoids, max_iter)
    n, k = max(rows, 1), max(min(len(init), 65536), 1)  # (the library refuses more medoids before it writes)
    res = (np.zeros(k, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64), np.zeros(k, dtype=np.uint32),
           np.zeros(max_iter + 1, dtype=np.float64))
    n_iter, conv = C.c_uint32(), C.c_int()
    check(fn(*lead, len(init), _ptr(init), max_iter, *_pointers(res), C.byref(n_iter), C.byref(conv)))
    n_iter, k = int(n_iter.value), len(init)
    return KMedoids(res[0][:k], res[1][:rows], res[2][:rows], res[3][:rows], res[4][:k], res[5][:n_iter + 1], n_iter, bool(conv.value))


def dev_kmedoids_workspace_bytes(rs, n_medoids, max_iter):
    """the size of d_work for dev_kmedoids, for the set's r1 at the time of the call; 0 for arguments the call refuses"""
    return int(_lib.load().kpop_dev_kmedoids_workspace_bytes(rs.handle, int(n_medoids), int(max_iter)))


def dev_kmedoids(rs, n_medoids, d_init, max_iter, d_work, d_counts, d_medoid=None, d_class_of=None, d_dist=None, d_own_mean=None, d_class_rows=None, d_cost=None,
                 stream=0):
    """enqueue only, max_iter + 1 rounds: d_counts[2] (u32: n_iter, converged); d_medoid / d_class_rows (u32 [n_medoids]), d_class_of (u32 [r1]),
    d_dist / d_own_mean (f64 [r1]), d_cost (f64 [max_iter + 1], NaN past n_iter), each or None; d_init (u32 [n_medoids]) is trusted to hold
    distinct rows"""
    check(_lib.load().kpop_dev_kmedoids(rs.handle, int(n_medoids), d_init, int(max_iter), d_work, d_medoid, d_class_of, d_dist, d_own_mean, d_class_rows, d_cost,
                                        d_counts, stream))


def distance_kmedoids(m, metric, medoids, kind=EUCLIDEAN, p=2.0, normalize=True, max_iter=100):
    """RefSet(m, ...).kmedoids(medoids, max_iter) without keeping the set, medoids an index array or a FarthestFirst: one call of
    kpop_distance_kmedoids -> KMedoids"""
    lead, rows = _set_geometry(m, metric, kind, p, normalize)
    return _kmedoids_call(_lib.load().kpop_distance_kmedoids, lead, rows, medoids, max_iter)


Lof = collections.namedtuple("Lof", "kdist n_neigh lrd lof")


def _lof_call(fn, lead, rows):
    n = max(rows, 1)
    res = (np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64))
    check(fn(*lead, *_pointers(res)))
    return Lof(*[x[:rows] for x in res])


def dev_lof_workspace_bytes(rs, k):
    """the size of d_work for dev_lof, for the set's r1 at the time of the call; 0 for a k the call refuses"""
    return int(_lib.load().kpop_dev_lof_workspace_bytes(rs.handle, _min_pts(k)))


def dev_lof(rs, k, d_work, d_kdist=None, d_n_neigh=None, d_lrd=None, d_lof=None, stream=0):
    """enqueue only: d_kdist / d_lrd / d_lof (f64 [r1]) and d_n_neigh (u32 [r1]) as RefSet.lof returns them, each or None"""
    check(_lib.load().kpop_dev_lof(rs.handle, _min_pts(k), d_work, d_kdist, d_n_neigh, d_lrd, d_lof, stream))


def dev_lof_score_workspace_bytes(rs, r2, k):
    """the size of d_work for dev_lof_score over r2 query rows: a slab's lists and sums, whatever the set's r1; 0 for a k the call refuses"""
    return int(_lib.load().kpop_dev_lof_score_workspace_bytes(rs.handle, int(r2), _min_pts(k)))


def dev_lof_score(rs, k, d_set_kdist, d_set_lrd, d_m2, r2, d_work, d_kdist=None, d_n_neigh=None, d_lrd=None, d_lof=None, stream=0):
    """enqueue only: d_set_kdist / d_set_lrd (f64 [r1]) from dev_lof at the same k, d_m2 (f64 [r2][n_dims]); the outputs as in dev_lof, [r2]"""
    check(_lib.load().kpop_dev_lof_score(rs.handle, _min_pts(k), d_set_kdist, d_set_lrd, d_m2, int(r2), d_work, d_kdist, d_n_neigh, d_lrd, d_lof, stream))


def distance_lof(m, metric, k=20, kind=EUCLIDEAN, p=2.0, normalize=True):
    """RefSet(m, ...).lof(k) without keeping the set: one call of kpop_distance_lof -> Lof"""
    lead, rows = _set_geometry(m, metric, kind, p, normalize)
    return _lof_call(_lib.load().kpop_distance_lof, lead + [_min_pts(k)], rows)


DensityPeaks = collections.namedtuple("DensityPeaks", "density delta parent labels counts")


def _density_peaks_call(fn, lead, rows, eps, density, min_density, min_delta):
    n = max(rows, 1)
    if density is not None:
        density = _c(density, np.float64)
        if density.shape != (rows,):
            raise ValueError("density: one score for each of the set's %d rows" % rows)
    cut = min_delta is not None
    res = (np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.uint32))
    labels, counts = (np.zeros(n, dtype=np.uint32), np.zeros(3, dtype=np.uint32)) if cut else (None, None)
    # (no eps: a NaN, which the library refuses when there is no density either)
    check(fn(*lead, float("nan") if eps is None else float(eps), None if density is None else _ptr(density), float(min_density),
             float(min_delta) if cut else float("inf"), *_pointers(res), _ptr(labels) if cut else None, _ptr(counts) if cut else None))
    return DensityPeaks(res[0][:rows], res[1][:rows], res[2][:rows], labels[:rows] if cut else None, counts)


def dev_density_peaks_workspace_bytes(rs):
    """the size of d_work for dev_density_peaks, for the set's r1 at the time of the call"""
    return int(_lib.load().kpop_dev_density_peaks_workspace_bytes(rs.handle))


def dev_density_peaks(rs, eps, d_work, d_density=None, min_density=float("-inf"), min_delta=float("inf"), d_density_out=None, d_delta=None, d_parent=None,
                      d_labels=None, d_counts=None, stream=0):
    """enqueue only: d_density (f64 [r1]) or None for the degrees at eps; d_density_out / d_delta (f64 [r1]), d_parent / d_labels (u32 [r1]),
    d_counts (u32 [3]) as RefSet.density_peaks returns them, each or None"""
    check(_lib.load().kpop_dev_density_peaks(rs.handle, float(eps), d_density, float(min_density), float(min_delta), d_work, d_density_out, d_delta, d_parent,
                                             d_labels, d_counts, stream))


def distance_density_peaks(m, metric, kind=EUCLIDEAN, p=2.0, normalize=True, eps=None, density=None, min_density=float("-inf"), min_delta=None):
    """RefSet(m, ...).density_peaks(eps, density, min_density, min_delta) without keeping the set: one call of kpop_distance_density_peaks ->
    DensityPeaks"""
    lead, rows = _set_geometry(m, metric, kind, p, normalize)
    return _density_peaks_call(_lib.load().kpop_distance_density_peaks, lead, rows, eps, density, min_density, min_delta)


def density_peaks_cut(density, delta, parent, min_density=float("-inf"), min_delta=float("inf")):
    """The cut of a density-peak forest at other thresholds, on the host (no GPU, no init) -> (labels u32 [r1], counts u32 [3]): what
    RefSet.density_peaks gives at these thresholds, from its density, delta and parent.  Refused: a NaN threshold, a parent that is
    neither NOISE, the row itself, nor a row ranking strictly above it (kpop_density_peaks_cut, include/kpop_hip.h)."""
    density, delta, parent = _c(density, np.float64), _c(delta, np.float64), np.asarray(parent)
    if parent.ndim != 1 or (len(parent) and (parent.min() < 0 or parent.max() > 0xFFFFFFFF)):
        raise ValueError("parent: one uint32 a row")
    parent = _c(parent, np.uint32)
    r1 = len(parent)
    if density.shape != (r1,) or delta.shape != (r1,):
        raise ValueError("density, delta, parent: one entry a row")
    labels, counts = np.zeros(max(r1, 1), dtype=np.uint32), np.zeros(3, dtype=np.uint32)
    check(_lib.load().kpop_density_peaks_cut(r1, _ptr(density), _ptr(delta), _ptr(parent), float(min_density), float(min_delta), _ptr(labels), _ptr(counts)))
    return labels[:r1], counts


def dense_labels(labels):
    """The labels that the clustering calls return (the smallest row index of a component, or NOISE) as classes 0 .. n - 1 in ascending
    label order -> (class_of u32 [r1], n_classes, label_of_class u32 [n_classes]); NOISE becomes NO_CLASS.  What clusters, forest_cut,
    dbscan and reachability_cut give goes through this into RefSet.silhouette."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or (len(labels) and (labels.min() < 0 or labels.max() > 0xFFFFFFFF)):
        raise ValueError("labels: one uint32 a row")
    labels = _c(labels, np.uint32)
    kept = labels != NOISE
    label_of_class, inverse = np.unique(labels[kept], return_inverse=True)
    class_of = np.full(len(labels), NO_CLASS, dtype=np.uint32)
    class_of[kept] = inverse.astype(np.uint32)
    return class_of, len(label_of_class), label_of_class.astype(np.uint32)
