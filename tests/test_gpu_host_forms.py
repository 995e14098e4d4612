"""The host-buffer forms of the calls on a resident set, through ctypes: the one rule they share (csrc/host_call.h; DESIGN.md, "The
self-join, once").  An output that include/kpop_hip.h documents as optional may be NULL, alone or with any other, and what the
caller does ask for does not depend on what it left out.

Every form in the table is called with every output present, with every optional output NULL and with each optional output alone
present; every call returns KPOP_OK and every output that is present holds the bits of the first call -- over the whole array, so also
the sentinel the test wrote where the call writes nothing.  Where an output is cut at a count the library reads first (the forests'
edges, the range query's lists, the traversal's picks), the radius leaves the count strictly between 0 and the room, and the entries
past it keep the sentinel.  For the representatives, the known rows' entries of both arrays stay the caller's.

Sets of 0, 1 and 67 rows of 3 dimensions (67: one ragged column group; 3: a ragged step), euclidean, normalised and not.  The list
of optional outputs is the header's: kpop_neighbours_within's two lists go together (one alone is KPOP_ERR_INVALID), kpop_kmedoids
needs a medoid and so a row, and n_passes of kpop_farthest_first is "a fact about the run": passed or left out, not compared."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 67)
D = 3
METRIC = np.array([1.0, 0.5, 2.0])
SENTINEL = 0xA5
U32, U64, F64, I32 = np.uint32, np.uint64, np.float64, np.int32
CTYPE = {U32: C.c_uint32, U64: C.c_uint64, F64: C.c_double, I32: C.c_int}
N_CLASSES, K, KS, MIN_PTS, MAX_PICKS, MAX_ITER, N_MEDOIDS = 3, 3, (1, 3), 3, 40, 10, 3
KEEP_AT_MOST, MAX_NEIGHBOURS = 2, 8


def rows_of(r1):
    """eight groups of rows apart from one another in place and in direction, so that a radius among the nearest-neighbour distances
    joins some rows and not all, normalised or not"""
    rng = np.random.RandomState(67)
    centres = 4.0 * rng.randn(8, D)
    m = centres[np.arange(67) % 8] + 0.3 * rng.randn(67, D)
    queries = np.vstack([rng.randn(4, D) * 4.0, m[:min(r1, 3)]])
    return np.ascontiguousarray(m[:r1]), np.ascontiguousarray(queries)


class Out:
    """an output of a call: n entries of dtype; optional: the header lets it be NULL, together with the others of its group; counted: cut
    at the form's count; compare False: not a result"""

    def __init__(self, name, dtype, n, optional=False, group=None, counted=False, compare=True):
        self.name, self.dtype, self.n, self.optional, self.counted, self.compare = name, dtype, max(int(n), 1), optional, counted, compare
        self.group = group or name


def ptr(a):
    return a.ctypes.data_as(C.POINTER(CTYPE[a.dtype.type]))


class Case:
    """a set and what the forms are asked about it"""

    def __init__(self, kpop, r1, normalize):
        self.r1, self.normalize = r1, normalize
        self.m, self.m2 = rows_of(r1)
        self.r2 = self.m2.shape[0]
        self.rs = kpop.RefSet(self.m, METRIC, 0, 2.0, bool(normalize))
        self.class_of = np.ascontiguousarray(np.arange(max(r1, 1)) % N_CLASSES, dtype=U32)
        self.ks = np.array(KS, dtype=U32)
        self.init = np.arange(N_MEDOIDS, dtype=U32) * 8  # rows of three groups
        self.radius = 1.0
        if r1 > 1:  # the median distance of a row to its nearest other row, as the set measures it
            G = self.rs.distance_rowwise(self.m)
            self.radius = float(np.median(np.sort(G, axis=1)[:, 1]))
        self.capacity = 0

    def forms(self):
        h, r1, r2, T = self.rs.handle, self.r1, self.r2, self.radius
        rows, room, slices, k_room = max(r1, 1), max(r1 - 1, 1), len(KS) * max(r1, 1), max(min(MAX_PICKS, r1), 1)
        lists = dict(optional=True, group="lists", counted=True)
        f = {
            "kpop_clusters_within": [h, T, 0, Out("labels", U32, rows), Out("n_clusters", U32, 1)],
            "kpop_representatives_within": [h, T, 0, Out("rep_of", U32, rows), Out("rep_dist", F64, rows, True), Out("n_reps", U32, 1)],
            "kpop_dbscan": [h, T, MIN_PTS, Out("labels", U32, rows), Out("core_of", U32, rows, True), Out("degree", U32, rows, True), Out("counts", U32, 3)],
            "kpop_spanning_forest": [h, T, Out("n_edges", U32, 1), Out("edge_i", U32, room, counted=True), Out("edge_j", U32, room, counted=True),
                                     Out("edge_dist", F64, room, counted=True), Out("labels", U32, rows, True)],
            "kpop_core_distances": [h, MIN_PTS, Out("core_dist", F64, rows)],
            "kpop_reachability_tree": [h, MIN_PTS, 2.0 * T, Out("n_edges", U32, 1), Out("edge_i", U32, room, counted=True), Out("edge_j", U32, room, counted=True),
                                       Out("edge_dist", F64, room, counted=True), Out("core_dist", F64, rows, True), Out("labels", U32, rows, True)],
            "kpop_neighbours_within": [h, ptr(self.m2), r2, T, self.capacity, Out("offsets", U64, r2 + 1), Out("idx", U32, self.capacity, **lists),
                                       Out("dist", F64, self.capacity, **lists)],
            "kpop_knn_vote": [h, ptr(self.class_of), N_CLASSES, ptr(self.m2), r2, K, Out("cls", U32, r2), Out("votes", U32, r2), Out("n", U32, r2),
                              Out("first", F64, r2, True)],
            "kpop_knn_ks_vote": [h, ptr(self.class_of), N_CLASSES, ptr(self.m2), r2, ptr(self.ks), len(KS), Out("cls", U32, len(KS) * r2),
                                 Out("votes", U32, len(KS) * r2), Out("n", U32, len(KS) * r2), Out("first", F64, len(KS) * r2, True)],
            "kpop_knn_validate": [h, ptr(self.class_of), N_CLASSES, None, ptr(self.ks), len(KS), Out("cls", U32, slices), Out("votes", U32, slices),
                                  Out("n", U32, slices), Out("first", F64, slices, True), Out("correct", U64, len(KS))],
            "kpop_silhouette": [h, ptr(self.class_of), N_CLASSES, Out("own_mean", F64, rows, True), Out("other_mean", F64, rows, True),
                                Out("other_class", U32, rows, True), Out("silhouette", F64, rows, True), Out("class_rows", U32, N_CLASSES, True),
                                Out("medoid", U32, N_CLASSES, True), Out("medoid_mean", F64, N_CLASSES, True)],
            "kpop_farthest_first": [h, MAX_PICKS, 3.0 * T, None, 0, Out("n_picks", U32, 1), Out("pick", U32, k_room, True, counted=True),
                                    Out("pick_radius", F64, k_room, True, counted=True), Out("pick_parent", U32, k_room, True, counted=True),
                                    Out("rep_of", U32, rows, True), Out("rep_dist", F64, rows, True), Out("n_passes", U32, 1, True, compare=False)],
            "kpop_refset_distance_rowwise": [h, ptr(self.m2), r2, Out("out", F64, r2 * r1)],
            "kpop_refset_distance_summary": [h, ptr(self.m2), r2, KEEP_AT_MOST, MAX_NEIGHBOURS, Out("stats", F64, r2 * 4), Out("n", U32, r2),
                                             Out("idx", U32, r2 * MAX_NEIGHBOURS), Out("dist", F64, r2 * MAX_NEIGHBOURS), Out("z", F64, r2 * MAX_NEIGHBOURS)],
        }
        if r1:  # (no medoids: KPOP_ERR_INVALID)
            k = min(N_MEDOIDS, r1)
            f["kpop_kmedoids"] = [h, k, ptr(self.init), MAX_ITER, Out("medoid", U32, k, True), Out("class_of", U32, rows, True), Out("dist", F64, rows, True),
                                  Out("own_mean", F64, rows, True), Out("class_rows", U32, k, True), Out("cost", F64, MAX_ITER + 1, True), Out("n_iter", U32, 1),
                                  Out("converged", I32, 1)]
        return f


# the count an output is cut at, and the room it is cut in
COUNT_OF = {"kpop_spanning_forest": lambda got: int(got["n_edges"][0]), "kpop_reachability_tree": lambda got: int(got["n_edges"][0]),
            "kpop_neighbours_within": lambda got: int(got["offsets"][-1]), "kpop_farthest_first": lambda got: int(got["n_picks"][0])}
FORMS = ("kpop_clusters_within", "kpop_representatives_within", "kpop_dbscan", "kpop_spanning_forest", "kpop_core_distances", "kpop_reachability_tree",
         "kpop_neighbours_within", "kpop_knn_vote", "kpop_knn_ks_vote", "kpop_knn_validate", "kpop_silhouette", "kpop_farthest_first", "kpop_kmedoids",
         "kpop_refset_distance_rowwise", "kpop_refset_distance_summary")


def call(name, args, present, before=None):
    """one call: the optional outputs whose group is not in `present` are NULL; every other output is an array of the sentinel (before(got)
    may write into them first) -> (the return code, the arrays by name)"""
    from kpop_amd import _lib
    got = {}
    for a in args:
        if isinstance(a, Out) and not (a.optional and a.group not in present):
            got[a.name] = np.frombuffer(bytes([SENTINEL]) * (a.n * np.dtype(a.dtype).itemsize), dtype=a.dtype).copy()
    if before:
        before(got)
    rc = getattr(_lib.load(), name)(*[(ptr(got[a.name]) if a.name in got else None) if isinstance(a, Out) else a for a in args])
    return rc, got


@pytest.fixture(scope="module")
def cases(kpop):
    made = {}
    for r1 in SIZES:
        for normalize in (0, 1):
            c = made[(r1, normalize)] = Case(kpop, r1, normalize)
            # the range query's room: what a counting call finds, and some more
            rc, got = call("kpop_neighbours_within", c.forms()["kpop_neighbours_within"], set())
            assert rc == 0
            c.capacity = int(got["offsets"][-1]) + 7
    yield made
    for c in made.values():
        c.rs.free()


@pytest.mark.parametrize("normalize", (0, 1))
@pytest.mark.parametrize("name,r1", [(name, r1) for name in FORMS for r1 in SIZES if (name, r1) != ("kpop_kmedoids", 0)])
def test_optional_outputs(cases, name, r1, normalize):
    args = cases[(r1, normalize)].forms()[name]
    outs = [a for a in args if isinstance(a, Out)]
    groups = sorted({a.group for a in outs if a.optional})
    rc, first = call(name, args, set(groups))
    assert rc == 0, "%s with every output: %d" % (name, rc)
    if name in COUNT_OF:
        n = COUNT_OF[name](first)
        for a in outs:
            if not a.counted:
                continue
            if r1 == 67:
                assert 0 < n < a.n, "%s: a count of %d in a room of %d pins nothing" % (name, n, a.n)
            assert n <= a.n and np.all(first[a.name][n:].view(np.uint8) == SENTINEL), "%s: %s is written past its %d entries" % (name, a.name, n)
    for present in [set()] + [{g} for g in groups]:
        rc, got = call(name, args, present)
        assert rc == 0, "%s with %s: %d" % (name, sorted(present) or "no optional output", rc)
        for a in outs:
            if a.name in got and a.compare:
                assert got[a.name].tobytes() == first[a.name].tobytes(), "%s with %s: %s differs" % (name, sorted(present) or "no optional output", a.name)


@pytest.mark.parametrize("normalize", (0, 1))
def test_the_known_rows_of_the_representatives_stay_the_callers(cases, normalize):
    c = cases[(67, normalize)]
    name, known_rows = "kpop_representatives_within", 30
    args = c.forms()[name]
    rc, scratch = call(name, args, {"rep_dist"})
    assert rc == 0 and 1 < int(scratch["n_reps"][0]) < 67

    def known(got):
        got["rep_of"][:known_rows] = scratch["rep_of"][:known_rows]

    args = [known_rows if i == 2 else a for i, a in enumerate(args)]
    for present in ({"rep_dist"}, set()):
        rc, got = call(name, args, present, before=known)
        assert rc == 0
        assert np.array_equal(got["rep_of"], scratch["rep_of"]) and got["n_reps"][0] == scratch["n_reps"][0]
        if present:
            assert np.all(got["rep_dist"][:known_rows].view(np.uint8) == SENTINEL)
            assert got["rep_dist"][known_rows:].tobytes() == scratch["rep_dist"][known_rows:].tobytes()
