"""Shared by test_ca_ref.py (CPU) and test_gpu_ca_routes.py (GPU): the tables of the eigen-solver route cases, their references
(computed once a table, never modified) and the one check both apply to a (twisted, inertia, twister) triple.

Tolerances come from the references alone (oracle/ca_ref.py): for every invariant 16 x the larger defect of ca_ref.ca's (LAPACK SVD)
and ca_ref.ca_gram's (numpy eigh of S'S) own outputs on the same table -- four bits for another order of the length-I dot products
and for up to ~15 sweeps of rotations where LAPACK makes one pass.  orthV has a floor of 1e-13: the cosine at which the solver's own
stopping rule may stop (jacobi_eigen_psd_device in ca.hip).  From 1,025 spectra on the full SVD is left out (seconds of CPU): ca_gram
alone, sigma still from numpy.linalg.svd(compute_uv=False)."""
import functools

import numpy as np

from oracle import ca_ref
from test_gpu_ca import synthetic_table

MARGIN = 16.0
COSINE_FLOOR = 1e-13
DEFECTS = ("orthT", "orthV", "lam", "lamT", "rec")  # (the inertia is held to lam's tolerance)
U = 2.0 ** -53


def random_table(I, J):
    """depth 50, one k-mer that occurs nowhere (row 5) -- except with fewer k-mers than spectra, where it would cost a rank and
    leave the last dimension null"""
    N = synthetic_table(np.random.RandomState(I + J), I, J, depth=50)
    if I > J and I > 5:
        N[5] = 0.0
    return N


def near_duplicate_table():
    """tools/probes/near_dependent_ca.py's table at 700 k-mers: thirty classes that are copies of others, ten that are copies up
    to one count in three k-mers.  129 dimensions with sigma_1 / sigma_d <= 919, then a drop to 1.8e14; an unpivoted Cholesky
    factorisation of its Gram matrix meets 31 pivots at the rounding floor."""
    rng = np.random.RandomState(3)
    I, J = 700, 160
    base = rng.gamma(2.0, 1.0, size=I)
    N = rng.poisson(np.outer(base, rng.lognormal(0, 0.5, size=J)) * 30).astype(np.float64)
    for j in range(30):
        N[:, 100 + j] = N[:, j]
    for j in range(10):
        N[:, 130 + j] = N[:, 40 + j]
        N[rng.randint(0, I, size=3), 130 + j] += 1
    return N


class Reference:
    def __init__(self, N, normalize):
        self.N, self.normalize = N, normalize
        self.N.setflags(write=False)
        I, J = N.shape
        self.nd = min(I, J) - 1
        self.ref = {"gram": ca_ref.invariants(N, normalize, *ca_ref.ca_gram(N, normalize))}
        self.sigma = self.ref["gram"]["sigma"]
        if J < 1025:
            self.ref["svd"] = ca_ref.invariants(N, normalize, *ca_ref.ca(N, normalize), sigma=self.sigma)
        self.live = self.ref["gram"]["live"]
        self.tol = {k: MARGIN * max(r[k] for r in self.ref.values()) for k in DEFECTS}
        self.tol["orthV"] = max(self.tol["orthV"], COSINE_FLOOR)
        self.tol["inertia"] = self.tol["lam"]

    def assert_sound(self, live):
        """a sick reference must not hide a failure"""
        assert self.live == live, (self.live, live)
        for r in self.ref.values():
            assert r["finite"] and r["massless_rows_zero"]
        for k, t in self.tol.items():
            assert t <= (2e-13 if k == "orthV" else 1e-12), (k, t)

    def invariants(self, twisted, inertia, twister):
        return ca_ref.invariants(self.N, self.normalize, twisted, inertia, twister, sigma=self.sigma)

    def check(self, twisted, inertia, twister, label="", route=""):
        """prints the figures (a row of DESIGN.md's table), then asserts them"""
        N, nd = self.N, self.nd
        I, J = N.shape
        assert twisted.shape == (J, nd) and inertia.shape == (nd,) and twister.shape == (nd, I)
        got = self.invariants(twisted, inertia, twister)
        print("\nCA-ROUTES | %s | %d x %d | %s | %s" % (label, I, J, route, " | ".join(
            "%s %.1e (%s; tol %.1e)" % (k, got[k], ", ".join("%s %.1e" % (n, r[k]) for n, r in self.ref.items()), self.tol[k]) for k in DEFECTS)))
        assert got["finite"], "an output holds a NaN or an infinity"
        assert got["massless_rows_zero"]
        for k in DEFECTS + ("inertia",):
            assert got[k] <= self.tol[k], (k, got[k], self.tol[k])
        # worst case: three roundings a term (sqrt, square, division) over a divisor summed in nd - 1 additions, and the
        # pairwise sum taken here (at most a dozen levels)
        assert got["inertia_sum"] <= (nd + 16) * U, got["inertia_sum"]
        # sorted eigenvalues through sqrt, square and one division: each is monotone under correct rounding
        assert got["inertia_rise"] == 0.0, got["inertia_rise"]
        # transition formula: a class's own normalised spectrum through the twister gives its position (on the live dimensions:
        # all of them but for the near-duplicate classes, whose null dimensions have rows of rounding noise over a singular value
        # of rounding noise in both references)
        x = N / N.sum(axis=0, keepdims=True)
        live = got["kappa"] <= 1e3
        np.testing.assert_allclose(twister[live] @ x, twisted.T[live], rtol=0, atol=1e-9 * np.max(np.abs(twisted)))
        return got


@functools.lru_cache(maxsize=None)
def reference(I, J, normalize=True):
    return Reference(random_table(I, J), normalize)


@functools.lru_cache(maxsize=None)
def near_duplicate_reference():
    return Reference(near_duplicate_table(), True)


def seeded_faults(ref, twisted, inertia, twister):
    """The check must see a twister whose rows are a valid basis in the wrong order (through the inertia: every row is tied to
    ITS singular value), and one whose leading row leans on its neighbour by 1e-9 (through orthT)."""
    swapped = np.array(twister, copy=True)
    swapped[[0, 1]] = swapped[[1, 0]]
    got = ref.invariants(twisted, inertia, swapped)
    assert got["inertia"] > ref.tol["inertia"], (got["inertia"], ref.tol["inertia"])
    mixed = np.array(twister, copy=True)
    mixed[0] = mixed[0] + 1e-9 * mixed[1]
    got = ref.invariants(twisted, inertia, mixed)
    assert got["orthT"] > ref.tol["orthT"], (got["orthT"], ref.tol["orthT"])
