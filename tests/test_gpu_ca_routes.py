"""Every route of the twister generator's eigen-solver (jacobi_eigen_psd_device in ca.hip chooses among five from the number of
spectra, the pivots of the Cholesky factorisation and the A/B bits of kpop_tune("dbg")), held to what makes its outputs a singular
value decomposition of the standardised table: oracle/ca_ref.py's invariants, which do not depend on signs or on gaps between
singular values, at tolerances taken from the CPU references alone (tests/ca_cases.py).  kpop_debug_ca says which route ran and
whether it converged: a case that takes another route than it is here for fails."""
import numpy as np
import pytest

import ca_cases

pytestmark = pytest.mark.gpu

PLAIN, LOOPED = 0, 9


def run(kpop, ref, label, blocked, on_factor, kernel, live=None, dbg=0, dead=None):
    from kpop_amd import api
    ref.assert_sound(ref.nd if live is None else live)
    api.tune("dbg", dbg)
    try:
        twisted, inertia, twister = kpop.ca(ref.N, ref.normalize)
        did = api.debug_ca()
    finally:
        api.tune("dbg", 0)
    route = "blocked %(blocked)d, on the factor %(on_factor)d, dead pivots %(dead)d, kernel %(kernel)d, %(sweeps)d sweeps (%(closing)d closing on G), cosine %(cosine).1e" % did
    ref.check(twisted, inertia, twister, label, route)
    assert did["converged"] == 1, did
    assert (did["blocked"], did["on_factor"], did["kernel"]) == (blocked, on_factor, kernel), did
    assert did["sweeps"] >= 1 and 0.0 <= did["cosine"] < 1e-13 and (did["closing"] >= 1) == bool(on_factor), did
    if dead is not None:
        assert dead(did["dead"]), did
    return twisted, inertia, twister


# J -> the route it takes by itself: plain steps below 32 spectra, then the register kernel on the Cholesky factor with
# ceil(J / 256) rows a thread, the looped kernel on the Gram matrix above 2,048
DEFAULT = [(3, PLAIN), (31, PLAIN), (32, 1), (33, 1), (35, 1), (255, 1), (256, 1), (257, 2), (258, 2), (513, 3), (1024, 4), (1025, 5),
           (1300, 6), (1636, 7), (2048, 8), (2049, LOOPED)]


@pytest.mark.parametrize("J,kernel", DEFAULT)
def test_default_route(kpop, J, kernel):
    """3: an odd number of columns (a bye a step); 35: J % 4 = 3 and ceil(J / 4) = 9, masked columns and the phantom block;
    257: 256 dimensions, exactly one slab of the U = S W product; 258: a last slab one dimension wide; 1636: the reference's
    own published dimension."""
    blocked = int(kernel != PLAIN)
    on_factor = int(blocked and kernel != LOOPED)
    run(kpop, ca_cases.reference(2 * J + 3, J), "default", blocked, on_factor, kernel, dead=(lambda d: d <= 1) if on_factor else (lambda d: d == 0))


def test_default_route_counts_as_they_are(kpop):
    run(kpop, ca_cases.reference(2 * 257 + 3, 257, False), "normalize=False", 1, 1, 2)


def test_smallest_table(kpop):
    run(kpop, ca_cases.reference(2, 2), "smallest", 0, 0, PLAIN)


@pytest.mark.parametrize("J,dbg,kernel", [(33, 2048, 1), (513, 2048, 3), (1025, 2048, 5), (2048, 2048, 8), (130, 64, LOOPED), (64, 32, PLAIN)])
def test_forced_route(kpop, J, dbg, kernel):
    """kpop_tune promises that results do not depend on its knobs: the same invariants at the same tolerances.  2048: the register
    kernel on G itself with V accumulated; 64: the looped kernel; 32: the plain steps."""
    run(kpop, ca_cases.reference(2 * J + 3, J), "dbg %d" % dbg, int(kernel != PLAIN), 0, kernel, dbg=dbg, dead=lambda d: d == 0)


def test_dead_pivots_send_the_iteration_back_to_G(kpop):
    """Near-duplicate classes: 31 pivots of the unpivoted factorisation sit at the rounding floor, G is restored and rotated with V
    accumulated.  The invariants on the 129 dimensions above the drop, the reconstruction over all 159."""
    run(kpop, ca_cases.near_duplicate_reference(), "near-duplicate classes", 1, 0, 1, live=129, dead=lambda d: d > 1)


@pytest.mark.parametrize("I,J,kernel", [(17, 40, 1), (120, 300, 2), (300, 2100, LOOPED)])
def test_fewer_kmers_than_spectra(kpop, I, J, kernel):
    """nd = I - 1, every dimension live; G has J - nd null directions (zero-norm columns once they are orthogonal).  Up to 2,048
    spectra they are dead pivots and the iteration runs on G; above, the looped kernel takes them without a factorisation."""
    run(kpop, ca_cases.reference(I, J), "I < J", 1, 0, kernel, dead=(lambda d: d == 0) if kernel == LOOPED else (lambda d: d > 1))


def test_the_check_sees_seeded_faults(kpop):
    ref = ca_cases.reference(2 * 33 + 3, 33)
    ca_cases.seeded_faults(ref, *kpop.ca(ref.N, True))
