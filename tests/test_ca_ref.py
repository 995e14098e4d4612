"""CPU: both references of the twister generator (oracle/ca_ref.py: LAPACK's SVD, and the Gram route in numpy) satisfy the
invariants the GPU routes are held to, within the condition tests/ca_cases.py sets, on the smallest case of every family of
tests/test_gpu_ca_routes.py -- and the check fails on seeded faults."""
import numpy as np
import pytest

import ca_cases
from oracle import ca_ref

FAMILIES = [("default", lambda: ca_cases.reference(9, 3), None), ("smallest", lambda: ca_cases.reference(2, 2), None),
            ("blocked", lambda: ca_cases.reference(67, 32), None), ("counts as they are", lambda: ca_cases.reference(517, 257, False), None),
            ("near-duplicate classes", ca_cases.near_duplicate_reference, 129), ("I < J", lambda: ca_cases.reference(17, 40), None)]


@pytest.mark.parametrize("name,make,live", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_references_satisfy_the_invariants(name, make, live):
    ref = make()
    ref.assert_sound(ref.nd if live is None else live)
    for label, f in (("ca_gram", ca_ref.ca_gram), ("ca", ca_ref.ca)):
        ref.check(*f(ref.N, ref.normalize), label="%s, %s" % (name, label), route="CPU")


def test_gram_route_agrees_with_the_svd():
    """inertia to rounding; class positions and twister up to the sign of a dimension (random table: no close singular values
    among the leading ones)"""
    ref = ca_cases.reference(69, 33)
    tw, inertia, T = ca_ref.ca_gram(ref.N, True)
    tw_o, in_o, T_o = ca_ref.ca(ref.N, True)
    np.testing.assert_allclose(inertia, in_o, rtol=1e-12)
    assert np.max(np.abs(ca_ref.align_signs(tw[:, :8], tw_o[:, :8], axis=1) - tw_o[:, :8])) <= 1e-10 * np.max(np.abs(tw_o))
    assert np.max(np.abs(ca_ref.align_signs(T[:8], T_o[:8], axis=0) - T_o[:8])) <= 1e-10 * np.max(np.abs(T_o))
    assert np.all(T[:, 5] == 0.0) and np.all(T_o[:, 5] == 0.0)


def test_the_check_sees_seeded_faults():
    ref = ca_cases.reference(69, 33)
    outs = ca_ref.ca_gram(ref.N, True)
    ca_cases.seeded_faults(ref, *outs)
    with pytest.raises(AssertionError):  # a NaN is a failure, never a pass
        bad = np.array(outs[2], copy=True)
        bad[3, 7] = np.nan
        ref.check(outs[0], outs[1], bad)
