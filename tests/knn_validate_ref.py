"""numpy reference of the k-NN validation (kpop_knn_validate, include/kpop_hip.h): the reference of the k-NN
vote (tests/knn_vote_ref.py) applied to the set's own r1 x r1 distance matrix with the entries that are left out set to NaN -- a NaN is
never a neighbour there.  Left out of row j's list: column j (group_of None), or every column of j's group.  By index or group, never by
distance.  Written from the declared semantics, not from the kernels."""
import numpy as np

from knn_vote_ref import NO_CLASS, knn_vote_ref


def leave_out(D, group_of=None):
    """-> a copy of the square matrix D with the entries that are left out set to NaN"""
    D = np.array(D, dtype=np.float64)
    assert D.ndim == 2 and D.shape[0] == D.shape[1]
    if group_of is None:
        np.fill_diagonal(D, np.nan)
    else:
        group_of = np.asarray(group_of)
        assert group_of.shape == (D.shape[0],)
        D[group_of[:, None] == group_of[None, :]] = np.nan
    return D


def knn_validate_ref(D, class_of, ks, group_of=None, n_classes=None):
    """-> (cls u32, votes u32, n u32, first f64, correct u64): the first four [len(ks)][r1], slice t the vote at k = ks[t] over the
    rows' lists without what is left out; correct[t] the rows whose class is their own (NO_CLASS is never correct)"""
    class_of = np.asarray(class_of)
    E = leave_out(D, group_of)
    r1 = E.shape[0]
    cls, votes, n = (np.zeros((len(ks), r1), dtype=np.uint32) for _ in range(3))
    first = np.zeros((len(ks), r1), dtype=np.float64)
    correct = np.zeros(len(ks), dtype=np.uint64)
    for t, k in enumerate(ks):
        cls[t], votes[t], n[t], first[t] = knn_vote_ref(E, class_of, k, n_classes)
        correct[t] = np.count_nonzero((cls[t] != NO_CLASS) & (cls[t].astype(np.int64) == class_of.astype(np.int64)))
    return cls, votes, n, first, correct


def same_validation(got, want, what=""):
    """the five arrays bit for bit"""
    from knn_vote_ref import same_votes
    assert len(got) == len(want) == 5, what
    for q in range(4):
        assert np.asarray(got[q]).shape == np.asarray(want[q]).shape, (what, q, np.asarray(got[q]).shape, np.asarray(want[q]).shape)
    for t in range(np.asarray(want[0]).shape[0]):
        same_votes(tuple(np.asarray(a)[t] for a in got[:4]), tuple(np.asarray(a)[t] for a in want[:4]), (what, "slice %d" % t))
    assert np.asarray(got[4]).dtype == np.uint64 and np.array_equal(got[4], want[4]), (what, "correct", np.asarray(got[4]).tolist(), np.asarray(want[4]).tolist())
