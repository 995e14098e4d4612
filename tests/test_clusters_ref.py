"""tests/clusters_ref.py, the numpy reference the GPU tests of kpop_clusters_within compare against, pinned on cases written by hand."""
import numpy as np
import pytest

from clusters_ref import cluster_sizes, clusters_ref

NAN = float("nan")


def seven_rows():
    """0 - 1 - 2 a chain (0 and 2 joined only through 1), 4 a duplicate of 3, 5 a row of NaN, 6 at exactly 1.0 from 3 and far from the rest"""
    D = np.full((7, 7), 9.0)
    np.fill_diagonal(D, 0.0)

    def put(j, i, v):
        D[j, i] = D[i, j] = v

    put(1, 0, 0.75)
    put(2, 1, 0.5)
    put(2, 0, 1.25)
    put(4, 3, 0.0)
    put(6, 3, 1.0)
    put(6, 4, 1.0)
    D[5, :] = NAN
    D[:, 5] = NAN
    return D


def test_seven_rows_by_hand():
    D = seven_rows()
    labels, n = clusters_ref(D, 1.0)  # the tie at T is inclusive
    assert labels.dtype == np.uint32
    assert labels.tolist() == [0, 0, 0, 3, 3, 5, 3] and n == 3
    assert cluster_sizes(labels) == [3, 3, 1]
    labels, n = clusters_ref(D, np.nextafter(1.0, 0.0))  # a rounding below the tie: row 6 is alone
    assert labels.tolist() == [0, 0, 0, 3, 3, 5, 6] and n == 4
    labels, n = clusters_ref(D, 0.6)  # 0 - 1 is cut
    assert labels.tolist() == [0, 1, 1, 3, 3, 5, 6] and n == 5
    labels, n = clusters_ref(D, 0.0)  # the duplicate alone
    assert labels.tolist() == [0, 1, 2, 3, 3, 5, 6] and n == 6
    labels, n = clusters_ref(D, -1.0)
    assert labels.tolist() == list(range(7)) and n == 7
    labels, n = clusters_ref(D, float("inf"))  # every pair whose distance is a number: the NaN row stays alone
    assert labels.tolist() == [0, 0, 0, 0, 0, 5, 0] and n == 2
    with pytest.raises(ValueError):
        clusters_ref(D, NAN)
    assert clusters_ref(np.zeros((0, 0)), 1.0)[1] == 0


def test_only_the_lower_triangle_is_read():
    D = seven_rows()
    want = clusters_ref(D, 1.0)[0]
    D[np.triu_indices(7)] = 0.0  # the diagonal and everything above it
    assert np.array_equal(clusters_ref(D, 1.0)[0], want)


def test_the_label_is_the_smallest_index_whatever_the_order_of_the_edges():
    """a component whose smallest row is met last: 5 - 9, 7 - 9, 2 - 7"""
    D = np.full((10, 10), 9.0)
    for j, i in ((9, 5), (9, 7), (7, 2)):
        D[j, i] = 0.1
    labels, n = clusters_ref(D, 0.5)
    assert labels.tolist() == [0, 1, 2, 3, 4, 2, 6, 2, 8, 2] and n == 7


def test_growing_equals_from_scratch():
    rng = np.random.RandomState(5)
    pts = np.round(rng.normal(size=(300, 2)), 1)
    pts[40] = NAN
    D = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    for T in (0.0, 0.1, 0.15, 0.3):
        whole, n = clusters_ref(D, T)
        assert np.array_equal(whole[whole], whole) and np.all(whole <= np.arange(300)) and n == len(set(whole.tolist()))
        assert whole[40] == 40
        for k in (0, 1, 150, 299, 300):
            first, _ = clusters_ref(D[:k, :k], T)
            grown, n_grown = clusters_ref(D, T, known=first)
            assert np.array_equal(grown, whole) and n_grown == n, (T, k)
    assert 3 < clusters_ref(D, 0.15)[1] < 297  # (neither everything nor nothing)
