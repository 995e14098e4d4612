"""tests/distill_ref.py, the CPU restatement the GPU distill is tested against, pinned to a case worked out by hand
(no GPU here): the yardstick must not merely agree with itself.

The case: 2 classes x 3 spectra, 3 k-mers; every spectrum sums to 16, so the normalised counts are sixteenths.
Spectra in database order A0 B0 A1 B1 A2 B2 (classes 0 1 0 1 0 1, numbered by first appearance), counts per k-mer:

             A0  A1  A2 |  B0  B1  B2
    k0        0   0   0 |   1   4   4         class A is all zero
    k1        0   1   3 |   4   8  10
    k2       16  15  13 |  11   4   2

In units of u = 1/16 (means) and u^2 = 1/256 (variances); n = 3 pairs in a diagonal cell, 9 in the off-diagonal one;
var = sum (d - mean)^2 / (n - 1); cov = sqrt(var) / mean:

    k0  AA  d = 0 0 0               mean 0   var 0               cov 0/0 = NaN
        BB  d = 3 3 0               mean 2   var (1+1+4)/2 = 3   cov sqrt(3)/2
        AB  d = 1 4 4, three times  mean 3   var 3(4+1+1)/8 = 9/4  cov (3/2)/3 = 1/2
    k1  AA  d = 1 3 2               mean 2   var (1+1+0)/2 = 1   cov 1/2
        BB  d = 4 6 2               mean 4   var (0+4+4)/2 = 4   cov 2/4 = 1/2
        AB  d = 4 8 10, 3 7 9, 1 5 7   sum 54, mean 6   squared deviations 4 4 16 9 1 9 25 1 1 = 70, var 70/8 = 35/4
                                    cov sqrt(35/4)/6
    k2  AA  d = 1 3 2               mean 2   var 1               cov 1/2
        BB  d = 7 9 2               mean 6   var (1+9+16)/2 = 13   cov sqrt(13)/6
        AB  d = 5 12 14, 4 11 13, 2 9 11   sum 81, mean 9   squared deviations 16 9 25 25 4 16 49 0 4 = 148, var 37/2
                                    cov sqrt(37/2)/9

Across cells, Inner = (AA, BB): Mean = half their sum, Median = sorted[2 / 2] = the larger; Outer = AB alone:

             InnerMean InnerMedian Outer |            InnerMean InnerMedian Outer
    Avg k0       1         2         3   |  Var k0       3/2        3        9/4
        k1       3         4         6   |      k1       5/2        4       35/4
        k2       4         6         9   |      k2        7        13       37/2
    COV k0      NaN       NaN       1/2         (AA's NaN makes both NaN)
        k1      1/2       1/2   sqrt(35/4)/6
        k2  (1/2 + sqrt(13)/6)/2  sqrt(13)/6  sqrt(37/2)/9       (sqrt(13)/6 = 0.6009.. > 1/2)

Fits of Outer on Inner over the three k-mers, b = Sxy/Sxx, a = my - b mx, residual = y - (a + b x):

    AvgMean    x = 1 3 4, y = 3 6 9: mx = 8/3, my = 6, Sxy = 5 + 0 + 4 = 9, Sxx = (25 + 1 + 16)/9 = 14/3,
               b = 27/14, a = 6 - 36/7 = 6/7, residuals 3/14, -9/14, 3/7
    AvgMedian  x = 2 4 6, y = 3 6 9: mx = 4, my = 6, Sxy = 6 + 0 + 6 = 12, Sxx = 8, b = 3/2, a = 0, residuals 0 0 0
    VarMean    x = 3/2 5/2 7, y = 9/4 35/4 37/2: mx = 11/3, my = 59/6,
               Sxy = (-13/6)(-91/12) + (-7/6)(-13/12) + (10/3)(26/3) = 1183/72 + 91/72 + 2080/72 = 559/12,
               Sxx = 169/36 + 49/36 + 400/36 = 103/6, b = 559/206, a = 59/6 - (559/206)(11/3) = -12/103
               residuals 9/4 + 12/103 - 1677/412 = -351/206, 35/4 + 12/103 - 2795/412 = 429/206, 37/2 + 12/103 - 3913/206 = -39/103
    VarMedian  x = 3 4 13, y as above: mx = 20/3, my = 59/6,
               Sxy = (-11/3)(-91/12) + (-8/3)(-13/12) + (19/3)(26/3) = 1001/36 + 104/36 + 1976/36 = 3081/36 = 1027/12,
               Sxx = (121 + 64 + 361)/9 = 182/3, b = 1027/728 = 79/56, a = 59/6 - (79/56)(20/3) = 3/7
               residuals 9/4 - 3/7 - 237/56 = -135/56, 35/4 - 3/7 - 79/14 = 75/28, 37/2 - 3/7 - 1027/56 = -15/56
    COVMean, COVMedian   k0's Inner is NaN: intercept, slope and every residual are NaN

The golden file tests/golden/distill_small.json holds these 54 + 12 values (scaled by u or u^2) as hex floats, rounded once
from the exact fractions and from sqrt() of exact arguments."""
import math
from fractions import Fraction as F

import numpy as np

from conftest import load_golden, unhex

import distill_ref

COUNTS = np.array([[0, 0, 16], [1, 4, 11], [0, 1, 15], [4, 8, 4], [0, 3, 13], [4, 10, 2]], dtype=np.int32)  # [spectrum][k-mer]
CLASSES = [0, 1, 0, 1, 0, 1]
U, U2 = F(1, 16), F(1, 256)
NAN = float("nan")


def by_hand():
    """the tables of the docstring -> (out [18][3], fits [6][2]) as floats rounded once"""
    s13, s35, s37 = math.sqrt(13.0), math.sqrt(8.75), math.sqrt(18.5)
    rows = [
        [F(1) * U, F(3) * U, F(4) * U], [F(3) * U, F(6) * U, F(9) * U], [F(3, 14) * U, F(-9, 14) * U, F(3, 7) * U],
        [F(2) * U, F(4) * U, F(6) * U], [F(3) * U, F(6) * U, F(9) * U], [F(0), F(0), F(0)],
        [F(3, 2) * U2, F(5, 2) * U2, F(7) * U2], [F(9, 4) * U2, F(35, 4) * U2, F(37, 2) * U2],
        [F(-351, 206) * U2, F(429, 206) * U2, F(-39, 103) * U2],
        [F(3) * U2, F(4) * U2, F(13) * U2], [F(9, 4) * U2, F(35, 4) * U2, F(37, 2) * U2], [F(-135, 56) * U2, F(75, 28) * U2, F(-15, 56) * U2],
        [NAN, 0.5, (0.5 + s13 / 6) / 2], [0.5, s35 / 6, s37 / 9], [NAN, NAN, NAN],
        [NAN, 0.5, s13 / 6], [0.5, s35 / 6, s37 / 9], [NAN, NAN, NAN],
    ]
    fits = [[F(6, 7) * U, F(27, 14)], [F(0), F(3, 2)], [F(-12, 103) * U2, F(559, 206)], [F(3, 7) * U2, F(79, 56)], [NAN, NAN], [NAN, NAN]]
    return np.array([[float(v) for v in r] for r in rows]), np.array([[float(v) for v in r] for r in fits])


def same(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_golden_file_is_the_hand_computation():
    g = load_golden("distill_small.json")
    out, fits = by_hand()
    assert g["row_names"] == list(distill_ref.ROW_NAMES)
    assert g["counts"] == COUNTS.tolist() and g["classes"] == CLASSES
    assert same(unhex(g["out"], (18, 3)), out) and same(unhex(g["fits"], (6, 2)), fits)


def test_reference_matches_the_hand_computation():
    g = load_golden("distill_small.json")
    want, want_fits = unhex(g["out"], (18, 3)), unhex(g["fits"], (6, 2))
    out, fits = distill_ref.distill(COUNTS, CLASSES)
    assert np.array_equal(np.isnan(out), np.isnan(want)) and np.array_equal(np.isnan(fits), np.isnan(want_fits))
    names = distill_ref.ROW_NAMES
    for r, name in enumerate(names):
        if name.startswith("Residual") or np.isnan(want[r]).all():
            continue
        if "COV" in name:  # square roots and a quotient: a few roundings of their own
            np.testing.assert_allclose(out[r], want[r], rtol=4 * 2.0 ** -52, err_msg=name)
        else:  # sums and quotients of small dyadic numbers: exact
            assert np.array_equal(out[r], want[r]), name
    for f in range(4):
        x, y = want[6 * (f // 2) + 3 * (f % 2)], want[6 * (f // 2) + 3 * (f % 2) + 1]
        a, b = want_fits[f]
        np.testing.assert_allclose(fits[f], want_fits[f], rtol=1e-14, atol=1e-14 * np.abs(y).max())
        # a residual is a difference of numbers of the size of y: absolute, in roundings of that size
        bar = 16 * 2.0 ** -52 * (np.abs(y).max() + abs(a) + abs(b) * np.abs(x).max())
        assert np.all(np.abs(out[6 * (f // 2) + 3 * (f % 2) + 2] - want[6 * (f // 2) + 3 * (f % 2) + 2]) <= bar), names[6 * (f // 2) + 3 * (f % 2) + 2]
    # the k-mer with the all-zero class: its diagonal cell is 0/0
    keys, n, mean, var, cov = distill_ref.cells(COUNTS, CLASSES)
    assert keys == [(0, 0), (0, 1), (1, 1)] and n.tolist() == [3, 9, 3]
    assert mean[0, 0] == 0.0 and var[0, 0] == 0.0 and np.isnan(cov[0, 0])


def test_reference_edge_semantics():
    rng = np.random.default_rng(1)
    counts = rng.poisson(5.0, size=(7, 40)).astype(np.int32)
    for bad in ([0] * 7, list(range(7))):
        try:
            distill_ref.distill(counts, bad)
        except distill_ref.InvalidNumberOfClasses as e:
            assert "Invalid_number_of_classes(%d)" % (max(bad) + 1) in str(e)
        else:
            raise AssertionError("no error for classes %r" % (bad,))
    names = distill_ref.ROW_NAMES
    # a singleton class: its diagonal cell has no pair, every Inner row is NaN (and with them the residuals)
    out, _ = distill_ref.distill(counts, [0, 1, 1, 1, 2, 2, 2])
    for r, name in enumerate(names):
        assert np.isnan(out[r]).all() == (not name.startswith("Outer")), name
    # a class of two: one pair, a mean but no variance
    out, _ = distill_ref.distill(counts, [0, 0, 1, 1, 1, 2, 2])
    for r, name in enumerate(names):
        assert np.isnan(out[r]).all() == ("Avg" not in name and not name.startswith("Outer")), name
    # a spectrum that sums to zero: 0/0 everywhere it takes part, so in every row
    counts[3] = 0
    out, fits = distill_ref.distill(counts, [0, 0, 0, 1, 1, 2, 2])
    assert np.isnan(out).all() and np.isnan(fits).all()
