"""CPU restatement of the declared semantics of distill ("distill"; lib/KMerDB.ml:812-976), in plain numpy.

Written from the declaration, not from the HIP code: float64, two passes per cell (mean first, then the squared
deviations), a plain loop over all pairs of spectra in the reference's visiting order.  The k-mers are the vector axis.
tests/test_distill_ref.py pins it to a case worked out by hand."""
import numpy as np

ROW_NAMES = tuple("%s%s%s" % (part, quantity, across) for quantity in ("Avg", "Var", "COV")
                  for across in ("Mean", "Median") for part in ("Inner", "Outer", "Residual"))


class InvalidNumberOfClasses(ValueError):
    pass


def normalised(counts):
    """counts [S, K] int -> x [S, K]: count / linear column sum (threshold 1, power 1: only counts >= 1 are summed);
    a true division, 0 / 0 = NaN for a spectrum that sums to zero"""
    counts = np.asarray(counts)
    sums = np.where(counts >= 1, counts, 0).astype(np.float64).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return counts.astype(np.float64) / sums[:, None]


def cells(counts, classes, n_classes=None):
    """-> (keys, n, mean, var, cov): keys is the list of cells (a, b), a <= b, in the reference's order (:876-889: (0, 0),
    (0, 1) .. (0, C-1), (1, 1), ..); n[cell] the number of pairs; the others [n_cells, K]"""
    counts = np.asarray(counts)
    classes = [int(c) for c in classes]
    S, K = counts.shape
    C = (max(classes) + 1) if n_classes is None else int(n_classes)
    if C == 1 or C == S:
        raise InvalidNumberOfClasses("Invalid_number_of_classes(%d)" % C)
    x = normalised(counts)
    keys = [(a, b) for a in range(C) for b in range(a, C)]
    diffs = {k: [] for k in keys}
    for i in range(S):
        for j in range(i + 1, S):
            diffs[(min(classes[i], classes[j]), max(classes[i], classes[j]))].append(np.abs(x[i] - x[j]))
    n = np.array([len(diffs[k]) for k in keys])
    mean = np.full((len(keys), K), np.nan)
    var = np.full((len(keys), K), np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        for c, k in enumerate(keys):
            if n[c] >= 1:
                total = np.zeros(K)
                for d in diffs[k]:
                    total = total + d
                mean[c] = total / n[c]
            if n[c] >= 2:
                sq = np.zeros(K)
                for d in diffs[k]:
                    sq = sq + (d - mean[c]) * (d - mean[c])
                var[c] = sq / (n[c] - 1)
        cov = np.sqrt(var) / mean
    return keys, n, mean, var, cov


def across(values):
    """values [m, K] -> (Mean, Median) over the m cells: sum / m and sorted[m // 2] (lib/Matrix.ml:632-690); NaN where any
    of the m values is NaN"""
    m = values.shape[0]
    bad = np.isnan(values).any(axis=0)
    total = np.zeros(values.shape[1])
    for v in values:
        total = total + v
    with np.errstate(invalid="ignore"):
        mean = total / m
        med = np.sort(values, axis=0)[m // 2]
    mean[bad] = np.nan
    med[bad] = np.nan
    return mean, med


def linear_fit(x, y):
    """-> (intercept, slope, residuals); NaN anywhere makes all of it NaN"""
    with np.errstate(divide="ignore", invalid="ignore"):
        mx, my = x.sum() / x.size, y.sum() / y.size
        b = ((x - mx) * (y - my)).sum() / ((x - mx) * (x - mx)).sum()
        a = my - b * mx
        return a, b, y - (a + b * x)


def distill(counts, classes, n_classes=None):
    """counts [S, K] int, classes [S] -> (out [18, K] in the order of ROW_NAMES, fits [6, 2] = intercept, slope)"""
    keys, _, mean, var, cov = cells(counts, classes, n_classes)
    inner = np.array([a == b for a, b in keys])
    K = mean.shape[1]
    out = np.full((18, K), np.nan)
    fits = np.full((6, 2), np.nan)
    for q, values in enumerate((mean, var, cov)):
        (i_mean, i_med), (o_mean, o_med) = across(values[inner]), across(values[~inner])
        for m, (xi, yo) in enumerate(((i_mean, o_mean), (i_med, o_med))):
            row = 6 * q + 3 * m
            out[row], out[row + 1] = xi, yo
            fits[2 * q + m, 0], fits[2 * q + m, 1], out[row + 2] = linear_fit(xi, yo)
    return out, fits
