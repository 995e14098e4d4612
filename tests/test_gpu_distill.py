"""GPU tests of distill (KPopCountDB -d; kpop_counter_distill / kpop_dev_counter_distill) against tests/distill_ref.py, the
plain numpy restatement of the semantics declared in INTEGRATION.md.

The bars are derived, not tuned:
  * NaN where and only where the reference has NaN; a reference value of exactly zero is exactly zero;
  * Avg rows: 1e-12 relative, the project's bar for f64 reductions (tests/test_gpu_counter.py);
  * Var and COV rows: max(1e-12, 4 n_max 2^-53 (1 + kappa)) relative -- n_max the pair count of the largest cell, kappa the
    largest mean^2 / var over the cells, both taken from the reference: what a one-pass sum of squares may lose.  Means
    and order statistics over cells are 1-Lipschitz in the cell values and inherit the bar;
  * Residual rows: 1e-12 (max|y| + |a| + |b| max|x|) absolute, from the reference's own fit;
  * fits: 1e-10 relative."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_cli import BIN

import distill_ref

pytestmark = pytest.mark.gpu

NAMES = distill_ref.ROW_NAMES
COUNTDB = os.path.join(BIN, "KPopCountDB")
COUNT = os.path.join(BIN, "KPopCount")


def poisson_db(seed, n_spectra, n_kmers, lam):
    return np.random.default_rng(seed).poisson(lam, size=(n_spectra, n_kmers)).astype(np.int32)


def conditioning(counts, classes):
    """-> (n_max, kappa) of the reference's cells"""
    _, n, mean, var, _ = distill_ref.cells(counts, classes)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = (mean * mean / var).ravel()  # 0/0 (an all-zero cell: nothing to lose) and cells without a variance are NaN
    k = k[~np.isnan(k)]
    return int(n.max()), float(k.max()) if k.size else 0.0


def rel_err(got, want):
    ok = np.isfinite(want) & (want != 0)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]))) if ok.any() else 0.0


def check_rows(got, want, want_fits, n_max, kappa, rows=range(18), what=""):
    """the bars of the module docstring on the given rows; prints every figure before it asserts"""
    var_bar = max(1e-12, 4.0 * n_max * 2.0 ** -53 * (1.0 + kappa))
    failures = []
    for r in rows:
        name = NAMES[r]
        g, w = got[r], want[r]
        if not np.array_equal(np.isnan(g), np.isnan(w)):
            failures.append("%s: NaN at %d places, the reference at %d" % (name, int(np.isnan(g).sum()), int(np.isnan(w).sum())))
            continue
        if not np.all(g[w == 0] == 0):
            failures.append("%s: a reference zero is not zero" % name)
        if name.startswith("Residual"):
            f = 2 * (r // 6) + (r % 6) // 3
            x, y = want[r - 2], want[r - 1]
            a, b = want_fits[f]
            if np.isnan(w).all():
                continue
            bar = 1e-12 * (np.abs(y).max() + abs(a) + abs(b) * np.abs(x).max())
            err = float(np.max(np.abs(g - w)))
        else:
            bar = 1e-12 if "Avg" in name else var_bar
            err = rel_err(g, w)
        print("%s %-18s err %.3e bar %.3e" % (what, name, err, bar))
        if not err <= bar:
            failures.append("%s: %.3e over the bar %.3e" % (name, err, bar))
    assert not failures, failures


def check_fits(got_fits, want_fits, what=""):
    assert np.array_equal(np.isnan(got_fits), np.isnan(want_fits)), (got_fits, want_fits)
    err = rel_err(got_fits, want_fits)
    print("%s fits err %.3e bar 1e-10" % (what, err))
    assert err <= 1e-10, (got_fits, want_fits)


def check_against_reference(kpop, counts, classes, what=""):
    want, want_fits = distill_ref.distill(counts, classes)
    n_max, kappa = conditioning(counts, classes)
    print("%s n_max %d kappa %.3g" % (what, n_max, kappa))
    got, got_fits = kpop.counter_distill(list(counts), classes)
    assert got.shape == want.shape and got_fits.shape == (6, 2)
    check_rows(got, want, want_fits, n_max, kappa, what=what)
    check_fits(got_fits, want_fits, what=what)
    return kappa


def interleaved(n_spectra, n_classes):
    return [i % n_classes for i in range(n_spectra)]


def unequal_3_5_17():
    order = np.random.default_rng(42).permutation(25)
    sizes = np.repeat([0, 1, 2], [3, 5, 17])[order]
    seen = {}
    return [seen.setdefault(int(c), len(seen)) for c in sizes]  # numbered by first appearance, sizes in whatever order


PARITY = {
    "12x3": (lambda: poisson_db(11, 12, 500, 3.0), lambda: interleaved(12, 3)),
    "40x4": (lambda: poisson_db(12, 40, 2000, 20.0), lambda: interleaved(40, 4)),
    "30x5-sparse": (lambda: poisson_db(13, 30, 1000, 0.3), lambda: interleaved(30, 5)),
    "3-5-17": (lambda: poisson_db(14, 25, 777, 5.0), unequal_3_5_17),
    "130x10": (lambda: poisson_db(15, 130, 300, 8.0), lambda: interleaved(130, 10)),
}


@pytest.mark.parametrize("shape", sorted(PARITY))
def test_parity_with_the_reference(kpop, shape):
    counts, classes = PARITY[shape][0](), PARITY[shape][1]()
    kappa = check_against_reference(kpop, counts, classes, what=shape)
    assert kappa <= 1e3, kappa  # the bar above stays a bar: no cell is let off


def test_classes_longer_than_a_chunk_and_more_cells_than_the_sort_holds(kpop):
    """beyond the shapes of the parity test: classes of 40 go through the cell kernel in chunks of 32 (a triangle and
    rectangles across chunks); 30 classes have 435 off-diagonal cells, more than a thread of the reduce kernel sorts in LDS
    (a wavefront selects among them in registers); 102 classes have more than a wavefront holds (the bit-serial selection)"""
    check_against_reference(kpop, poisson_db(21, 80, 200, 6.0), interleaved(80, 2), what="80x2")
    check_against_reference(kpop, poisson_db(22, 75, 150, 6.0), [0] * 35 + [1] * 33 + [2] * 7, what="35-33-7")
    check_against_reference(kpop, poisson_db(23, 90, 150, 10.0), interleaved(90, 30), what="90x30")
    check_against_reference(kpop, poisson_db(24, 204, 70, 10.0), interleaved(204, 102), what="204x102")


def test_edge_semantics(kpop):
    counts = poisson_db(31, 9, 400, 12.0)
    # a singleton class: no pair in its diagonal cell, every Inner row (and every residual) is NaN
    classes = [0, 1, 1, 1, 1, 2, 2, 2, 2]
    got, _ = kpop.counter_distill(list(counts), classes)
    for r, name in enumerate(NAMES):
        assert np.isnan(got[r]).all() == (not name.startswith("Outer")), name
    check_against_reference(kpop, counts, classes, what="singleton")
    # a class of two: one pair, a mean and no variance
    classes = [0, 0, 1, 1, 1, 1, 2, 2, 2]
    got, _ = kpop.counter_distill(list(counts), classes)
    for r, name in enumerate(NAMES):
        assert np.isnan(got[r]).all() == ("Avg" not in name and not name.startswith("Outer")), name
        assert np.isfinite(got[r]).all() == ("Avg" in name or name.startswith("Outer")), name
    check_against_reference(kpop, counts, classes, what="pair")
    # a spectrum that sums to zero is 0/0 wherever it takes part
    empty = counts.copy()
    empty[4] = 0
    got, fits = kpop.counter_distill(list(empty), [0, 0, 0, 1, 1, 1, 2, 2, 2])
    assert np.isnan(got).all() and np.isnan(fits).all()
    want, _ = distill_ref.distill(empty, [0, 0, 0, 1, 1, 1, 2, 2, 2])
    assert np.isnan(want).all()
    # the number of classes
    for bad in ([0] * 9, list(range(9))):
        with pytest.raises(kpop.KPopError, match=r"Invalid_number_of_classes\(%d\)" % (max(bad) + 1)):
            kpop.counter_distill(list(counts), bad)
        with pytest.raises(distill_ref.InvalidNumberOfClasses):
            distill_ref.distill(counts, bad)
    with pytest.raises(kpop.KPopError):  # a class index out of range
        kpop.counter_distill(list(counts), [0, 0, 0, 1, 1, 1, 2, 2, 3], n_classes=3)
    with pytest.raises(kpop.KPopError):  # an empty class
        kpop.counter_distill(list(counts), [0, 0, 0, 0, 0, 2, 2, 2, 2], n_classes=3)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_invariances_at_k12_size(kpop):
    """every canonical 12-mer (8,390,656 rows), 24 spectra in 4 classes"""
    K, S, n_classes = 8390656, 24, 4
    rng = np.random.default_rng(5)
    counts = [rng.poisson(6.0, size=K).astype(np.int32) for _ in range(S)]  # (no class of six is all zero at any k-mer: every fit is finite)
    classes = interleaved(S, n_classes)
    out, fits = kpop.counter_distill(counts, classes)
    again, fits2 = kpop.counter_distill(counts, classes)
    assert np.array_equal(bits(out), bits(again)) and np.array_equal(bits(fits), bits(fits2))
    del again
    doubled = list(counts)
    doubled[7] = counts[7] * 2  # the normalised counts are the same numbers
    again, fits2 = kpop.counter_distill(doubled, classes)
    assert np.array_equal(bits(out), bits(again)) and np.array_equal(bits(fits), bits(fits2))
    del again, doubled
    assert np.isfinite(fits).all()
    # 2,000 k-mers at random against the reference run on those rows alone (with the whole database's column sums: a
    # k-mer's Inner and Outer rows depend on nothing else)
    pick = np.sort(rng.choice(K, size=2000, replace=False))
    sums = np.array([c.astype(np.int64).sum() for c in counts], dtype=np.float64)
    sub = np.array([c[pick] for c in counts])
    real_normalised = distill_ref.normalised
    distill_ref.normalised = lambda c: np.asarray(c).astype(np.float64) / sums[:, None]
    try:
        want, want_fits = distill_ref.distill(sub, classes)
        n_max, kappa = conditioning(sub, classes)
    finally:
        distill_ref.normalised = real_normalised
    print("k12 n_max %d kappa %.3g" % (n_max, kappa))
    inner_outer = [r for r in range(18) if not NAMES[r].startswith("Residual")]
    check_rows(out[:, pick], want, want_fits, n_max, kappa, rows=inner_outer, what="k12")
    # the residual rows from the GPU's own Inner and Outer rows and fits
    for f in range(6):
        row = 6 * (f // 2) + 3 * (f % 2)
        x, y, (a, b) = out[row], out[row + 1], fits[f]
        res = y - (a + b * x)
        bar = 1e-12 * (np.abs(y).max() + abs(a) + abs(b) * np.abs(x).max())
        err = float(np.max(np.abs(out[row + 2] - res)))
        print("k12 %-18s err %.3e bar %.3e" % (NAMES[row + 2], err, bar))
        assert err <= bar, NAMES[row + 2]


def test_device_form_on_a_stream_and_in_bands(kpop):
    """kpop_dev_counter_distill on a stream of the caller's, in a workspace of exactly the size asked for: the host form's
    bits; and again in several bands (kpop_tune("distill_band")): the same bits"""
    import torch
    from kpop_amd import _lib, api
    L = _lib.load()
    S, n_classes, K = 26, 3, 5000
    counts = poisson_db(41, S, K, 4.0)
    classes = interleaved(S, n_classes)
    want, want_fits = kpop.counter_distill(list(counts), classes)
    dev = torch.device("cuda", 0)
    ld = int(L.kpop_dev_counter_ld(K))
    storage = torch.zeros((S, ld), dtype=torch.int32, device=dev)
    storage[:, :K] = torch.from_numpy(counts).to(dev)
    d_classes = torch.tensor(classes, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.kpop_dev_counter_distill_workspace_bytes(S, K, n_classes)), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    try:
        for band in (0, 1700, 128):  # one band; 3 bands (1,792 k-mers each); 40 bands
            api.tune("distill_band", band)
            out = torch.full((18, K), -1.0, dtype=torch.float64, device=dev)
            fits = np.full((6, 2), -1.0)
            rc = L.kpop_dev_counter_distill(storage.data_ptr(), ld, S, K, d_classes.data_ptr(), n_classes, ws.data_ptr(), out.data_ptr(),
                                            fits.ctypes.data_as(C.POINTER(C.c_double)), stream.cuda_stream)
            assert rc == 0, L.kpop_last_error()
            stream.synchronize()
            assert np.array_equal(bits(out.cpu().numpy()), bits(want)), band
            assert np.array_equal(bits(fits), bits(want_fits)), band
    finally:
        api.tune("distill_band", 0)
    bad = torch.tensor([0] * S, dtype=torch.int32, device=dev)
    assert L.kpop_dev_counter_distill(storage.data_ptr(), ld, S, K, bad.data_ptr(), 1, ws.data_ptr(), out.data_ptr(), None, stream.cuda_stream) != 0
    assert b"Invalid_number_of_classes(1)" in L.kpop_last_error()


@pytest.mark.skipif(not os.path.exists(COUNTDB), reason="host CLIs not built")
def test_cli_distill(tmp_path, pyref):
    k = 4
    rng = np.random.default_rng(8)
    seqs = [("s%d" % i, "".join(rng.choice(list("ACGT"), size=int(rng.integers(200, 500))))) for i in range(10)]
    with open(tmp_path / "x.fa", "w") as f:
        for tag, seq in seqs:
            f.write(">%s\n%s\n" % (tag, seq))
    group = ["abc"[i % 3] for i in range(10)]  # 4 / 3 / 3
    (tmp_path / "meta.txt").write_text("label\tclass\tsite\n" + "".join("s%d\t%s\tnorth\n" % (i, group[i]) for i in range(10)))
    penv = dict(os.environ, PATH=BIN + ":" + os.environ.get("PATH", ""))
    sh = lambda cmd: subprocess.run(["bash", "-c", cmd], cwd=str(tmp_path), capture_output=True, text=True, timeout=300, env=penv)
    assert sh("KPopCount -k %d -L -f x.fa -o spectra" % k).returncode == 0
    r = sh("KPopCountDB -k spectra -m meta.txt -d class ranking -v")
    assert r.returncode == 0, r.stderr
    fit_lines = [l for l in r.stderr.splitlines() if "Fit for" in l]
    assert len(fit_lines) == 6 and all(" * x" in l for l in fit_lines), r.stderr
    assert [l.split("Fit for ")[1].split(" is ")[0] for l in fit_lines] == ["avgs mean", "avgs median", "vars mean", "vars median", "covs mean",
                                                                           "covs median"]
    # the database as KPopCountDB holds it: k-mers in order of first appearance, a spectrum's own in ascending order
    spectra = [pyref.count_read(s, k) for _, s in seqs]
    rows = []
    for sp in spectra:
        rows += [h for h in sorted(sp) if h not in rows]
    counts = np.array([[sp.get(h, 0) for h in rows] for sp in spectra], dtype=np.int32)
    classes = [ord(g) - ord("a") for g in group]
    lines = (tmp_path / "ranking.KPopDistill.txt").read_text().splitlines()
    assert lines[0].split("\t") == ['""'] + ['"%s"' % n for n in NAMES]
    assert [l.split("\t")[0] for l in lines[1:]] == ['"%s"' % pyref.to_hex(h, k) for h in rows]
    got = np.array([[float(v) for v in l.split("\t")[1:]] for l in lines[1:]]).T
    want, want_fits = distill_ref.distill(counts, classes)
    n_max, kappa = conditioning(counts, classes)
    print("cli n_max %d kappa %.3g" % (n_max, kappa))
    check_rows(got, want, want_fits, n_max, kappa, what="cli")  # (the 15 digits of the print are far inside the bars)
    for line, (a, b) in zip(fit_lines, want_fits):
        ga, gb = float(line.split(" is ")[1].split(" + ")[0]), float(line.split(" + ")[1].split(" * x")[0])
        if np.isnan(a):  # (a k-mer whose Inner COV is 0/0: the reference's fit is NaN too)
            assert np.isnan(ga) and np.isnan(gb), line
            continue
        assert abs(ga - a) <= 5.1e-6 * abs(a) and abs(gb - b) <= 5.1e-6 * abs(b), line  # (%.6g: half a unit of the sixth digit)
    # -d runs where it stands among the actions: after -c there are as many classes as spectra
    r = sh("KPopCountDB -k spectra -m meta.txt -c class -d class late")
    assert r.returncode == 1 and "Invalid_number_of_classes(3)" in r.stderr
    r = sh("KPopCountDB -k spectra -m meta.txt -d class /dev/stdout")
    assert r.returncode == 0 and r.stdout.splitlines() == lines
    r = sh("KPopCountDB -k spectra -m meta.txt -d nothere out")
    assert r.returncode == 1 and "Classes_label_not_found" in r.stderr
    r = sh("KPopCountDB -k spectra -m meta.txt -d site out")
    assert r.returncode == 1 and "Invalid_number_of_classes(1)" in r.stderr
