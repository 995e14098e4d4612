"""numpy restatement of the correspondence analysis KPopTwist runs in R (src/KPopTwist:93-116, library `ca`).

TEST INFRASTRUCTURE ONLY.  PARITY UNPINNED: R is not available here, so this restates the published
algorithm of ca::ca / ca::cacoord (Nenadic & Greenacre) as the wrapper uses it:
    stuff   <- per-column normalised counts               (:93-94)
    ca(stuff): P = N/sum(N); r, c masses; S = D_r^-1/2 (P - r c') D_c^-1/2; S = U diag(sv) V'
    twisted <- cacoord(cols=TRUE)  = principal column coordinates  D_c^-1/2 V diag(sv)     (:98-100)
    inertia <- sv^2 / sum(sv^2)                                                       (:105)
    twister <- t(cacoord(rows=TRUE) / sv) = standard row coordinates' = (D_r^-1/2 U)'   (:110-116)
with nd = min(I, J) - 1 dimensions.  The sign of every dimension is arbitrary (LAPACK).
"""
import numpy as np


def ca(counts, normalize=True):
    """counts: I x J (k-mers x spectra).  -> twisted (J x nd), inertia (nd), twister (nd x I)."""
    N = np.asarray(counts, dtype=np.float64)
    I, J = N.shape
    if normalize:
        N = N / N.sum(axis=0, keepdims=True)
    P = N / N.sum()
    r = P.sum(axis=1)
    c = P.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        S = (P - np.outer(r, c)) / np.sqrt(np.outer(r, c))
    S[~np.isfinite(S)] = 0.0  # k-mers seen in no spectrum carry no mass
    U, sv, Vt = np.linalg.svd(S, full_matrices=False)
    nd = min(I, J) - 1
    sv, U, V = sv[:nd], U[:, :nd], Vt.T[:, :nd]
    with np.errstate(divide="ignore", invalid="ignore"):
        rowstd = U / np.sqrt(r)[:, None]
    rowstd[~np.isfinite(rowstd)] = 0.0
    twisted = V / np.sqrt(c)[:, None] * sv
    inertia = sv ** 2 / np.sum(sv ** 2)
    return twisted, inertia, rowstd.T.copy()


def _standardised(counts, normalize):
    """P's masses and the standardised residuals S of a count table, as ca() forms them"""
    N = np.asarray(counts, dtype=np.float64)
    if normalize:
        N = N / N.sum(axis=0, keepdims=True)
    P = N / N.sum()
    r = P.sum(axis=1)
    c = P.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        S = (P - np.outer(r, c)) / np.sqrt(np.outer(r, c))
    S[~np.isfinite(S)] = 0.0
    return r, c, S


def ca_gram(counts, normalize=True):
    """The same analysis by the route the GPU takes, in numpy f64: G = S'S, its eigenvectors V (numpy.linalg.eigh, by decreasing
    eigenvalue), sv = sqrt(eigenvalue), W = V / sv (0 where sv = 0), U = S W.  -> twisted, inertia, twister as ca() gives them."""
    r, c, S = _standardised(counts, normalize)
    I, J = S.shape
    nd = min(I, J) - 1
    lam, V = np.linalg.eigh(S.T @ S)
    order = np.argsort(-lam, kind="stable")[:nd]
    sv = np.sqrt(np.maximum(lam[order], 0.0))
    V = V[:, order]
    with np.errstate(divide="ignore", invalid="ignore"):
        W = np.where(sv > 0.0, V / sv, 0.0)
        rowstd = (S @ W) / np.sqrt(r)[:, None]
    rowstd[~np.isfinite(rowstd)] = 0.0
    twisted = V / np.sqrt(c)[:, None] * sv
    total = np.sum(sv ** 2)
    inertia = sv ** 2 / total if total > 0.0 else np.zeros(nd)
    return twisted, inertia, rowstd.T.copy()


def invariants(counts, normalize, twisted, inertia, twister, sigma=None):
    """How far (twisted, inertia, twister) are from BEING a singular value decomposition of the table's standardised residuals
    S = U diag(sigma) V' -- properties that hold for every valid choice of signs and of bases inside equal singular values, so
    nothing here depends on a gap between two of them.  With r, c the masses, T the twister, kappa_d = sigma_1 / sigma_d from
    the reference sigma (numpy.linalg.svd(S, compute_uv=False) unless given) and the dimensions with kappa_d <= 1e3 `live`:
      orthT   max over live d, e of |(T diag(r) T' - I)_de| / (kappa_d kappa_e)      (U'U = I; the Gram route loses kappa_d kappa_e)
      orthV   M = twisted' diag(c) twisted; max over live d != e of |M_de| / sqrt(M_dd M_ee)
      lam     max over live d of |M_dd - sigma_d^2| / sigma_1^2
      lamT    the same with |S' u_d|^2, u_d = sqrt(r) T_d, in the place of M_dd      (ties every twister row to ITS singular value)
      inertia max over all d of |inertia_d - M_dd / sum(M)| and, over live d, of |inertia_d - |S' u_d|^2 / sum(sigma^2)|
      rec     |(T' twisted' - (P - r c') / (r c')) o sqrt(r c')|_F / |S|_F  over ALL dimensions, rows with mass
    and: finite (every output), inertia_sum = |sum(inertia) - 1|, inertia_rise = the largest increase along inertia (0 if none),
    massless_rows_zero (twister columns of k-mers without mass are exactly zero), live (their number), sigma, kappa."""
    r, c, S = _standardised(counts, normalize)
    I, J = S.shape
    nd = min(I, J) - 1
    T = np.asarray(twister, dtype=np.float64)
    tw = np.asarray(twisted, dtype=np.float64)
    inertia = np.asarray(inertia, dtype=np.float64)
    assert T.shape == (nd, I) and tw.shape == (J, nd) and inertia.shape == (nd,)
    out = {"finite": bool(np.all(np.isfinite(T)) and np.all(np.isfinite(tw)) and np.all(np.isfinite(inertia)))}
    sigma = np.linalg.svd(S, compute_uv=False)[:nd] if sigma is None else np.asarray(sigma, dtype=np.float64)[:nd]
    with np.errstate(divide="ignore"):
        kappa = np.where(sigma > 0.0, sigma[0] / sigma, np.inf)
    live = kappa <= 1e3
    kl = kappa[live]
    out.update(sigma=sigma, kappa=kappa, live=int(live.sum()))
    with np.errstate(invalid="ignore", over="ignore"):
        Tl = T[live]
        A = (Tl * r) @ Tl.T - np.eye(len(kl))
        out["orthT"] = float(np.max(np.abs(A) / np.outer(kl, kl)))
        M = (tw.T * c) @ tw
        dM = np.diag(M).copy()
        Ml = M[np.ix_(live, live)]
        cos = np.abs(Ml) / np.sqrt(np.outer(dM[live], dM[live]))
        np.fill_diagonal(cos, 0.0)
        out["orthV"] = float(np.max(cos))
        out["lam"] = float(np.max(np.abs(dM[live] - sigma[live] ** 2)) / sigma[0] ** 2)
        back = np.sum(((Tl * np.sqrt(r)) @ S) ** 2, axis=1)  # |S' u_d|^2
        out["lamT"] = float(np.max(np.abs(back - sigma[live] ** 2)) / sigma[0] ** 2)
        out["inertia"] = float(np.max([np.max(np.abs(inertia - dM / dM.sum())), np.max(np.abs(inertia[live] - back / np.sum(sigma ** 2)))]))
        out["inertia_sum"] = float(abs(inertia.sum() - 1.0))
        out["inertia_rise"] = float(max(0.0, np.max(np.diff(inertia)))) if nd > 1 else 0.0
        mass = r > 0.0
        E = (T[:, mass].T * np.sqrt(r[mass])[:, None]) @ (tw * np.sqrt(c)[:, None]).T - S[mass]
        out["rec"] = float(np.linalg.norm(E) / np.linalg.norm(S))
    out["massless_rows_zero"] = bool(np.all(T[:, ~mass] == 0.0))
    for k in ("orthT", "orthV", "lam", "lamT", "inertia", "rec"):
        if not np.isfinite(out[k]):
            out[k] = np.inf  # (a NaN compares False with everything: as a defect it is infinite)
    return out


def align_signs(a, ref, axis):
    """Flip the sign of each dimension of `a` (dimension index along `axis`) to match `ref`."""
    a = np.array(a, dtype=np.float64, copy=True)
    dot = np.sum(a * ref, axis=1 - axis)
    s = np.where(dot < 0, -1.0, 1.0)
    return a * (s[None, :] if axis == 1 else s[:, None])
