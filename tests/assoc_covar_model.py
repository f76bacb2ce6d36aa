"""The contract of the association scan with covariates (include/dbtk_assoc_covar.h) in numpy float64, on top of tests/assoc_model.py:
the partial correlation of every (row, phenotype) pair given the covariates and the intercept.  tests/test_assoc_covar_model.py pins it
to the multiple regression y ~ 1 + C + x (numpy lstsq, scipy's t tail)."""
import math

import numpy as np

import assoc_model
from assoc_model import NONE, U, bh, locus_of, pvalue, row_stats

COLLINEAR = 1e-6
COVAR_MAX = 128


def basis(covar):
    """covar[q][n] (the samples in the order of the rows of Q wanted) -> Q[q][n]: an orthonormal basis of the centred columns, by
    np.linalg.qr.  ValueError("covariate j ...") on a column that is constant or whose share left by the columns before it is <= COLLINEAR."""
    covar = np.asarray(covar, np.float64)
    q, n = covar.shape
    if not q:
        return np.zeros((0, n))
    c = covar - covar.sum(axis=1, keepdims=True) / n
    for j in range(q):
        if not np.isfinite(covar[j]).all() or covar[j].min() == covar[j].max():
            raise ValueError(f"covariate {j} is constant or not finite")
    Qm, R = np.linalg.qr(c.T)
    for j in range(q):
        if not R[j, j] ** 2 > COLLINEAR * float((c[j] * c[j]).sum()):
            raise ValueError(f"covariate {j} is collinear")
    return np.ascontiguousarray(Qm.T)


def partial(G, sample_of, pheno, covar, Q=None):
    """r[nrows][P] (nan on rows that are not tested), tested[nrows], share_x[nrows] = Sxx' / Sxx (nan where the row fails the two
    tests of the plain scan), share_y[P] = Syy' / Syy.  covar[q][n] lists sample j = sample_of[j], as pheno does; Q[q][n], when given,
    is over the samples in ASCENDING order (what dbtk_assoc_covar_basis makes of the sorted columns)."""
    order = np.argsort(np.asarray(sample_of, np.int64), kind="stable")
    n = len(order)
    y = np.asarray(pheno, np.float64).reshape(-1, n)[:, order]
    covar = np.asarray(covar, np.float64).reshape(-1, n)[:, order]
    q = covar.shape[0]
    if Q is None:
        Q = basis(covar)
    Q = np.asarray(Q, np.float64).reshape(q, n)
    x, tested, dx, sxx = row_stats(G, sample_of)
    dy = y - y.sum(axis=1, keepdims=True) / n
    syy = (dy * dy).sum(axis=1)
    sxy = np.stack([(dx * dy[p]).sum(axis=1) for p in range(len(dy))], axis=1)   # (as assoc_model.correlations sums it)
    sxx_left, syy_left, sxy_left = sxx.copy(), syy.copy(), sxy.copy()
    for j in range(q):                                                             # j ascending, the three in the same order
        a = (dx * Q[j]).sum(axis=1)
        b = (dy * Q[j]).sum(axis=1)
        sxx_left = sxx_left - a * a
        syy_left = syy_left - b * b
        sxy_left = sxy_left - a[:, None] * b[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        share_x = np.where(tested, sxx_left / np.where(tested, sxx, 1.0), np.nan)
        share_y = syy_left / syy
        if q:
            tested = tested & (sxx_left > COLLINEAR * sxx)
        r = sxy_left / np.sqrt(sxx_left[:, None] * syy_left[None, :])
    r = np.clip(r, -1.0, 1.0)
    r[~tested] = np.nan
    return r, tested, share_x, share_y


def scan(G, sample_of, pheno, covar, Q=None, nk_cum=None, pairs=None, p_threshold=None):
    """What assoc_model.scan returns (best, hits, r, tested, paired) with dof = n - 2 - q, plus share_x[nrows] and share_y[P].  A
    phenotype whose share_y <= COLLINEAR raises ValueError (the library refuses it by name); so does n < q + 3 or q > COVAR_MAX."""
    n = len(sample_of)
    q = np.asarray(covar, np.float64).reshape(-1, n).shape[0]
    if n < q + 3 or q > COVAR_MAX:
        raise ValueError("n < q + 3 or q > COVAR_MAX")
    r, tested, share_x, share_y = partial(G, sample_of, pheno, covar, Q)
    if q and not (share_y > COLLINEAR).all():
        raise ValueError(f"phenotype {int(np.argmin(share_y))} is explained by the covariates")
    nrows, P = r.shape
    neff, dof = n - q, n - 2 - q
    paired = np.zeros((nrows, P), bool)
    if pairs is None:
        paired[:] = True
    else:
        off, idx = pairs
        for l in range(len(off) - 1):
            r0, r1 = (int(nk_cum[l - 1]) if l else 0), int(nk_cum[l])
            for p in set(int(v) for v in idx[off[l]:off[l + 1]]):
                paired[r0:r1, p] = True

    def stats(rr):
        se = math.sqrt((1.0 - rr * rr) / dof)
        return se, (rr / se if se else math.copysign(math.inf, rr)), pvalue(rr, neff)

    best = []
    for p in range(P):
        use = paired[:, p] & tested
        b = dict(n_tests=int(use.sum()), skipped=int((paired[:, p] & ~tested).sum()), row=NONE, locus=NONE, r=0.0, se=0.0, t=0.0, p=0.0, p_bonf=0.0, q=0.0)
        if b["n_tests"]:
            r2 = np.where(use, r[:, p] * r[:, p], -1.0)
            row = int(np.argmax(r2))  # (the first of the largest)
            rr = float(r[row, p])
            se, t, pv = stats(rr)
            b.update(row=row, locus=locus_of(nk_cum, row), r=rr, se=se, t=t, p=pv)
            b["p_bonf"] = b["p"] * b["n_tests"]
        best.append(b)
    have = [p for p in range(P) if best[p]["n_tests"]]
    for p, qv in zip(have, bh([best[p]["p_bonf"] for p in have])):
        best[p]["q"] = float(qv)
    hits = None
    if p_threshold is not None:
        hits = []
        for p in range(P):
            for row in np.nonzero(paired[:, p] & tested)[0]:
                rr = float(r[row, p])
                se, t, pv = stats(rr)
                if pv <= p_threshold:
                    hits.append((p, locus_of(nk_cum, int(row)), int(row), rr, t, pv))
    return dict(best=best, hits=hits, r=r, tested=tested, paired=paired, share_x=share_x, share_y=share_y)


def tolerance(G, sample_of, pheno, q, share_x, share_y):
    """The bound on |r_device - r_model| per row (tests/test_assoc_covar_gpu.py derives it):
    4 [(n + 4)(1 + 2 sqrt(q)) + q] 2^-53 (1 + kappa) / min(share of the row, smallest share of a phenotype); 0 on rows without a share.
    With q = 0 it is assoc_model.tolerance."""
    base = assoc_model.tolerance(G, sample_of, pheno)      # 4 (n + 4) U (1 + kappa), 0 on rows that are not tested
    n = len(sample_of)
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.minimum(np.where(np.isfinite(share_x) & (share_x > 0), share_x, np.inf), float(np.min(share_y)) if q else 1.0)
        per_n = base / (4.0 * (n + 4) * U)
        return np.where(np.isfinite(rho), 4.0 * ((n + 4) * (1.0 + 2.0 * math.sqrt(q)) + q) * U * per_n / rho, 0.0)


best_tsv = assoc_model.best_tsv


def hits_tsv(names, hits):
    out = ["pheno\tlocus\trow\tr\tt\tp"]
    for p, locus, row, r, t, pv in hits:
        out.append("\t".join([names[p], "NA" if locus == NONE else str(locus), str(row), assoc_model.fmt(r), assoc_model.fmt(t), assoc_model.fmt(pv)]))
    return "\n".join(out) + "\n"
