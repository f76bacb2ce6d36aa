"""The contract of the association scan (include/dbtk_assoc.h) in numpy float64: numpy and the standard library only, so that the GPU
tests can use it anywhere.  tests/test_assoc_model.py pins it to scipy (linregress on the z-scored pair, false_discovery_control)."""
import math

import numpy as np

NONE = 0xFFFFFFFF
U = 2.0 ** -53


def _betacf(a, b, x):
    """continued fraction of the regularised incomplete beta function (modified Lentz)"""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 20000):
        m2 = 2.0 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        de = d * c
        h *= de
        if abs(de - 1.0) < 1e-16:
            break
    return h


def pvalue(r, n):
    """two-sided Student-t tail with n - 2 degrees of freedom of t = r sqrt((n - 2) / (1 - r^2)) = I_{1 - r^2}((n - 2) / 2, 1 / 2); 0 at |r| = 1"""
    ar = abs(float(r))
    if ar >= 1.0:
        return 0.0
    a, b = 0.5 * (n - 2), 0.5
    x, y = (1.0 - ar) * (1.0 + ar), ar * ar
    lnfront = math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + (b * math.log(y) if y > 0 else 0.0)
    if y == 0.0:
        return 1.0
    if x < (a + 1.0) / (a + b + 2.0):
        return min(1.0, math.exp(lnfront) * _betacf(a, b, x) / a)
    return min(1.0, max(0.0, 1.0 - math.exp(lnfront) * _betacf(b, a, y) / b))


def bh(p):
    """Benjamini-Hochberg (statsmodels fdrcorrection, scipy false_discovery_control): clipped at 1"""
    p = np.asarray(p, np.float64)
    m = len(p)
    if not m:
        return p.copy()
    order = np.argsort(p, kind="stable")
    v = p[order] * m / np.arange(1, m + 1)
    v = np.minimum.accumulate(v[::-1])[::-1]
    q = np.empty(m)
    q[order] = np.minimum(v, 1.0)
    return q


def row_stats(G, sample_of):
    """x (float64, the mask's samples in ascending order), tested, centred x, Sxx of every row of the float32 matrix G[nrows][ns]"""
    cols = np.sort(np.asarray(sample_of, np.int64))
    x = np.asarray(G, np.float32)[:, cols].astype(np.float64)
    fin = np.isfinite(x).all(axis=1)
    with np.errstate(invalid="ignore"):
        tested = fin & (x.min(axis=1) != x.max(axis=1))
    xs = np.where(tested[:, None], x, 0.0)
    d = xs - xs.sum(axis=1, keepdims=True) / x.shape[1]
    return x, tested, d, (d * d).sum(axis=1)


def correlations(G, sample_of, pheno):
    """r[nrows][P] (nan on rows that are not tested) and tested[nrows]"""
    order = np.argsort(np.asarray(sample_of, np.int64), kind="stable")
    y = np.asarray(pheno, np.float64).reshape(-1, len(order))[:, order]
    x, tested, dx, sxx = row_stats(G, sample_of)
    n = x.shape[1]
    dy = y - y.sum(axis=1, keepdims=True) / n
    syy = (dy * dy).sum(axis=1)
    # (Sxy summed like Sxx and Syy, a row at a time in numpy's one order: a row that equals a phenotype gives Sxy == Sxx == Syy and r == 1)
    sxy = np.stack([(dx * dy[p]).sum(axis=1) for p in range(len(dy))], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = sxy / np.sqrt(sxx[:, None] * syy[None, :])
    r = np.clip(r, -1.0, 1.0)
    r[~tested] = np.nan
    return r, tested


def locus_of(nk_cum, row):
    if nk_cum is None:
        return NONE
    l = int(np.searchsorted(np.asarray(nk_cum, np.int64), row, side="right"))
    return l if l < len(nk_cum) else NONE


def scan(G, sample_of, pheno, nk_cum=None, pairs=None, p_threshold=None):
    """best: per phenotype a dict(n_tests, skipped, row, locus, r, se, t, p, p_bonf, q); hits: [(pheno, locus, row, r, t, p)] sorted, or
    None without a threshold.  pairs = (off[ntr + 1], pheno_idx) or None (every phenotype against every row)."""
    r, tested = correlations(G, sample_of, pheno)
    nrows, P = r.shape
    n = len(sample_of)
    paired = np.zeros((nrows, P), bool)
    if pairs is None:
        paired[:] = True
    else:
        off, idx = pairs
        for l in range(len(off) - 1):
            r0, r1 = (int(nk_cum[l - 1]) if l else 0), int(nk_cum[l])
            for p in set(int(v) for v in idx[off[l]:off[l + 1]]):
                paired[r0:r1, p] = True
    best = []
    for p in range(P):
        use = paired[:, p] & tested
        b = dict(n_tests=int(use.sum()), skipped=int((paired[:, p] & ~tested).sum()), row=NONE, locus=NONE, r=0.0, se=0.0, t=0.0, p=0.0, p_bonf=0.0, q=0.0)
        if b["n_tests"]:
            r2 = np.where(use, r[:, p] * r[:, p], -1.0)
            row = int(np.argmax(r2))  # (the first of the largest)
            rr = float(r[row, p])
            se = math.sqrt((1.0 - rr * rr) / (n - 2))
            b.update(row=row, locus=locus_of(nk_cum, row), r=rr, se=se, t=(rr / se if se else math.copysign(math.inf, rr)), p=pvalue(rr, n))
            b["p_bonf"] = b["p"] * b["n_tests"]
        best.append(b)
    have = [p for p in range(P) if best[p]["n_tests"]]
    for p, q in zip(have, bh([best[p]["p_bonf"] for p in have])):
        best[p]["q"] = float(q)
    hits = None
    if p_threshold is not None:
        hits = []
        for p in range(P):
            for row in np.nonzero(paired[:, p] & tested)[0]:
                rr = float(r[row, p])
                pv = pvalue(rr, n)
                if pv <= p_threshold:
                    se = math.sqrt((1.0 - rr * rr) / (n - 2))
                    hits.append((p, locus_of(nk_cum, int(row)), int(row), rr, (rr / se if se else math.copysign(math.inf, rr)), pv))
    return dict(best=best, hits=hits, r=r, tested=tested, paired=paired)


def tolerance(G, sample_of, pheno):
    """The bound on |r_device - r_model| per row (see tests/test_assoc_gpu.py for the derivation): 4 (n + 4) 2^-53 (1 + kappa), kappa the
    larger of the row's max|v| / sd(v) and the largest such ratio over the phenotypes; 0 on rows that are not tested."""
    x, tested, d, sxx = row_stats(G, sample_of)
    n = x.shape[1]
    y = np.asarray(pheno, np.float64).reshape(-1, n)
    kp = max(float(np.abs(v).max() / v.std()) for v in y)
    with np.errstate(invalid="ignore", divide="ignore"):
        kr = np.where(tested, np.abs(np.where(tested[:, None], x, 0.0)).max(axis=1) / np.sqrt(np.where(tested, sxx, 1.0) / n), 0.0)
    return np.where(tested, 4.0 * (n + 4) * U * (1.0 + np.maximum(kr, kp)), 0.0)


def fmt(v):
    return "%.6e" % v


def best_tsv(names, best):
    out = ["pheno\tn_tests\tskipped\tlocus\trow\tr\tse\tt\tp\tp_bonf\tq"]
    for name, b in zip(names, best):
        head = f"{name}\t{b['n_tests']}\t{b['skipped']}\t"
        if not b["n_tests"]:
            out.append(head + "\t".join(["NA"] * 8))
        else:
            out.append(head + "\t".join(["NA" if b["locus"] == NONE else str(b["locus"]), str(b["row"])] + [fmt(b[k]) for k in ("r", "se", "t", "p", "p_bonf", "q")]))
    return "\n".join(out) + "\n"
