"""The contract of the permutation p-values of the association scan (include/dbtk_assoc_perm.h) in Python and numpy float64: the seeded
generator with Python integers, the maxima T[P][B + 1] on top of assoc_model.row_stats / assoc_covar_model.partial, and n_ge, p_perm and
q_perm.  numpy and the standard library only."""
import numpy as np

import assoc_covar_model as cm
import assoc_model

M64 = (1 << 64) - 1
PERM_MAX = 1000000


class SplitMix64:
    def __init__(self, seed):
        self.s = int(seed) & M64

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)


def generate(n, B, seed):
    """perm[B][n] uint32: permutations 1 .. B in that order from one stream; each from the identity, i = n - 1 down to 1,
    j = (next() * (i + 1)) >> 64, swap."""
    g = SplitMix64(seed)
    out = np.zeros((B, n), np.uint32)
    for b in range(B):
        p = list(range(n))
        for i in range(n - 1, 0, -1):
            j = (g.next() * (i + 1)) >> 64
            p[i], p[j] = p[j], p[i]
        out[b] = p
    return out


def is_permutation(row, n):
    row = np.asarray(row, np.int64)
    return len(row) == n and (np.sort(row) == np.arange(n)).all()


def paired_matrix(nrows, P, nk_cum, pairs):
    paired = np.zeros((nrows, P), bool)
    if pairs is None:
        paired[:] = True
        return paired
    off, idx = pairs
    for l in range(len(off) - 1):
        r0, r1 = (int(nk_cum[l - 1]) if l else 0), int(nk_cum[l])
        for p in set(int(v) for v in idx[off[l]:off[l + 1]]):
            paired[r0:r1, p] = True
    return paired


def maxima(G, sample_of, pheno, perms, nk_cum=None, pairs=None, covar=None, Q=None):
    """T[P][B + 1] (slot 0 the identity; 0 for a phenotype without tests), n_tests[P], y[P][n]: what is permuted (the centred
    phenotypes, with covariates their residuals), over the samples in ascending order.  perms[B][n] over those positions.  A slot whose
    permuted vector is byte-equal to the vector itself gets T_0's own bits (the device sends both through one code path)."""
    order = np.argsort(np.asarray(sample_of, np.int64), kind="stable")
    n = len(order)
    y = np.asarray(pheno, np.float64).reshape(-1, n)[:, order]
    P = y.shape[0]
    perms = np.asarray(perms, np.int64).reshape(-1, n)
    B = perms.shape[0]
    x, tested, dx, sxx = assoc_model.row_stats(G, sample_of)
    dy = y - y.sum(axis=1, keepdims=True) / n
    syy = (dy * dy).sum(axis=1)
    if covar is not None and np.asarray(covar).size:
        c = np.asarray(covar, np.float64).reshape(-1, n)[:, order]
        Qm = cm.basis(c) if Q is None else np.asarray(Q, np.float64).reshape(-1, n)
        _, tested, _, _ = cm.partial(G, sample_of, pheno, covar, Q=Qm)
        a = dx @ Qm.T
        b = dy @ Qm.T
        dx = dx - a @ Qm
        dy = dy - b @ Qm                     # permuted as it is, not projected again (FastQTL)
        sxx = sxx - (a * a).sum(axis=1)
        syy = syy - (b * b).sum(axis=1)
    paired = paired_matrix(x.shape[0], P, nk_cum, pairs)
    use = paired & tested[:, None]
    T = np.zeros((P, B + 1))
    allp = np.vstack([np.arange(n)[None, :], perms])
    dxu = np.where(tested[:, None], dx, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        for p in range(P):
            if not use[:, p].any():
                continue
            cols = dy[p][allp]                                   # [B + 1][n]
            r = (dxu @ cols.T) / np.sqrt(sxx * syy[p])[:, None]  # [nrows][B + 1]
            r2 = np.clip(r, -1.0, 1.0) ** 2
            T[p] = np.where(use[:, p][:, None], r2, 0.0).max(axis=0)
            for b in range(1, B + 1):
                if cols[b].tobytes() == cols[0].tobytes():
                    T[p, b] = T[p, 0]
    return T, use.sum(axis=0), dy


def fold(T, n_tests):
    """n_ge[P], p_perm[P], q_perm[P]"""
    T = np.asarray(T)
    P, B = T.shape[0], T.shape[1] - 1
    n_ge = np.zeros(P, np.int64)
    p_perm = np.zeros(P)
    q_perm = np.zeros(P)
    have = [p for p in range(P) if n_tests[p]]
    for p in have:
        n_ge[p] = int((T[p, 1:] >= T[p, 0]).sum())
        p_perm[p] = (n_ge[p] + 1) / (B + 1)
    if have:
        q_perm[have] = assoc_model.bh(p_perm[have])
    return n_ge, p_perm, q_perm


def assert_margins(T, y, perms, bound, ties=()):
    """Every |T_b - T_0| is exactly 0 with y o pi_b byte-equal to y (or (p, b) listed in `ties`), or at least 1000 times the bound[p]."""
    perms = np.asarray(perms, np.int64).reshape(-1, y.shape[1])
    for p in range(T.shape[0]):
        for b in range(1, T.shape[1]):
            d = abs(T[p, b] - T[p, 0])
            same = y[p][perms[b - 1]].tobytes() == y[p].tobytes() or (p, b) in ties
            if same:
                assert d == 0.0, (p, b, d)
            else:
                assert d >= 1000.0 * bound[p], (p, b, d, bound[p])


def perm_tsv(names, n_tests, rows, T, n_ge, p_perm, q_perm):
    B = T.shape[1] - 1
    out = ["pheno\tn_tests\trow\tr2\tn_perm\tn_ge\tp_perm\tq_perm"]
    for p, name in enumerate(names):
        if not n_tests[p]:
            out.append(f"{name}\t0\tNA\tNA\t{B}\tNA\tNA\tNA")
        else:
            out.append(f"{name}\t{int(n_tests[p])}\t{int(rows[p])}\t{assoc_model.fmt(T[p, 0])}\t{B}\t{int(n_ge[p])}\t{assoc_model.fmt(p_perm[p])}\t{assoc_model.fmt(q_perm[p])}")
    return "\n".join(out) + "\n"
