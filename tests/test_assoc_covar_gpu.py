"""The association scan with covariates on the GPU (include/dbtk_assoc_covar.h, csrc/dbtk_assoc.hip: k_assoc_scan<., true> and
k_assoc_covar_pheno) at library level, against tests/assoc_covar_model.py fed the same float32 matrix AND the handle's own basis Q
(dbtk_assoc_covar_basis of the covariates in ascending sample order, which is what dbtk_assoc_covar_set computes): model and kernel then
differ in the order of their sums only.

The tolerance is derived, not measured; it extends the derivation of tests/test_assoc_gpu.py.  u = 2^-53.  Write everything in units of
sqrt(Sxx) and sqrt(Syy): x^ = dx / sqrt(Sxx), y^ = dy / sqrt(Syy).  From that derivation, per side, Sxy / sqrt(Sxx Syy) carries an absolute
error of at most (n + 2) u (1 + kappa), kappa = max|v| / sd(v) over the row and the phenotypes (the rounding of each dx = fl(x - m)).
  a_j / sqrt(Sxx) is a sum of n products dx_i Q_ij with sum Q_ij^2 = 1: by Cauchy-Schwarz its error is at most (n + 2) u (1 + kappa), and
  the same holds for b_j / sqrt(Syy).
  sum_j a^_j b^_j: sum_j (|da_j| |b^_j| + |a^_j| |db_j|) <= (n + 2) u (1 + kappa) (sum |b^_j| + sum |a^_j|) <= 2 sqrt(q) (n + 2) u (1 + kappa),
  because sum a^_j^2 <= 1 gives sum |a^_j| <= sqrt(q); the q multiply-adds of the subtraction add at most q u.
So E = [(n + 2)(1 + 2 sqrt(q)) + q] u (1 + kappa) bounds the absolute error of Sxy' / sqrt(Sxx Syy), and in the same way that of the two
shares rho_x = Sxx' / Sxx and rho_y = Syy' / Syy (there da_j meets a^_j itself).  r = (Sxy' / sqrt(Sxx Syy)) / sqrt(rho_x rho_y) with
|Sxy' / sqrt(Sxx Syy)| <= sqrt(rho_x rho_y): the cancellation amplifies by 1 / rho,
  |dr| <= E / sqrt(rho_x rho_y) + |r| (E / (2 rho_x) + E / (2 rho_y)) <= 2 E / min(rho_x, rho_y),
plus the roundings of the product, the square root and the division (3 u, absorbed by n + 4 for n + 2).  Between the two sides, per row,
    TOL_R = 4 [(n + 4)(1 + 2 sqrt(q)) + q] 2^-53 (1 + kappa) / min(rho_x, rho_y)          (assoc_covar_model.tolerance)
with rho_y the smallest share among the phenotypes.  This is the issue's starting form; the check above found nothing to correct in it.
With q = 0 and rho = 1 it is the bound of tests/test_assoc_gpu.py.  se, t and p follow from r as there with n - q in place of n
(test_assoc_gpu.compare is called with n - q: se = sqrt((1 - r^2) / (n - q - 2)), p = pvalue(r, n - q)).

n_tests, skipped, rows, loci and the hit set compare EXACTLY; for that every test first asserts (test_assoc_gpu.assert_margins and
share_margins below) that its own inputs keep, by a factor of 1000: the best r^2 from the runner-up, every tested r^2 from the kernel's hit
threshold, and every row's residual share from DBTK_ASSOC_COVAR_COLLINEAR (below COLLINEAR / 1000 or above 1000 COLLINEAR; every
phenotype's share above 1000 COLLINEAR).  The seeds were chosen so that the model alone satisfies this (checked without a GPU)."""
import math

import numpy as np
import pytest

import assoc_covar_model as cm
import assoc_model
import bind
from test_assoc_gpu import NPHENO, P_THRESHOLD, assert_margins, compare, hand_made, put
from test_pred_device import _Hip

abi, pkg = bind.abi, bind.pkg

# (n, ns, q, seed): dof 1, a second covariate chunk and lanes without a sample; one covariate; exactly one chunk; three chunks at the last
# register-resident n; the cap at the first n that is not resident; a third segment
CASES = [(12, 20, 9, 3), (65, 70, 1, 1), (65, 70, 8, 1), (512, 520, 17, 1), (513, 520, 128, 1), (1100, 1111, 9, 1)]
ROW_SPAN, ROW_NEAR = 11, 12   # in the locus of 40 rows, beside the special rows of test_assoc_gpu.hand_made (2, 3, 4, 7, 9, 20)


@pytest.fixture(scope="module")
def dbtk():
    return pkg.Dbtk()


@pytest.fixture(scope="module")
def hip():
    return _Hip()


def covar_case(n, ns, q, seed):
    """test_assoc_gpu.hand_made plus covariates (small integers, all but the first two with noise), phenotypes that lean on the covariates
    as well as on their row (not the phenotype that a row equals bit for bit), a row that is an exact float32 combination of the integer
    covariates and that row plus noise."""
    c = hand_made(n, ns, seed=1000 * seed + n)
    rng = np.random.default_rng(77 + seed)
    covar = rng.integers(0, 4, (q, n)).astype(np.float64)
    covar[2:] += rng.normal(0, 0.25, (max(q - 2, 0), n))
    pheno, so, r40 = c["pheno"], c["sample_of"], c["r40"]
    for p in range(NPHENO):
        if p != c["p_one"]:
            pheno[p] += covar.T @ rng.normal(0, 0.5, q)
    combo = 1.0 + 2.0 * covar[0] + (3.0 * covar[1] if q > 1 else 0.0)
    c["G"][r40 + ROW_SPAN, so] = combo.astype(np.float32)
    assert (c["G"][r40 + ROW_SPAN, so].astype(np.float64) == combo).all()
    c["G"][r40 + ROW_NEAR, so] = (combo + rng.normal(0, 1.4, n)).astype(np.float32)
    c.update(covar=covar, q=q, names=[f"cov{j}" for j in range(q)])
    return c


def basis_of(dbtk, c):
    order = np.argsort(c["sample_of"], kind="stable")
    return pkg.assoc_covar_basis(dbtk, c["covar"][:, order])


def share_margins(m):
    sx = m["share_x"][np.isfinite(m["share_x"])]
    assert ((sx < cm.COLLINEAR / 1000) | (sx > 1000 * cm.COLLINEAR)).all(), sx[(sx >= cm.COLLINEAR / 1000) & (sx <= 1000 * cm.COLLINEAR)]
    assert (m["share_y"] > 1000 * cm.COLLINEAR).all(), m["share_y"].min()


def model_of(dbtk, c, Q, pairs=None):
    """the model's scan, its tolerance and the kernel's threshold, with every margin asserted"""
    n, q = len(c["sample_of"]), c["q"]
    m = cm.scan(c["G"], c["sample_of"], c["pheno"], c["covar"], Q=Q, nk_cum=c["nk_cum"], pairs=pairs, p_threshold=P_THRESHOLD)
    tol = cm.tolerance(c["G"], c["sample_of"], c["pheno"], q, m["share_x"], m["share_y"])
    assert tol[m["tested"]].max() < 1e-7
    share_margins(m)
    assert_margins(m, c["G"], c["sample_of"], tol, pkg.assoc_r2_threshold(dbtk, P_THRESHOLD, n - q))
    r40 = c["r40"]
    assert not m["tested"][r40 + ROW_SPAN] and m["tested"][r40 + ROW_NEAR] and 1e-3 < m["share_x"][r40 + ROW_NEAR] < 0.5
    assert m["tested"][r40 + 4] and not m["tested"][r40 + 2] and not m["tested"][r40 + 3]
    return m, tol


def test_the_inputs_keep_their_margins_without_a_gpu(dbtk):
    """what the GPU tests assert of their inputs before they compare, on every case: the seeds are good wherever the suite runs"""
    for n, ns, q, seed in CASES:
        c = covar_case(n, ns, q, seed)
        Q = basis_of(dbtk, c)
        m, _ = model_of(dbtk, c, Q)
        model_of(dbtk, c, Q, pairs=c["pairs"])
        own = cm.scan(c["G"], c["sample_of"], c["pheno"], c["covar"], nk_cum=c["nk_cum"])   # numpy's QR spans the same space
        assert [b["row"] for b in own["best"]] == [b["row"] for b in m["best"]] and (own["tested"] == m["tested"]).all()
        assert np.nanmax(np.abs(own["r"] - m["r"])) < 1e-7


@pytest.mark.gpu
@pytest.mark.parametrize("n,ns,q,seed", CASES)
def test_scan_with_covariates_on_hand_made_matrices(dbtk, hip, n, ns, q, seed):
    c = covar_case(n, ns, q, seed)
    G, sample_of, pheno, nk_cum, r40 = c["G"], c["sample_of"], c["pheno"], c["nk_cum"], c["r40"]
    Q = basis_of(dbtk, c)
    A = pkg.Assoc(dbtk, ns, sample_of, pheno)
    d = put(hip, G)
    try:
        assert A.covariates() == (0, n - 2)
        A.set_covariates(c["covar"], names=c["names"])
        assert A.covariates() == (q, n - 2 - q)
        # every phenotype against every row
        m, tol = model_of(dbtk, c, Q)
        A.scan_device(d, G.shape[0], nk_cum=nk_cum, p_threshold=P_THRESHOLD)
        best, hits = A.best(), A.hits()
        compare(best, hits, m, n - q, tol)
        assert all(b["n_tests"] == G.shape[0] - 3 and b["skipped"] == 3 for b in best)   # constant, not finite, explained by the covariates
        one = best[c["p_one"]]
        assert one["row"] == r40 + 7 and one["r"] == 1.0 and one["p"] == 0.0 and one["t"] == math.inf and one["se"] == 0.0
        assert best[c["p_tie"]]["row"] == m["best"][c["p_tie"]]["row"]
        if m["best"][c["p_tie"]]["row"] in (r40 + 9, r40 + 20):
            assert best[c["p_tie"]]["row"] == r40 + 9                                     # duplicate rows: the lower one
        dup = {h[0]: h[3] for h in hits if h[2] == r40 + 9}
        assert all(h[3] == dup[h[0]] for h in hits if h[2] == r40 + 20 and h[0] in dup)   # and they tie bit for bit
        # the pair list
        A.set_pairs(*c["pairs"])
        mp, _ = model_of(dbtk, c, Q, pairs=c["pairs"])
        A.scan_device(d, G.shape[0], nk_cum=nk_cum, p_threshold=P_THRESHOLD)
        bp, hp = A.best(), A.hits()
        compare(bp, hp, mp, n - q, tol)
        assert bp[c["p_one"]]["r"] == 1.0 and bp[c["p_one"]]["p"] == 0.0
        assert all(h[2] < int(nk_cum[-1]) for h in hp)
        # twice the same bytes
        A.scan_device(d, G.shape[0], nk_cum=nk_cum, p_threshold=P_THRESHOLD)
        assert A.best() == bp and A.hits() == hp
    finally:
        hip.free(d)
        A.close()


@pytest.mark.gpu
def test_removing_the_covariates_gives_back_the_plain_scan(dbtk, hip, tmp_path):
    n, ns, q, seed = CASES[1]
    c = covar_case(n, ns, q, seed)
    G, nk_cum = c["G"], c["nk_cum"]
    plain = pkg.Assoc(dbtk, ns, c["sample_of"], c["pheno"])
    A = pkg.Assoc(dbtk, ns, c["sample_of"], c["pheno"])
    d = put(hip, G)
    try:
        plain.scan_device(d, G.shape[0], nk_cum=nk_cum, p_threshold=P_THRESHOLD)
        plain.write(str(tmp_path / "plain"))
        A.set_covariates(c["covar"])
        A.scan_device(d, G.shape[0], nk_cum=nk_cum, p_threshold=P_THRESHOLD)
        with_cov = A.best()
        assert [b["row"] for b in with_cov] != [b["row"] for b in plain.best()] or [b["r"] for b in with_cov] != [b["r"] for b in plain.best()]
        A.set_covariates(None)
        assert A.covariates() == (0, n - 2)
        with pytest.raises(pkg.DbtkError):
            A.best()                                     # setting covariates invalidates the scan made last
        A.scan_device(d, G.shape[0], nk_cum=nk_cum, p_threshold=P_THRESHOLD)
        assert A.best() == plain.best() and A.hits() == plain.hits()
        A.write(str(tmp_path / "back"))
        for ext in (".assoc.best.tsv", ".assoc.hits.tsv"):
            assert open(str(tmp_path / "back") + ext, "rb").read() == open(str(tmp_path / "plain") + ext, "rb").read()
    finally:
        hip.free(d)
        A.close()
        plain.close()


@pytest.mark.gpu
def test_set_covariates_refusals(dbtk):
    rng = np.random.default_rng(9)
    n, ns = 12, 14
    sample_of = rng.permutation(ns)[:n]
    covar = rng.integers(0, 4, (3, n)).astype(np.float64) + rng.normal(0, 0.3, (3, n))
    pheno = rng.normal(0, 1, (3, n))
    pheno[1] = 2.0 * covar[0] - covar[2] + 3.0           # inside the span of the covariates and the intercept
    A = pkg.Assoc(dbtk, ns, sample_of, pheno, names=["weight", "height", "age"])
    cases = [
        (covar, None, "phenotype height is explained by the covariates"),
        (rng.normal(0, 1, (n - 2, n)), None, "q + 3"),   # n = q + 2
        (np.vstack([covar, covar[1]]), ["a", "b", "c", "again"], "covariate again is constant or collinear"),
        (np.vstack([covar[:1], np.full(n, 0.1)]), None, "covariate c1 is constant"),
        (np.where(np.arange(3 * n).reshape(3, n) == 17, np.nan, covar), None, "covariate c1 has a value that is not finite"),
    ]
    try:
        for cv, names, msg in cases:
            with pytest.raises(pkg.DbtkError) as e:
                A.set_covariates(cv, names=names)
            assert e.value.status == abi.ERR_ARG and msg in str(e.value), str(e.value)
            assert A.covariates() == (0, n - 2)
        A.set_covariates(covar[:2])                      # without the third covariate the phenotype keeps a share
        assert A.covariates() == (2, n - 4)
        with pytest.raises(pkg.DbtkError):
            A.set_covariates(covar)
        assert A.covariates() == (2, n - 4)              # a refused call leaves what was set
    finally:
        A.close()
    big_n = abi.ASSOC_COVAR_MAX + 12
    B = pkg.Assoc(dbtk, big_n, np.arange(big_n), rng.normal(0, 1, (1, big_n)))
    try:
        with pytest.raises(pkg.DbtkError) as e:
            B.set_covariates(rng.normal(0, 1, (abi.ASSOC_COVAR_MAX + 1, big_n)))
        assert e.value.status == abi.ERR_ARG and "DBTK_ASSOC_COVAR_MAX" in str(e.value)
    finally:
        B.close()
