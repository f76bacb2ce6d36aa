"""tests/assoc_covar_model.py against an independent implementation: the coefficient of x in the multiple regression y ~ 1 + C + x by
numpy's least squares, its standard error from the residual variance and (X'X)^-1, its p from scipy's Student-t tail.  That the partial
correlation's t = r / sqrt((1 - r^2) / (n - 2 - q)) IS that coefficient's t is the Frisch-Waugh-Lovell theorem; here it is checked in
numbers.  Without covariates the model must be tests/assoc_model.py to the bit, and there must be inputs on which the covariates change
the answer (otherwise the GPU tests could not tell the feature from its absence)."""
import numpy as np
import pytest
from scipy import stats

import assoc_covar_model as cm
import assoc_model


def inputs(n, q, seed, nrows=7, P=3):
    rng = np.random.default_rng(seed)
    sample_of = rng.permutation(n + 4)[:n]
    G = rng.gamma(2.0, 1.5, (nrows, n + 4)).astype(np.float32)
    covar = rng.integers(0, 4, (q, n)).astype(np.float64) + rng.normal(0, 0.5, (q, n))
    pheno = rng.normal(0, 1, (P, n))
    for p in range(P):
        pheno[p] += 0.7 * G[p, sample_of] + covar.T @ rng.normal(0, 0.6, q)
    G[5, sample_of] += (covar.T @ rng.normal(0, 0.8, q)).astype(np.float32)   # a row that leans on the covariates as well
    return G, sample_of, pheno, covar


@pytest.mark.parametrize("q", [1, 5, 12])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_model_is_the_multiple_regression(q, seed):
    """rtol 1e-8 on t.  Both sides are float64; least squares through the normal equations or the QR loses about u cond^2 with cond the
    condition number of the column-scaled design [1, C, x].  The test asserts cond <= 1e3, so the loss is <= 1.1e-16 * 1e6 = 1.1e-10: two
    digits of margin.  p is a function of t and dof alone, d ln p / d ln t is at most dof for the t tail (p ~ t^-dof far out), hence
    rtol dof * 1e-8 on p against 2 * scipy.stats.t.sf(|t|, dof), plus the 2.2e-12 of the continued fraction (tests/test_assoc_host.py)."""
    n = 40
    G, sample_of, pheno, covar = inputs(n, q, seed)
    m = cm.scan(G, sample_of, pheno, covar, p_threshold=1.0)
    dof = n - 2 - q
    assert m["tested"].all() and len(m["hits"]) == G.shape[0] * pheno.shape[0]
    x_all = G[:, sample_of].astype(np.float64)
    for p, _, row, r, t, pv in m["hits"]:
        X = np.column_stack([np.ones(n), covar.T, x_all[row]])
        scaled = X / np.sqrt((X * X).sum(axis=0))
        assert np.linalg.cond(scaled) <= 1e3
        beta, _, rank, _ = np.linalg.lstsq(X, pheno[p], rcond=None)
        assert rank == q + 2
        res = pheno[p] - X @ beta
        s2 = float(res @ res) / dof
        se = np.sqrt(s2 * np.linalg.inv(X.T @ X)[-1, -1])
        t_ols = beta[-1] / se
        assert abs(t - t_ols) <= 1e-8 * abs(t_ols), (p, row, t, t_ols)
        p_ols = 2.0 * stats.t.sf(abs(t_ols), dof)
        assert abs(pv - p_ols) <= (dof * 1e-8 + 2.2e-12) * p_ols, (p, row, pv, p_ols)
        assert np.sign(r) == np.sign(beta[-1])
    for p, b in enumerate(m["best"]):   # the best row is the hit with the largest r^2, and its numbers are that hit's
        mine = [h for h in m["hits"] if h[0] == p]
        top = max(mine, key=lambda h: (h[3] * h[3], -h[2]))
        assert (b["row"], b["r"], b["t"], b["p"]) == (top[2], top[3], top[4], top[5]) and b["n_tests"] == len(mine)
        assert b["se"] == np.sqrt((1 - b["r"] ** 2) / dof) and b["p_bonf"] == b["p"] * b["n_tests"]


def test_without_covariates_the_model_is_the_plain_model():
    for n, seed in ((3, 5), (40, 6), (130, 7)):
        G, sample_of, pheno, _ = inputs(n, 1, seed)
        G[2] = 1.5                                     # a constant row
        G[4, sample_of[0]] = np.inf                    # a row that is not finite
        nk_cum = np.array([2, 2, 6], np.uint32)
        pairs = ([0, 2, 3, 5], [0, 2, 1, 0, 1])
        for kw in (dict(), dict(nk_cum=nk_cum, p_threshold=0.3), dict(nk_cum=nk_cum, pairs=pairs, p_threshold=1.0)):
            a = cm.scan(G, sample_of, pheno, np.zeros((0, n)), **kw)
            b = assoc_model.scan(G, sample_of, pheno, **kw)
            assert a["best"] == b["best"] and a["hits"] == b["hits"]
            assert a["r"].tobytes() == b["r"].tobytes() and (a["tested"] == b["tested"]).all() and (a["paired"] == b["paired"]).all()
            assert (a["share_y"] == 1.0).all() and (a["share_x"][a["tested"]] == 1.0).all()
        tol = cm.tolerance(G, sample_of, pheno, 0, a["share_x"], a["share_y"])
        assert np.allclose(tol, assoc_model.tolerance(G, sample_of, pheno), rtol=1e-15, atol=0)


def test_covariates_change_the_best_row():
    """A phenotype driven by a covariate and, weakly, by row 0; row 1 is that covariate plus noise.  Without covariates row 1 wins (it
    carries the covariate), with them row 0 does: a scan that ignored --assoc-covar would fail the tests that compare best rows."""
    rng = np.random.default_rng(11)
    n = 60
    sample_of = np.arange(n)
    c = rng.integers(0, 3, n).astype(np.float64) + rng.normal(0, 0.3, n)
    G = rng.gamma(2.0, 1.5, (5, n)).astype(np.float32)
    G[1] = (c + rng.normal(0, 0.3, n)).astype(np.float32)
    pheno = (3.0 * c + 0.8 * G[0] + rng.normal(0, 0.5, n)).reshape(1, n)
    plain = assoc_model.scan(G, sample_of, pheno)["best"][0]
    given = cm.scan(G, sample_of, pheno, c.reshape(1, n))
    assert plain["row"] == 1 and given["best"][0]["row"] == 0
    assert given["share_x"][1] < 0.2 < given["share_x"][0] and 1e-3 < given["share_y"][0] < 0.5
    assert abs(given["best"][0]["r"]) > 0.8 and given["best"][0]["p"] < plain["p"] * 1e6


def test_model_refusals():
    n = 12
    G, sample_of, pheno, covar = inputs(n, 3, 4)
    for bad, msg in ((np.vstack([covar, covar[0] + covar[2]]), "covariate 3"), (np.vstack([covar[:1], np.full(n, 2.0)]), "covariate 1"), (np.vstack([covar, covar[1]]), "covariate 3")):
        with pytest.raises(ValueError, match=msg):
            cm.scan(G, sample_of, pheno, bad)
    with pytest.raises(ValueError, match="phenotype 1"):
        cm.scan(G, sample_of, np.vstack([pheno[0], 2 * covar[0] - covar[1] + 3]), covar)
    with pytest.raises(ValueError):
        cm.scan(G, sample_of, pheno, np.random.default_rng(0).normal(0, 1, (10, n)))   # n < q + 3
