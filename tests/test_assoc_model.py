"""tests/assoc_model.py against an independent implementation: scipy.stats.linregress on the z-scored pair gives the slope, rvalue, stderr
and pvalue of ordinary least squares with a constant, which is what script/eqtl.noPerm.py asks of statsmodels
(sm.OLS(y, add_constant(x))); scipy.stats.false_discovery_control is the Benjamini-Hochberg of statsmodels' fdrcorrection.
statsmodels is not installed where these tests were written: the script itself was NOT run, the closed forms are pinned to scipy."""
import math

import numpy as np
import pytest

import assoc_model

stats = pytest.importorskip("scipy.stats")


def zscore(v):
    return (v - v.mean()) / v.std()  # np.std, ddof 0, as the script


def small_case(seed, nrows=12, ns=40, n=29, P=3):
    rng = np.random.default_rng(seed)
    G = rng.gamma(2.0, 1.5, (nrows, ns)).astype(np.float32)
    sample_of = rng.permutation(ns)[:n]
    pheno = rng.normal(0, 1, (P, n)) + 0.4 * G[rng.integers(0, nrows, P)][:, sample_of]
    return G, sample_of, pheno


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_every_pair_equals_linregress_on_the_z_scored_pair(seed):
    G, sample_of, pheno = small_case(seed)
    n = len(sample_of)
    m = assoc_model.scan(G, sample_of, pheno, p_threshold=1.0)
    assert len(m["hits"]) == G.shape[0] * pheno.shape[0]
    for p, _, row, r, t, pv in m["hits"]:
        x = zscore(G[row, sample_of].astype(np.float64))
        y = zscore(pheno[p])
        lr = stats.linregress(x, y)
        se = math.sqrt((1 - r * r) / (n - 2))
        assert abs(lr.slope - r) < 1e-13 and abs(lr.rvalue - r) < 1e-13
        assert abs(lr.stderr - se) < 1e-13 * max(1, se) and abs(lr.pvalue - pv) <= 1e-10 * pv
        assert abs(t - lr.slope / lr.stderr) <= 1e-11 * abs(t)
    for p, b in enumerate(m["best"]):
        r2 = [h[3] ** 2 for h in m["hits"] if h[0] == p]
        assert b["n_tests"] == G.shape[0] and b["skipped"] == 0 and b["r"] ** 2 == max(r2) and b["p_bonf"] == b["p"] * G.shape[0]
    q = stats.false_discovery_control([b["p_bonf"] for b in m["best"]], method="bh")
    assert np.allclose([b["q"] for b in m["best"]], np.minimum(q, 1.0), rtol=1e-14, atol=0)


def test_bh_equals_false_discovery_control():
    rng = np.random.default_rng(5)
    for m in (1, 2, 7, 100):
        p = rng.uniform(0, 1, m) ** 3
        p[rng.integers(0, m)] = 0.0
        if m > 2:
            p[1] = p[2]  # a tie
        assert np.allclose(assoc_model.bh(p), stats.false_discovery_control(p, method="bh"), rtol=1e-14, atol=0)
    # p_bonf above 1 enters unclipped and leaves clipped
    assert list(assoc_model.bh([3.0, 0.2])) == [1.0, 0.4]
    assert len(assoc_model.bh([])) == 0


def test_pvalue_equals_the_t_tail():
    for n in (3, 4, 10, 100, 879):
        for r in (1e-6, 0.01, 0.3, 0.7, 0.99, 1 - 1e-9):
            t = r * math.sqrt((n - 2) / ((1 - r) * (1 + r)))
            want = 2 * stats.t.sf(t, n - 2)
            if want > 1e-300:
                assert abs(assoc_model.pvalue(r, n) - want) <= 1e-11 * want, (n, r)
                assert assoc_model.pvalue(-r, n) == assoc_model.pvalue(r, n)
    assert assoc_model.pvalue(1.0, 10) == 0.0 and assoc_model.pvalue(-1.0, 3) == 0.0 and assoc_model.pvalue(0.0, 10) == 1.0


def test_untested_rows_ties_pairs_and_exact_one():
    rng = np.random.default_rng(9)
    ns, n = 20, 14
    sample_of = np.arange(3, 3 + n)
    G = rng.normal(5, 2, (9, ns)).astype(np.float32)
    G[1] = 2.5                      # constant
    G[2, 7] = np.inf                # one inf inside the mask
    G[3, 0] = np.nan                # a nan outside the mask: tested
    G[4] = 1.0
    G[4, 9] = 2.0                   # a single sample differs
    G[6] = G[5]                     # a tie: the lower row wins
    pheno = np.stack([G[5, sample_of].astype(np.float64) * 3 + 1, rng.normal(0, 1, n), G[8, sample_of].astype(np.float64)])
    m = assoc_model.scan(G, sample_of, pheno, p_threshold=1.0)
    assert list(m["tested"]) == [True, False, False, True, True, True, True, True, True]
    b = m["best"]
    assert b[0]["n_tests"] == 7 and b[0]["skipped"] == 2 and b[0]["row"] == 5 and abs(b[0]["r"] - 1) < 1e-12
    assert b[2]["row"] == 8 and b[2]["r"] == 1.0 and b[2]["p"] == 0.0 and b[2]["se"] == 0.0 and b[2]["t"] == math.inf and b[2]["q"] == 0.0
    # pairs: locus 0 = rows 0..2 with phenotype 1, locus 1 = no row, locus 2 = rows 3..6 with phenotypes 0 and 1 (0 listed twice); rows 7, 8 belong to no locus
    nk_cum = [3, 3, 7]
    mp = assoc_model.scan(G, sample_of, pheno, nk_cum=nk_cum, pairs=([0, 1, 1, 4], [1, 0, 1, 0]), p_threshold=1.0)
    bp = mp["best"]
    assert (bp[0]["n_tests"], bp[0]["skipped"], bp[0]["row"], bp[0]["locus"]) == (4, 0, 5, 2)
    assert (bp[1]["n_tests"], bp[1]["skipped"]) == (5, 2) and bp[2]["n_tests"] == 0 and bp[2]["row"] == assoc_model.NONE and bp[2]["q"] == 0.0
    assert sorted(set((h[0], h[2]) for h in mp["hits"])) == [(0, 3), (0, 4), (0, 5), (0, 6), (1, 0), (1, 3), (1, 4), (1, 5), (1, 6)]
    text = assoc_model.best_tsv(["a", "b", "c"], bp)
    assert text.split("\n")[3] == "c\t0\t0\t" + "\t".join(["NA"] * 8) and text.split("\n")[1].startswith("a\t4\t0\t2\t5\t")
