"""The permutation p-values of the association scan on the GPU (include/dbtk_assoc_perm.h, csrc/dbtk_assoc_perm_dev.h: k_assoc_perm) at
library level, against tests/assoc_perm_model.py fed the same float32 matrix and the same permutations.

The tolerance is the derived one of tests/test_assoc_gpu.py (with covariates: of tests/test_assoc_covar_gpu.py), unchanged: a permutation
changes the ORDER of one factor of Sxy, not the conditioning of anything, so |r_device - r_model| <= tol per row, and for the statistic
T = max r^2 of a phenotype |T_device - T_model| <= 2 tol (1 + tol) with tol the largest bound over the rows paired with it
(d(r^2) <= 2 |r| dr + dr^2, |r| <= 1; a maximum moves by no more than its arguments).

n_ge, the rows and n_tests compare EXACTLY.  For that every case first asserts (assoc_perm_model.assert_margins) that each |T_b - T_0| of
the model is either exactly 0 with y o pi_b byte-equal to y, or at least 1000 times the bound; test_assoc_perm_host.py makes the same
assertion on every case of this file that needs no device to be built, wherever the suite runs."""
import numpy as np
import pytest

import assoc_covar_model as cm
import assoc_model
import assoc_perm_model as pm
import bind
from test_assoc_covar_gpu import covar_case
from test_assoc_gpu import NPHENO, P_THRESHOLD, cohort_pheno, hand_made, put
from test_pred import make_cohort
from test_pred_device import _Hip

abi, pkg = bind.abi, bind.pkg

NOISE = 4                      # phenotypes of pure noise behind the 12 of hand_made: their n_ge is not 0
CHUNK = 8                      # PM_CHUNK (test_assoc_perm_host.py reads it from the source and compares)
# (n, ns, B, seed): every n of the issue with one B, every B with one n; B + 1 columns per phenotype: 8 fill a chunk, 9 start a second
MODEL_CASES = [(3, 9, 65, 1), (64, 70, 1, 1), (65, 70, CHUNK - 1, 1), (512, 520, CHUNK, 1), (513, 520, CHUNK + 1, 1), (1100, 1111, 65, 1)]
# (n, ns, q, B, seed)
COVAR_CASES = [(12, 20, 9, 9, 3), (65, 70, 8, 7, 1), (513, 520, 128, 8, 1), (1100, 1111, 9, 3, 1)]
ALL_ROWS_CASE = (130, 140, 9, 2)   # without a pair list: P = 12 against all 359 rows, a second work item
ORACLE_CASE = (65, 70, 9, 4)       # the permuted vectors as explicit phenotypes of the plain scan


@pytest.fixture(scope="module")
def dbtk():
    return pkg.Dbtk()


@pytest.fixture(scope="module")
def hip():
    return _Hip()


def with_noise(c, seed, n):
    """hand_made's (or covar_case's) case plus NOISE phenotypes of pure noise, paired with the loci of 5, 40 and 300 rows"""
    rng = np.random.default_rng(9000 + seed)
    c["pheno"] = np.vstack([c["pheno"], rng.normal(0, 1, (NOISE, n))])
    off, idx = c["pairs"]
    noff, nidx = [0], []
    for l in range(len(off) - 1):
        nidx += list(idx[off[l]:off[l + 1]])
        if l >= 4:
            nidx += list(range(NPHENO, NPHENO + NOISE))
        noff.append(len(nidx))
    c["pairs"] = (noff, nidx)
    return c


def plain_case(n, ns, seed):
    return with_noise(hand_made(n, ns, seed=300 + 7 * seed + n), seed, n)


def covariate_case(n, ns, q, seed):
    return with_noise(covar_case(n, ns, q, seed), seed, n)


def bound_of(tol, use):
    """per phenotype 2 tol (1 + tol), tol the largest bound over its tested rows"""
    t = np.array([tol[use[:, p]].max() if use[:, p].any() else 0.0 for p in range(use.shape[1])])
    return 2.0 * t * (1.0 + t)


def model_of(c, perms, pairs, Q=None, ties=()):
    """T of the model, n_tests, its bound per phenotype, with the margins asserted"""
    covar = c.get("covar")
    T, n_tests, y = pm.maxima(c["G"], c["sample_of"], c["pheno"], perms, nk_cum=c["nk_cum"], pairs=pairs, covar=covar, Q=Q)
    if covar is None:
        m = assoc_model.scan(c["G"], c["sample_of"], c["pheno"], nk_cum=c["nk_cum"], pairs=pairs)
        tol = assoc_model.tolerance(c["G"], c["sample_of"], c["pheno"])
    else:
        m = cm.scan(c["G"], c["sample_of"], c["pheno"], covar, Q=Q, nk_cum=c["nk_cum"], pairs=pairs)
        tol = cm.tolerance(c["G"], c["sample_of"], c["pheno"], c["q"], m["share_x"], m["share_y"])
    use = m["paired"] & m["tested"][:, None]
    assert (use.sum(axis=0) == n_tests).all()
    bound = bound_of(tol, use)
    assert bound.max() < 1e-6
    pm.assert_margins(T, y, perms, bound, ties)
    return T, n_tests, bound, m


def check(A, T, n_tests, bound, m, B):
    """the handle's results against the model's"""
    res, best = A.perm_results(), A.best()
    n_ge, p_perm, q_perm = pm.fold(T, n_tests)
    got = np.array([A.perm_stats(p) for p in range(A.P)])
    for p in range(A.P):
        print(f"pheno {p}: n_tests {n_tests[p]} max |T - model| {np.abs(got[p] - T[p]).max():.3e} bound {bound[p]:.3e} n_ge {res[p]['n_ge']}")
    for p in range(A.P):
        r = res[p]
        assert best[p]["n_tests"] == n_tests[p] and r["n_perm"] == B and r["row"] == best[p]["row"] == m["best"][p]["row"], (p, r, best[p])
        assert (np.abs(got[p] - T[p]) <= bound[p]).all(), (p, np.abs(got[p] - T[p]).max(), bound[p])
        if not n_tests[p]:
            assert (got[p] == 0).all() and r["n_ge"] == 0 and r["p_perm"] == 0 and r["q_perm"] == 0 and r["r2"] == 0 and r["row"] == abi.ASSOC_NONE
            continue
        assert r["r2"] == got[p][0] and abs(r["r2"] - best[p]["r"] ** 2) <= bound[p], (p, r["r2"], best[p]["r"] ** 2)
        assert r["n_ge"] == n_ge[p], (p, r["n_ge"], n_ge[p])
        assert r["p_perm"] == (r["n_ge"] + 1) / (B + 1)
    have = [p for p in range(A.P) if n_tests[p]]
    assert np.allclose([res[p]["q_perm"] for p in have], q_perm[have], rtol=1e-14, atol=0)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("n,ns,B,seed", MODEL_CASES)
def test_perm_scan_against_the_model(dbtk, hip, n, ns, B, seed):
    c = plain_case(n, ns, seed)
    perms = pm.generate(n, B, seed)
    T, n_tests, bound, m = model_of(c, perms, c["pairs"])
    A = pkg.Assoc(dbtk, ns, c["sample_of"], c["pheno"])
    fresh = pkg.Assoc(dbtk, ns, c["sample_of"], c["pheno"])
    d = put(hip, c["G"])
    try:
        A.set_pairs(*c["pairs"])
        A.set_permutations(B, seed=seed)
        assert (A.permutations() == perms).all()
        A.perm_scan_device(d, c["G"].shape[0], nk_cum=c["nk_cum"], p_threshold=P_THRESHOLD)
        got = check(A, T, n_tests, bound, m, B)
        assert any(r["n_ge"] > 0 for r in A.perm_results()[NPHENO:]) or B == 1
        best, hits = A.best(), A.hits()
        if n == 3:   # every seeded permutation that happens to be the identity ties bit for bit
            ident = [b for b in range(B) if (perms[b] == np.arange(n)).all()]
            assert ident and all((got[:, b + 1] == got[:, 0]).all() for b in ident)
        # twice on the same handle and once on a fresh one: the same bytes
        A.perm_scan_device(d, c["G"].shape[0], nk_cum=c["nk_cum"], p_threshold=P_THRESHOLD)
        assert np.array([A.perm_stats(p) for p in range(A.P)]).tobytes() == got.tobytes()
        fresh.set_pairs(*c["pairs"])
        fresh.set_permutations(B, perms=perms)
        fresh.perm_scan_device(d, c["G"].shape[0], nk_cum=c["nk_cum"], p_threshold=P_THRESHOLD)
        assert np.array([fresh.perm_stats(p) for p in range(A.P)]).tobytes() == got.tobytes() and fresh.perm_results() == A.perm_results()
        # the ordinary results are those of the plain scan with the same arguments
        fresh.scan_device(d, c["G"].shape[0], nk_cum=c["nk_cum"], p_threshold=P_THRESHOLD)
        assert fresh.best() == best and fresh.hits() == hits
        with pytest.raises(pkg.DbtkError):
            fresh.perm_results()          # a plain scan leaves no permutation result behind
        assert A.perm_times()[0] > 0
    finally:
        hip.free(d)
        A.close()
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,ns,q,B,seed", COVAR_CASES)
def test_perm_scan_with_covariates(dbtk, hip, n, ns, q, B, seed):
    c = covariate_case(n, ns, q, seed)
    order = np.argsort(c["sample_of"], kind="stable")
    Q = pkg.assoc_covar_basis(dbtk, c["covar"][:, order])
    perms = pm.generate(n, B, seed)
    T, n_tests, bound, m = model_of(c, perms, c["pairs"], Q=Q)
    A = pkg.Assoc(dbtk, ns, c["sample_of"], c["pheno"])
    d = put(hip, c["G"])
    try:
        A.set_pairs(*c["pairs"])
        A.set_covariates(c["covar"])
        A.set_permutations(B, seed=seed)
        A.perm_scan_device(d, c["G"].shape[0], nk_cum=c["nk_cum"], p_threshold=P_THRESHOLD)
        check(A, T, n_tests, bound, m, B)
    finally:
        hip.free(d)
        A.close()


@pytest.mark.gpu
def test_perm_scan_without_a_pair_list(dbtk, hip):
    n, ns, B, seed = ALL_ROWS_CASE
    c = hand_made(n, ns, seed=300 + 7 * seed + n)
    perms = pm.generate(n, B, seed)
    T, n_tests, bound, m = model_of(c, perms, None)
    A = pkg.Assoc(dbtk, ns, c["sample_of"], c["pheno"])
    d = put(hip, c["G"])
    try:
        A.set_permutations(B, seed=seed)
        A.perm_scan_device(d, c["G"].shape[0], nk_cum=c["nk_cum"])
        check(A, T, n_tests, bound, m, B)
        assert all(t == c["G"].shape[0] - 2 for t in n_tests)
    finally:
        hip.free(d)
        A.close()


def tie_case():
    """(65, 70): phenotype 12 (noise) has the same value at the positions 5 and 40 of the mask in ascending order"""
    n, ns = 65, 70
    c = plain_case(n, ns, 5)
    order = np.argsort(c["sample_of"], kind="stable")
    c["pheno"][NPHENO, order[40]] = c["pheno"][NPHENO, order[5]]
    swap = np.arange(n, dtype=np.uint32)
    swap[5], swap[40] = 40, 5
    return c, n, ns, swap


@pytest.mark.gpu
def test_exact_ties(dbtk, hip):
    c, n, ns, swap = tie_case()
    B = 5
    ident = np.tile(np.arange(n, dtype=np.uint32), (B, 1))
    mixed = np.vstack([pm.generate(n, 3, 11), swap[None, :]])
    A = pkg.Assoc(dbtk, ns, c["sample_of"], c["pheno"])
    d = put(hip, c["G"])
    try:
        A.set_pairs(*c["pairs"])
        A.set_permutations(B, perms=ident)
        A.perm_scan_device(d, c["G"].shape[0], nk_cum=c["nk_cum"])
        T, n_tests, bound, m = model_of(c, ident, c["pairs"])
        check(A, T, n_tests, bound, m, B)
        for p, r in enumerate(A.perm_results()):
            if n_tests[p]:
                assert r["n_ge"] == B and r["p_perm"] == 1.0
        A.set_permutations(4, perms=mixed)
        with pytest.raises(pkg.DbtkError):
            A.perm_results()              # new permutations invalidate the result
        A.perm_scan_device(d, c["G"].shape[0], nk_cum=c["nk_cum"])
        T, n_tests, bound, m = model_of(c, mixed, c["pairs"])
        check(A, T, n_tests, bound, m, 4)
        t = A.perm_stats(NPHENO)
        assert t[4] == t[0] and A.perm_stats(NPHENO + 1)[4] != A.perm_stats(NPHENO + 1)[0]
    finally:
        hip.free(d)
        A.close()


@pytest.mark.gpu
def test_the_plain_scan_fed_the_permuted_vectors_agrees(dbtk, hip):
    """a second oracle on the device: the B permuted vectors as explicit phenotypes of k_assoc_scan through a matching pair list"""
    n, ns, B, seed = ORACLE_CASE
    c = plain_case(n, ns, seed)
    perms = pm.generate(n, B, seed)
    T, n_tests, bound, m = model_of(c, perms, c["pairs"])
    P = c["pheno"].shape[0]
    order = np.argsort(c["sample_of"], kind="stable")
    ys = c["pheno"][:, order]
    explicit = np.zeros((P * B, n))
    for p in range(P):
        for b in range(B):
            explicit[p * B + b, order] = ys[p][perms[b]]
    off, idx = c["pairs"]
    eoff, eidx = [0], []
    for l in range(len(off) - 1):
        eidx += [p * B + b for p in idx[off[l]:off[l + 1]] for b in range(B)]
        eoff.append(len(eidx))
    A = pkg.Assoc(dbtk, ns, c["sample_of"], c["pheno"])
    E = pkg.Assoc(dbtk, ns, c["sample_of"], explicit)
    d = put(hip, c["G"])
    try:
        A.set_pairs(off, idx)
        A.set_permutations(B, perms=perms)
        A.perm_scan_device(d, c["G"].shape[0], nk_cum=c["nk_cum"])
        E.set_pairs(eoff, eidx)
        E.scan_device(d, c["G"].shape[0], nk_cum=c["nk_cum"])
        eb = E.best()
        for p in range(P):
            t = A.perm_stats(p)
            for b in range(B):
                assert eb[p * B + b]["n_tests"] == n_tests[p]
                if n_tests[p]:
                    assert abs(eb[p * B + b]["r"] ** 2 - t[b + 1]) <= 2 * bound[p], (p, b)
    finally:
        hip.free(d)
        A.close()
        E.close()


@pytest.mark.gpu
def test_perm_scan_pred_and_dosage(dbtk):
    """The matrices come from the handles themselves, as in test_assoc_gpu: after the bias correction, and the dosage values."""
    meta, counts, depths = make_cohort(3, ns=37, ntr=50, max_k=160)
    counts = counts & np.uint64((1 << 40) - 1)   # (see test_assoc_gpu: the generator's 2^40 outliers leave no margin)
    ns, ntr, B = 37, 50, 9
    rng = np.random.default_rng(1)
    sample_of = np.sort(rng.choice(np.arange(1, ns - 1), 30, replace=False))
    n = len(sample_of)
    perms = pm.generate(n, B, 3)
    off, idx = [0], []
    for l in range(ntr):
        idx += sorted(int(v) for v in rng.choice(6, int(rng.integers(0, 4)), replace=False))
        off.append(len(idx))
    P = pkg.Pred(dbtk, ns, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"], nk=meta["nk"])
    P.load(0, counts, depths)
    P.correct()
    D = pkg.Dosage(dbtk, ns, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"], nk=meta["nk"])
    D.load(0, counts, depths)
    D.finish()
    unit = np.arange(1, ntr + 1, dtype=np.uint32)
    for M, nk_cum, scan in ((P.matrix(), meta["nk_cum"], lambda A: A.perm_scan_pred(P, p_threshold=1e-3)), (D.values(), unit, lambda A: A.perm_scan_dosage(D, p_threshold=1e-3))):
        pheno = np.vstack([cohort_pheno(M, sample_of, 4, seed=6), np.random.default_rng(4).normal(0, 1, (2, n))])
        c = dict(G=M, sample_of=sample_of, pheno=pheno, nk_cum=nk_cum)
        T, n_tests, bound, m = model_of(c, perms, (off, idx))
        A = pkg.Assoc(dbtk, ns, sample_of, pheno)
        A.set_pairs(off, idx)
        with pytest.raises(pkg.DbtkError) as e:
            scan(A)
        assert e.value.status == abi.ERR_ARG and "no permutations are set" in str(e.value)
        A.set_permutations(B, seed=3)
        scan(A)
        check(A, T, n_tests, bound, m, B)
        A.close()
    P.close()
    D.close()


@pytest.mark.gpu
def test_perm_refusals_and_the_file(dbtk, hip, tmp_path):
    n, ns, B, seed = 65, 70, 7, 1
    c = plain_case(n, ns, seed)
    perms = pm.generate(n, B, seed)
    A = pkg.Assoc(dbtk, ns, c["sample_of"], c["pheno"], names=[f"gene{p}" for p in range(NPHENO + NOISE)])
    d = put(hip, c["G"])
    try:
        off, idx = c["pairs"]
        lone = [p for p in range(NPHENO) if p not in idx]
        A.set_pairs(off, idx)
        with pytest.raises(pkg.DbtkError) as e:
            A.perm_scan_device(d, c["G"].shape[0], nk_cum=c["nk_cum"])
        assert e.value.status == abi.ERR_ARG and "no permutations are set" in str(e.value)
        bad = perms.copy()
        bad[4, 7] = bad[4, 8]                                   # a value twice
        far = perms.copy()
        far[2, 0] = n                                           # a value off the end
        for pp, row in ((bad, 4), (far, 2)):
            with pytest.raises(pkg.DbtkError) as e:
                A.set_permutations(B, perms=pp)
            assert e.value.status == abi.ERR_ARG and f"row {row} is not a permutation" in str(e.value), str(e.value)
        with pytest.raises(pkg.DbtkError) as e:
            A.set_permutations(abi.ASSOC_PERM_MAX + 1, seed=1)
        assert e.value.status == abi.ERR_ARG and "DBTK_ASSOC_PERM_MAX" in str(e.value)
        assert A.permutations().shape == (0, n)                 # refused calls set nothing
        A.set_permutations(B, seed=seed)
        with pytest.raises(pkg.DbtkError):
            A.perm_results()                                    # before a scan
        with pytest.raises(pkg.DbtkError):
            A.perm_write(str(tmp_path / "early"))
        A.perm_scan_device(d, c["G"].shape[0], nk_cum=c["nk_cum"])
        res, best = A.perm_results(), A.best()
        A.perm_write(str(tmp_path / "o"))
        T = np.array([A.perm_stats(p) for p in range(A.P)])
        want = pm.perm_tsv([f"gene{p}" for p in range(A.P)], [b["n_tests"] for b in best], [b["row"] for b in best], T, [r["n_ge"] for r in res], [r["p_perm"] for r in res],
                           [r["q_perm"] for r in res])
        assert open(str(tmp_path / "o") + ".assoc.perm.tsv").read() == want
        assert (not lone) or "\t0\tNA\tNA\t7\tNA\tNA\tNA\n" in want
        rng = np.random.default_rng(3)
        A.set_covariates(rng.normal(0, 1, (2, n)))
        with pytest.raises(pkg.DbtkError):
            A.perm_results()                                    # covariates invalidate the result
        with pytest.raises(pkg.DbtkError):
            A.perm_stats(0)
        assert (A.permutations() == perms).all()                # the permutations themselves stay
        A.set_permutations(0)
        assert A.permutations().shape == (0, n)
    finally:
        hip.free(d)
        A.close()
