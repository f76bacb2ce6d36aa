"""The association scan on the GPU (include/dbtk_assoc.h, csrc/dbtk_assoc.hip) at library level, against tests/assoc_model.py fed the
same float32 inputs.

The tolerance is derived, not measured.  Model and kernel both work in float64 on the same widened float32 entries and differ in the
ORDER of their sums only.  With u = 2^-53: a sum of n float64 terms in any order has a relative error of at most (n - 1) u against the
sum of the absolute values of its terms (Higham, Accuracy and Stability, 4.4).  Sxx and Syy have positive terms, so each is right to
(n + 2) u relative (the + 2: the subtraction and the product of each term).  Sxy = sum dx dy is right to (n + 2) u sum |dx dy|, and by
Cauchy-Schwarz sum |dx dy| <= sqrt(Sxx Syy): an ABSOLUTE error of (n + 2) u in r.  The square root of the denominator halves the two
relative errors of Sxx and Syy and adds one rounding, the division another: |r| ((n + 2) u + 2 u).  An error dm in a row's mean shifts
every dx by the same amount: it enters Sxx as n dm^2 and Sxy as dm sum dy, and sum dy is itself only a rounding residue, so both are of
second order in u; what is of first order is the rounding of each dx = fl(x - m), relative u of |dx| but, where |m| >> sd, carrying the
mean's own error n u max|x| / sd relative to the row's spread.  So per side |dr| <= 2 (n + 4) u (1 + kappa), kappa = max|v| / sd(v) over
the row and the phenotypes (the row's conditioning: a row that the bias correction left constant up to float32 rounding is tested, and its
r is rounding noise on both sides), and between the two sides, per row,
    TOL_R = 4 (n + 4) 2^-53 (1 + kappa)                                         (assoc_model.tolerance)
se = sqrt((1 - r^2) / (n - 2)) moves by |r| dr / ((n - 2) se) and two roundings; t = r / se by |t| (dr / |r| + dse / se).  p is a
function of r alone: it must lie between the model's p at |r| - TOL_R and at |r| + TOL_R (widened by the 2.2e-12 of
tests/test_assoc_host.py on each side).  n_tests, skipped, rows, loci and the hit set compare EXACTLY; for that every test first asserts
that its own inputs keep each best-versus-runner-up gap in r^2, and each distance of a tested pair's r^2 from the kernel's threshold, at
1000 times the bound of the rows involved (rows that are copies of the best row are no runners-up: they tie bit for bit, and the lower row must win)."""
import math
import os

import numpy as np
import pytest

import assoc_model
import bind
from test_pred import make_cohort
from test_pred_device import _Hip

abi, pkg = bind.abi, bind.pkg

# loci of 0, 1, tile - 1, tile, tile + 1 rows, one past a workgroup's pass (32), one past a work item (256); their phenotypes: none for
# one locus, chunk + 1 for two; 6 trailing rows of no locus
LOCUS_ROWS = [0, 1, 3, 4, 5, 40, 300]
LOCUS_PHENOS = [2, 3, 0, 9, 3, 9, 3]
TRAILING = 6
NPHENO = 12
# (n, ns): the issue's n; the last n whose rows stay in registers and the first that does not (= a second LDS segment); a third segment
MASKS = [(3, 9), (63, 70), (64, 70), (65, 70), (130, 140), (512, 520), (513, 520), (1100, 1111)]
HITS_SMALL = 64
P_THRESHOLD = 0.05


@pytest.fixture(scope="module")
def dbtk():
    return pkg.Dbtk()


@pytest.fixture(scope="module")
def hip():
    return _Hip()


def mask_of(n, ns, rng):
    """n of ns samples: sample 0, the last one and one in the middle are always masked out"""
    out = {0, ns - 1, ns // 2}
    rest = [s for s in range(ns) if s not in out]
    out |= set(int(v) for v in rng.choice(rest, ns - n - 3, replace=False))
    keep = np.array([s for s in range(ns) if s not in out], np.int64)
    assert len(keep) == n
    return rng.permutation(keep)  # (the table may list the samples in any order)


def hand_made(n, ns, seed):
    rng = np.random.default_rng(seed)
    nk_cum = np.cumsum(LOCUS_ROWS).astype(np.uint32)
    nrows = int(nk_cum[-1]) + TRAILING
    sample_of = mask_of(n, ns, rng)
    G = rng.gamma(2.0, 1.5, (nrows, ns)).astype(np.float32)
    masked = np.setdiff1d(np.arange(ns), sample_of)
    G[::3, masked[0]] = np.nan           # outside the mask anything may stand: these rows are tested all the same
    G[1::5, masked[-1]] = np.inf
    pheno = rng.normal(0, 1, (NPHENO, n))
    for p in range(NPHENO):              # every phenotype leans on a row of its own, so that its best row stands clear of the rest
        pheno[p] += 0.8 * G[(37 * p + 11) % nrows, sample_of] / 1.5
    off, idx = [0], []
    for l, k in enumerate(LOCUS_PHENOS):
        idx += sorted(int(v) for v in rng.choice(NPHENO, k, replace=False))
        off.append(len(idx))
    r40 = int(nk_cum[4])                 # the locus of 40 rows carries the special rows
    G[r40 + 2, :] = 2.5                                                    # constant
    G[r40 + 3, sample_of[n // 2]] = np.inf                                  # one inf inside the mask
    G[r40 + 4, :] = 1.0
    G[r40 + 4, sample_of[1]] = 3.0                                          # a single sample differs
    p_one = idx[off[5]]                                                     # a phenotype of that locus
    pheno[p_one] = rng.gamma(2.0, 1.5, n).astype(np.float32).astype(np.float64)
    G[r40 + 7, sample_of] = pheno[p_one].astype(np.float32)                 # a row that equals a phenotype: r = 1, p = 0
    p_tie = idx[off[5] + 1]
    G[r40 + 20] = G[r40 + 9]                                                # duplicate rows: a tie in r^2, the lower row wins
    pheno[p_tie] = rng.normal(0, 1, n) + 2.0 * G[r40 + 9, sample_of]
    if n == 3:                                                              # (3 points: keep the leaning phenotypes off a perfect fit)
        pheno[p_tie] = rng.normal(0, 1, n) + 0.5 * G[r40 + 9, sample_of]
    return dict(G=G, ns=ns, sample_of=sample_of, pheno=pheno, nk_cum=nk_cum, pairs=(off, idx), r40=r40, p_one=p_one, p_tie=p_tie)


def assert_margins(m, G, sample_of, tol, r2crit):
    """the inputs keep every decision that the test compares exactly 1000 bounds away from its edge"""
    cols = np.sort(np.asarray(sample_of))
    r2 = m["r"] * m["r"]
    use = m["paired"] & m["tested"][:, None]
    tol2 = 2.0 * tol                     # per row: d(r^2) <= 2 |r| dr
    for p, b in enumerate(m["best"]):
        if not b["n_tests"]:
            continue
        same = np.array([G[row, cols].tobytes() == G[b["row"], cols].tobytes() for row in range(G.shape[0])])
        rest = use[:, p] & ~same
        if rest.any():
            gap = b["r"] ** 2 - r2[rest, p]
            assert (gap >= 1000 * np.maximum(tol2[rest], tol2[b["row"]])).all(), (p, b["row"], gap.min())
        assert b["row"] == min(np.nonzero(use[:, p] & same)[0])
    if r2crit is not None:
        d = np.abs(r2 - r2crit)
        assert (d[use] >= 1000 * np.broadcast_to(tol2[:, None], d.shape)[use]).all(), d[use].min()


def compare(best, hits, m, n, tols):
    for p, (g, w) in enumerate(zip(best, m["best"])):
        tol = tols[w["row"]] if w["n_tests"] else 0.0
        assert (g["n_tests"], g["skipped"], g["row"], g["locus"]) == (w["n_tests"], w["skipped"], w["row"], w["locus"]), (p, g, w)
        if not w["n_tests"]:
            assert g["r"] == 0 and g["p"] == 0 and g["q"] == 0
            continue
        assert abs(g["r"] - w["r"]) <= tol, (p, g["r"], w["r"], tol)
        if abs(w["r"]) == 1.0:
            assert g["r"] == w["r"] and g["se"] == 0.0 and g["t"] == w["t"] and g["p"] == 0.0 and g["p_bonf"] == 0.0
        else:
            tol_se = tol * abs(w["r"]) / ((n - 2) * w["se"]) + 4 * assoc_model.U * w["se"]
            assert abs(g["se"] - w["se"]) <= tol_se, (p, g["se"], w["se"], tol_se)
            tol_t = abs(w["t"]) * (tol / max(abs(w["r"]), 1e-300) + tol_se / w["se"] + 4 * assoc_model.U)
            assert abs(g["t"] - w["t"]) <= tol_t, (p, g["t"], w["t"], tol_t)
            lo, hi = assoc_model.pvalue(min(abs(w["r"]) + tol, 1.0), n), assoc_model.pvalue(max(abs(w["r"]) - tol, 0.0), n)
            assert lo * (1 - 5e-12) <= g["p"] <= hi * (1 + 5e-12), (p, lo, g["p"], hi)
        assert g["p_bonf"] == g["p"] * g["n_tests"]
    have = [p for p in range(len(best)) if best[p]["n_tests"]]
    q = assoc_model.bh([best[p]["p_bonf"] for p in have])
    assert np.allclose([best[p]["q"] for p in have], q, rtol=1e-14, atol=0)
    if m["hits"] is not None:
        assert [(h[0], h[1], h[2]) for h in hits] == [(h[0], h[1], h[2]) for h in m["hits"]]
        for g, w in zip(hits, m["hits"]):
            assert abs(g[3] - w[3]) <= tols[w[2]]


def put(hip, G):
    return hip.put(np.ascontiguousarray(G, np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("n,ns", MASKS)
def test_scan_device_on_hand_made_matrices(dbtk, hip, n, ns):
    c = hand_made(n, ns, seed=100 + n)
    G, sample_of, pheno, nk_cum = c["G"], c["sample_of"], c["pheno"], c["nk_cum"]
    tol = assoc_model.tolerance(G, sample_of, pheno)
    assert tol.max() < 1e-9
    A = pkg.Assoc(dbtk, ns, sample_of, pheno)
    r2crit = pkg.assoc_r2_threshold(dbtk, P_THRESHOLD, n)
    d = put(hip, G)
    try:
        # every phenotype against every row (the trailing rows included)
        m = assoc_model.scan(G, sample_of, pheno, nk_cum=nk_cum, p_threshold=P_THRESHOLD)
        assert_margins(m, G, sample_of, tol, r2crit)
        A.scan_device(d, G.shape[0], nk_cum=nk_cum, p_threshold=P_THRESHOLD)
        best = A.best()
        compare(best, A.hits(), m, n, tol)
        assert all(b["n_tests"] == G.shape[0] - 2 and b["skipped"] == 2 for b in best)      # the constant row and the row with an inf
        one = best[c["p_one"]]
        assert one["row"] == c["r40"] + 7 and one["r"] == 1.0 and one["p"] == 0.0 and one["t"] == math.inf and one["locus"] == 5
        assert best[c["p_tie"]]["row"] == c["r40"] + 9 or n == 3
        assert m["tested"][c["r40"] + 4] and not m["tested"][c["r40"] + 2] and not m["tested"][c["r40"] + 3]
        # the same without locus boundaries: every locus reads NONE
        A.scan_device(d, G.shape[0], p_threshold=-1.0)
        nb = A.best()
        assert all(b["locus"] == abi.ASSOC_NONE for b in nb) and [b["row"] for b in nb] == [b["row"] for b in best]
        with pytest.raises(pkg.DbtkError):
            A.hits()
        # the pair list
        A.set_pairs(*c["pairs"])
        mp = assoc_model.scan(G, sample_of, pheno, nk_cum=nk_cum, pairs=c["pairs"], p_threshold=P_THRESHOLD)
        assert_margins(mp, G, sample_of, tol, r2crit)
        A.scan_device(d, G.shape[0], nk_cum=nk_cum, p_threshold=P_THRESHOLD)
        bp, hp = A.best(), A.hits()
        compare(bp, hp, mp, n, tol)
        assert bp[c["p_one"]]["r"] == 1.0 and (bp[c["p_tie"]]["row"] == c["r40"] + 9 or n == 3)
        assert any(b["n_tests"] == 0 for b in bp) or len(set(c["pairs"][1])) == NPHENO
        assert all(h[2] < int(nk_cum[-1]) for h in hp)                                        # no trailing row is tested
        # twice the same bytes
        A.scan_device(d, G.shape[0], nk_cum=nk_cum, p_threshold=P_THRESHOLD)
        assert A.best() == bp and A.hits() == hp
    finally:
        hip.free(d)
        A.close()


@pytest.mark.gpu
def test_hit_buffer_overflow_is_an_error_with_the_count(dbtk, hip, tmp_path):
    """DBTK_ASSOC_HITS = 64: 13 rows x 5 phenotypes = 65 hits overflow (the message names the knob and the 65, the best table is
    complete, no list is handed out); 16 x 4 = 64 hits fit."""
    rng = np.random.default_rng(7)
    ns = n = 20
    old = os.environ.get("DBTK_ASSOC_HITS")
    os.environ["DBTK_ASSOC_HITS"] = str(HITS_SMALL)
    try:
        for nrows, P, over in ((13, 5, True), (16, 4, False)):
            G = rng.normal(0, 1, (nrows, ns)).astype(np.float32)
            pheno = rng.normal(0, 1, (P, n))
            A = pkg.Assoc(dbtk, ns, np.arange(n), pheno)
            d = put(hip, G)
            m = assoc_model.scan(G, np.arange(n), pheno, p_threshold=1.0)
            assert len(m["hits"]) == nrows * P
            if over:
                with pytest.raises(pkg.DbtkError) as e:
                    A.scan_device(d, nrows, p_threshold=1.0)
                assert e.value.status == abi.ERR_OVERFLOW and "DBTK_ASSOC_HITS" in str(e.value) and "65" in str(e.value)
                assert [b["row"] for b in A.best()] == [b["row"] for b in m["best"]]
                with pytest.raises(pkg.DbtkError):
                    A.hits()
                A.scan_device(d, nrows, p_threshold=-1.0)   # without a list the same scan is fine
            else:
                A.scan_device(d, nrows, p_threshold=1.0)
                assert [(h[0], h[2]) for h in A.hits()] == [(h[0], h[2]) for h in m["hits"]] and len(A.hits()) == HITS_SMALL
            hip.free(d)
            A.close()
        os.environ["DBTK_ASSOC_HITS"] = "48"
        with pytest.raises(pkg.DbtkError) as e:
            pkg.Assoc(dbtk, ns, np.arange(n), pheno)
        assert e.value.status == abi.ERR_ARG and "power of two" in str(e.value)
    finally:
        if old is None:
            del os.environ["DBTK_ASSOC_HITS"]
        else:
            os.environ["DBTK_ASSOC_HITS"] = old


def cohort_pheno(M, sample_of, P, seed):
    rng = np.random.default_rng(seed)
    n = len(sample_of)
    x, tested, _, _ = assoc_model.row_stats(M, sample_of)
    rows = np.nonzero(tested)[0]
    pheno = rng.normal(0, 1, (P, n))
    for p in range(P):
        v = x[rows[(p * 17 + 3) % len(rows)]]
        pheno[p] += 1.5 * (v - v.mean()) / v.std()
    return pheno


@pytest.mark.gpu
def test_scan_pred_before_and_after_the_correction_and_scan_dosage(dbtk, tmp_path):
    """The matrices come from the handles themselves (dbtk_pred_matrix, dbtk_dosage_values): the model is fed what the scan read."""
    meta, counts, depths = make_cohort(3, ns=37, ntr=50, max_k=160)
    # (the generator adds 2^40 to five k-mers in every sample: rows whose spread is a millionth of their mean.  The bound scales with
    # that conditioning, and no margin of this test would survive it; they are taken off again)
    counts = counts & np.uint64((1 << 40) - 1)
    ns, ntr = 37, 50
    rng = np.random.default_rng(1)
    sample_of = np.sort(rng.choice(np.arange(1, ns - 1), 30, replace=False))
    n = len(sample_of)
    P = pkg.Pred(dbtk, ns, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"], nk=meta["nk"])
    P.load(0, counts, depths)
    off = [0]
    idx = []
    for l in range(ntr):
        idx += sorted(int(v) for v in rng.choice(6, int(rng.integers(0, 4)), replace=False))
        off.append(len(idx))
    for stage in ("raw", "corrected"):
        if stage == "corrected":
            P.correct()
        M = P.matrix()
        pheno = cohort_pheno(M, sample_of, 6, seed=len(stage))
        tol = assoc_model.tolerance(M, sample_of, pheno)
        A = pkg.Assoc(dbtk, ns, sample_of, pheno, names=[f"gene{i}" for i in range(6)])
        for pairs in (None, (off, idx)):
            if pairs:
                A.set_pairs(*pairs)
            m = assoc_model.scan(M, sample_of, pheno, nk_cum=meta["nk_cum"], pairs=pairs, p_threshold=1e-3)
            assert_margins(m, M, sample_of, tol, pkg.assoc_r2_threshold(dbtk, 1e-3, n))
            A.scan_pred(P, p_threshold=1e-3)
            compare(A.best(), A.hits(), m, n, tol)
        A.write(str(tmp_path / stage))
        text = open(str(tmp_path / stage) + ".assoc.best.tsv").read().split("\n")
        assert text[0] == "pheno\tn_tests\tskipped\tlocus\trow\tr\tse\tt\tp\tp_bonf\tq" and text[1].startswith("gene0\t") and len(text) == 8
        assert open(str(tmp_path / stage) + ".assoc.hits.tsv").readline() == "pheno\tlocus\trow\tr\tt\tp\n"
        assert A.times()[0] > 0
        A.close()
    # the refusals
    pheno = cohort_pheno(M, sample_of, 2, seed=5)
    A = pkg.Assoc(dbtk, ns, sample_of, pheno)
    W = pkg.PredWindowed(dbtk, ns, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"], 400, nk=meta["nk"])
    other = pkg.Assoc(dbtk, ns + 1, sample_of, pheno)
    A.set_pairs([0, 1, 2], [0, 1])   # a pair list over 2 loci, the matrix has 50
    for call, msg in ((lambda: A.scan_pred(W), "windowed"), (lambda: other.scan_pred(P), "samples"), (lambda: A.scan_pred(P), "2 loci")):
        with pytest.raises(pkg.DbtkError) as e:
            call()
        assert e.value.status == abi.ERR_ARG and msg in str(e.value), str(e.value)
    with pytest.raises(pkg.DbtkError):
        A.best()                      # a refused scan leaves no result behind
    W.close()
    other.close()
    A.set_pairs([], [])
    # dosage: the rows are loci, locus l's group is l
    D = pkg.Dosage(dbtk, ns, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"], nk=meta["nk"])
    D.load(0, counts, depths)
    with pytest.raises(pkg.DbtkError) as e:
        A.scan_dosage(D)
    assert e.value.status == abi.ERR_ARG and "unfinished" in str(e.value)
    D.finish()
    V = D.values()
    pheno = cohort_pheno(V, sample_of, 5, seed=8)
    B = pkg.Assoc(dbtk, ns, sample_of, pheno)
    tol = assoc_model.tolerance(V, sample_of, pheno)
    unit = np.arange(1, ntr + 1, dtype=np.uint32)
    doff = list(range(0, 2 * ntr + 1, 2))
    didx = [int(v) for l in range(ntr) for v in sorted(((l % 5), (l * 3 + 1) % 5))]
    for pairs in (None, (doff, didx)):
        if pairs:
            B.set_pairs(*pairs)
        m = assoc_model.scan(V, sample_of, pheno, nk_cum=unit, pairs=pairs, p_threshold=0.01)
        assert_margins(m, V, sample_of, tol, pkg.assoc_r2_threshold(dbtk, 0.01, n))
        B.scan_dosage(D, p_threshold=0.01)
        compare(B.best(), B.hits(), m, n, tol)
        assert all(b["locus"] == b["row"] for b in B.best() if b["n_tests"])
    for x in (A, B, D, P):
        x.close()


@pytest.mark.gpu
def test_create_refusals(dbtk):
    ns = 12
    good = np.arange(12.0).reshape(1, 12) ** 2
    cases = [
        (np.arange(2), good[:, :2], "at least 3"),
        (np.array([0, 1, 12]), good[:, :3], "sample 12 >="),
        (np.array([0, 4, 4]), good[:, :3], "sample 4 is given twice"),
        (np.arange(4), np.array([[1.0, 2.0, np.nan, 3.0]]), "not finite"),
        (np.arange(4), np.array([[1.0, 2.0, np.inf, 3.0]]), "not finite"),
        (np.arange(4), np.array([[1.0, 2.0, 0.0, 3.0], [5.0, 5.0, 5.0, 5.0]]), "phenotype height is constant"),
    ]
    for sample_of, pheno, msg in cases:
        with pytest.raises(pkg.DbtkError) as e:
            pkg.Assoc(dbtk, ns, sample_of, pheno, names=["weight", "height"][:pheno.shape[0]])
        assert e.value.status == abi.ERR_ARG and msg in str(e.value), str(e.value)
    rng = np.random.default_rng(2)
    A = pkg.Assoc(dbtk, ns, np.arange(ns), rng.normal(0, 1, (65, ns)))
    h = _Hip()
    d = h.put(rng.normal(0, 1, (5, ns)).astype(np.float32))
    try:
        with pytest.raises(pkg.DbtkError) as e:
            A.scan_device(d, 5)
        assert e.value.status == abi.ERR_ARG and "65 phenotypes" in str(e.value)
        for off, idx, msg in (([0, 1], [65], "index 65"), ([0, 2, 1], [0, 1], "decreases"), ([1, 2], [0, 1], "off[0]")):
            with pytest.raises(pkg.DbtkError) as e:
                A.set_pairs(off, idx)
            assert e.value.status == abi.ERR_ARG and msg in str(e.value), str(e.value)
        A.set_pairs([0, 65], list(range(65)))   # with a pair list 65 phenotypes are fine
        A.scan_device(d, 5, nk_cum=[5])
        assert all(b["n_tests"] == 5 for b in A.best())
        with pytest.raises(pkg.DbtkError) as e:
            A.scan_device(d, 5, nk_cum=[6])
        assert e.value.status == abi.ERR_ARG
        with pytest.raises(pkg.DbtkError) as e:
            A.scan_device(A.pheno.ctypes.data, 5, nk_cum=[5])   # host memory
        assert e.value.status == abi.ERR_ARG and "device memory" in str(e.value)
    finally:
        h.free(d)
        A.close()
