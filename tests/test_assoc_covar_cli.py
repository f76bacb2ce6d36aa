"""`--assoc-covar` on the two command lines.  danbing-tk-pred in the five-file and the --dosage form: OUTPREF.assoc.best.tsv and
OUTPREF.assoc.hits.tsv must be the model's text (tests/assoc_covar_model.py fed the matrix that the tool wrote, or the handle's dosage
values), exactly in the integer columns and the hit set, and within the tolerances of tests/test_assoc_covar_gpu.py, parsed back from
%.6e, in the others; two --assoc groups with different covariate files in one run; the same commands without --assoc-covar write the
bytes of the unchanged path (a run of that path in the same test).  `danbing-tk --cohort --pred --assoc --assoc-covar` writes the bytes of
danbing-tk-pred over the cohort's count files."""
import os
import subprocess
import sys

import numpy as np
import pytest

import assoc_covar_model as cm
import assoc_model
import bind
import cases
from test_assoc_cli import EXTS, PRED, read_bytes, write_pairs, write_table
from test_assoc_gpu import assert_margins
from test_assoc_covar_gpu import share_margins
from test_cohort import SETS, golden_ikmer_meta, make_samples, manifest, run
from test_pred import make_cohort

sys.path.insert(0, os.path.join(bind.ROOT, "oracle"))
import pred_oracle as PO  # noqa: E402

pkg = bind.pkg
pytestmark = pytest.mark.gpu
NS, NTR, N = 37, 50, 30


def rel6(v):
    """what %.6e keeps of v: half a unit of its seventh digit"""
    return 5.1e-7 * abs(v)


def text_equals_model(prefix, names, m, tol, neff, with_hits):
    """the integer columns and the hit set exactly; r, se, t, p, p_bonf within the derived tolerance plus the %.6e rounding"""
    lines = open(prefix + EXTS[0]).read().split("\n")
    want = cm.best_tsv(names, m["best"]).split("\n")
    assert lines[0] == want[0] and len(lines) == len(want) and lines[-1] == ""
    for line, wline, w in zip(lines[1:-1], want[1:-1], m["best"]):
        f, g = line.split("\t"), wline.split("\t")
        assert f[:5] == g[:5], (line, wline)
        if not w["n_tests"]:
            assert f == g
            continue
        t = tol[w["row"]]
        r, se, tt, p, pb = (float(v) for v in f[5:10])
        assert abs(r - w["r"]) <= t + rel6(w["r"])
        if abs(w["r"]) == 1.0:
            assert f[5:10] == g[5:10]
            continue
        tol_se = t * abs(w["r"]) / ((neff - 2) * w["se"]) + 4 * assoc_model.U * w["se"]
        assert abs(se - w["se"]) <= tol_se + rel6(w["se"])
        tol_t = abs(w["t"]) * (t / abs(w["r"]) + tol_se / w["se"] + 4 * assoc_model.U)
        assert abs(tt - w["t"]) <= tol_t + rel6(w["t"])
        lo, hi = assoc_model.pvalue(min(abs(w["r"]) + t, 1.0), neff), assoc_model.pvalue(max(abs(w["r"]) - t, 0.0), neff)
        assert lo * (1 - 5e-12) - rel6(lo) <= p <= hi * (1 + 5e-12) + rel6(hi)
        assert abs(pb - p * w["n_tests"]) <= 2 * rel6(pb)
    if not with_hits:
        assert not os.path.exists(prefix + EXTS[1])
        return
    lines = open(prefix + EXTS[1]).read().split("\n")
    want = cm.hits_tsv(names, m["hits"]).split("\n")
    assert lines[0] == want[0] and len(lines) == len(want)
    for line, wline, w in zip(lines[1:-1], want[1:-1], m["hits"]):
        f, g = line.split("\t"), wline.split("\t")
        assert f[:3] == g[:3] and abs(float(f[3]) - w[3]) <= tol[w[2]] + rel6(w[3])


def margins(lib, m, M, sample_of, pheno, q, p_threshold):
    tol = cm.tolerance(M, sample_of, pheno, q, m["share_x"], m["share_y"])
    share_margins(m)
    assert_margins(m, M, sample_of, tol, pkg.assoc_r2_threshold(lib, p_threshold, len(sample_of) - q) if p_threshold is not None else None)
    return tol


def test_pred_tool_with_covariates_in_both_forms(tmp_path):
    tmp = str(tmp_path)
    meta, counts, depths = make_cohort(3, ns=NS, ntr=NTR, max_k=160)
    counts = counts & np.uint64((1 << 40) - 1)   # (as tests/test_assoc_gpu.py: rows whose spread is a millionth of their mean keep no margin)
    nk = meta["nk"]
    ik = os.path.join(tmp, "ikmer.meta")
    PO.write_ikmer_meta(ik, nk, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"])
    with open(os.path.join(tmp, "gt.meta"), "w") as f:
        for s in range(NS):
            fn = os.path.join(tmp, f"s{s}.trkmc.ar")
            with open(fn, "wb") as g:
                g.write(np.uint64(nk).tobytes() + counts[s].tobytes())
            f.write(f"{fn}\t{float(depths[s])!r}\n")
    rng = np.random.default_rng(14)
    sample_of = rng.permutation(np.arange(2, NS - 1))[:N]
    names = [f"gene{i}" for i in range(4)]
    cov = [rng.integers(0, 3, (q, N)).astype(np.float64) + rng.normal(0, 0.3, (q, N)) for q in (3, 9)]
    cnames = [[f"pc{j}" for j in range(len(c))] for c in cov]
    tabs = []
    for i in range(2):
        pheno = rng.normal(0, 1, (4, N)) + (counts[sample_of][:, [11 + i, 500 + i, 900 + i, 1500 + i]].T / depths[sample_of][None, :]) * 0.5 + rng.normal(0, 0.7, (4, len(cov[i]))) @ cov[i]
        tabs.append(pheno)
        write_table(os.path.join(tmp, f"t{i}.tsv"), sample_of, pheno, names)
        shuffled = rng.permutation(N)            # the covariate file lists the samples in an order of its own
        write_table(os.path.join(tmp, f"c{i}.tsv"), sample_of[shuffled], cov[i][:, shuffled], cnames[i])
    off, idx = [0], []
    for l in range(NTR):
        idx += sorted(int(v) for v in rng.choice(4, int(rng.integers(0, 3)), replace=False))
        off.append(len(idx))
    write_pairs(os.path.join(tmp, "pairs.tsv"), off, idx, names)
    t0, t1, c0, c1, pairs = (os.path.join(tmp, x) for x in ("t0.tsv", "t1.tsv", "c0.tsv", "c1.tsv", "pairs.tsv"))
    five = [os.path.join(tmp, "gt.meta"), ik] + [os.path.join(tmp, x) for x in ("raw.gt", "cor.gt", "bias.tsv")]
    o = [os.path.join(tmp, f"o{i}") for i in range(4)]
    # two groups with their own covariates, a third without any, a fourth on the raw matrix
    r = subprocess.run([PRED, "--assoc", t0, o[0], "--assoc-covar", c0, "--assoc-p", "0.001", "--assoc", t1, o[1], "--assoc-pairs", pairs, "--assoc-p", "0.01", "--assoc-covar", c1,
                        "--assoc", t0, o[2], "--assoc-p", "0.001", "--assoc", t1, o[3], "--assoc-covar", c1, "--assoc-raw"] + five, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr.count("# assoc ") == 3 and f"# assoc {o[0]}: n {N}, 3 covariates, dof {N - 5}\n" in r.stderr and f"# assoc {o[1]}: n {N}, 9 covariates, dof {N - 11}\n" in r.stderr
    raw = np.fromfile(five[2], np.float32, offset=8).reshape(nk, NS)
    cor = np.fromfile(five[3], np.float32, offset=8).reshape(nk, NS)
    lib = pkg.Dbtk()
    order = np.argsort(sample_of, kind="stable")
    Qs = [pkg.assoc_covar_basis(lib, c[:, order]) for c in cov]   # the bases the handles made: the text went through repr() unchanged
    for prefix, M, tab, q, kw in ((o[0], cor, 0, 0, dict(p_threshold=0.001)), (o[1], cor, 1, 1, dict(pairs=(off, idx), p_threshold=0.01)), (o[3], raw, 1, 1, dict())):
        m = cm.scan(M, sample_of, tabs[tab], cov[q], Q=Qs[q], nk_cum=meta["nk_cum"], **kw)
        tol = margins(lib, m, M, sample_of, tabs[tab], len(cov[q]), kw.get("p_threshold"))
        text_equals_model(prefix, names, m, tol, N - len(cov[q]), "p_threshold" in kw)
    # the same commands without --assoc-covar: the bytes of the unchanged path, run here
    files = [open(f, "rb").read() for f in five[2:]]
    r = subprocess.run([PRED, "--assoc", t0, o[2] + "x", "--assoc-p", "0.001"] + five, capture_output=True, text=True)
    assert r.returncode == 0 and "# assoc" not in r.stderr
    assert read_bytes(o[2]) == read_bytes(o[2] + "x") and read_bytes(o[2])[0] != read_bytes(o[0])[0]
    assert [open(f, "rb").read() for f in five[2:]] == files
    P = pkg.Pred(lib, NS, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"], nk=nk)
    P.load(0, counts, depths)
    P.correct()
    A = pkg.Assoc(lib, NS, sample_of, tabs[0], names=names)
    A.scan_pred(P, p_threshold=0.001)
    A.write(o[2] + "lib")
    assert read_bytes(o[2] + "lib") == read_bytes(o[2])
    # and with covariates the tool writes what the library writes in this process
    A.set_covariates(cov[0], names=cnames[0])
    A.scan_pred(P, p_threshold=0.001)
    A.write(o[0] + "lib")
    assert read_bytes(o[0] + "lib") == read_bytes(o[0])
    A.close()
    P.close()
    # the dosage form: the rows are loci
    three = [five[0], ik, os.path.join(tmp, "dbias.tsv")]
    r = subprocess.run([PRED, "--assoc", t0, o[0] + "d", "--assoc-covar", c0, "--assoc-p", "0.05", "--assoc", t1, o[1] + "d", "--assoc-covar", c1, "--assoc-pairs", pairs,
                        "--dosage", os.path.join(tmp, "dos.tsv")] + three, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    D = pkg.Dosage(lib, NS, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"], nk=nk)
    D.load(0, counts, depths)
    D.finish()
    V = D.values()
    D.close()
    unit = np.arange(1, NTR + 1, dtype=np.uint32)
    for prefix, tab, q, kw in ((o[0] + "d", 0, 0, dict(p_threshold=0.05)), (o[1] + "d", 1, 1, dict(pairs=(off, idx)))):
        m = cm.scan(V, sample_of, tabs[tab], cov[q], Q=Qs[q], nk_cum=unit, **kw)
        tol = margins(lib, m, V, sample_of, tabs[tab], len(cov[q]), kw.get("p_threshold"))
        text_equals_model(prefix, names, m, tol, N - len(cov[q]), "p_threshold" in kw)
    # a phenotype that the covariates explain is refused when they are set, with its name
    inside = tabs[0].copy()
    inside[2] = 1.0 + cov[0][0] - 2.0 * cov[0][2]
    write_table(os.path.join(tmp, "inside.tsv"), sample_of, inside, names)
    r = subprocess.run([PRED, "--assoc", os.path.join(tmp, "inside.tsv"), o[0] + "i", "--assoc-covar", c0] + five, capture_output=True, text=True)
    assert r.returncode == 1 and "--assoc-covar" in r.stderr and "phenotype gene2 is explained by the covariates" in r.stderr and not os.path.exists(o[0] + "i" + EXTS[0])


def test_cohort_assoc_covar_equals_the_pred_tool(tmp_path):
    spec = SETS["g1"]
    gdir = os.path.join(cases.GOLDEN, spec["dir"])
    tmp = str(tmp_path)
    files = make_samples(gdir, tmp)
    ns = len(files)
    depths = [30.5, 0.75, 41.0, 17.25, 3.0, 55.125][:ns]
    ik = os.path.join(tmp, "ikmer.meta")
    meta = golden_ikmer_meta(gdir, ik)
    with open(os.path.join(tmp, "gt.meta.txt"), "w") as f:
        for i, d in enumerate(depths):
            f.write("%s.trkmc.ar\t%r\n" % (os.path.join(tmp, "coh", "c%d" % i), d))
    rng = np.random.default_rng(6)
    sample_of = [5, 0, 2, 3, 1]
    names = ["a", "b", "c"]
    pheno = rng.normal(0, 1, (3, len(sample_of)))
    table, covar, pairs = (os.path.join(tmp, x) for x in ("pheno.tsv", "covar.tsv", "pairs.tsv"))
    write_table(table, sample_of, pheno, names)
    write_table(covar, sample_of[::-1], np.array([[1.0, 0.0, 0.0, 1.0, 0.5]]), ["sex"])
    off = list(range(meta["ntr"] + 1))
    idx = [l % 3 for l in range(meta["ntr"])]
    write_pairs(pairs, off, idx, names)

    def groups(tag, cv):
        g0 = ["--assoc", table, os.path.join(tmp, tag + "0")] + cv + ["--assoc-p", "0.5"]
        return g0 + ["--assoc", table, os.path.join(tmp, tag + "1"), "--assoc-pairs", pairs, "--assoc-raw"] + cv

    os.makedirs(os.path.join(tmp, "coh"))
    rows = [(f, os.path.join(tmp, "coh", "c%d" % i), repr(dp)) for i, (f, dp) in enumerate(zip(files, depths))]
    coh = [os.path.join(tmp, "coh." + x) for x in ("raw.gt", "cor.gt", "bias.tsv")]
    two = [os.path.join(tmp, "two." + x) for x in ("raw.gt", "cor.gt", "bias.tsv")]
    cv = ["--assoc-covar", covar]
    r = run(spec["flags"] + ["--cohort", manifest(tmp_path / "m.tsv", rows), "--pred", ik] + coh + groups("c", cv), cwd=gdir)
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-3000:]
    assert r.stderr.count(b"# assoc ") == 2 and b"n 5, 1 covariates, dof 2\n" in r.stderr
    r = subprocess.run([PRED] + groups("p", cv) + [os.path.join(tmp, "gt.meta.txt"), ik] + two, capture_output=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([PRED] + groups("n", []) + [os.path.join(tmp, "gt.meta.txt"), ik] + two, capture_output=True)
    assert r.returncode == 0, r.stderr
    for i in range(2):
        x = read_bytes(os.path.join(tmp, "c%d" % i))
        assert x == read_bytes(os.path.join(tmp, "p%d" % i)) and x[0].count(b"\n") == 4, i
        assert x[0] != read_bytes(os.path.join(tmp, "n%d" % i))[0]       # the covariates changed the numbers
    # the counts of tests against the model on the matrix the run wrote (dof 2: the numbers themselves are held by the test above)
    cor = np.fromfile(coh[1], np.float32, offset=8).reshape(meta["nk"], ns)
    cvals = np.array([[1.0, 0.0, 0.0, 1.0, 0.5]])[:, ::-1]
    m = cm.scan(cor, sample_of, pheno, cvals, nk_cum=meta["nk_cum"])
    ok = (m["share_x"][np.isfinite(m["share_x"])] > 1000 * cm.COLLINEAR) | (m["share_x"][np.isfinite(m["share_x"])] < cm.COLLINEAR / 1000)
    for line, w in zip(open(os.path.join(tmp, "c0") + EXTS[0]).read().split("\n")[1:-1], m["best"]):
        f = line.split("\t")
        assert not ok.all() or (int(f[1]), int(f[2])) == (w["n_tests"], w["skipped"])
        assert int(f[1]) + int(f[2]) == w["n_tests"] + w["skipped"] and int(f[1]) > 0
