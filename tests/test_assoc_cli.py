"""`--assoc` on the two command lines.  danbing-tk-pred in both forms (five files; --dosage), with and without a pair list, two --assoc
groups in one run, --assoc-raw: the files must be the bytes that the library writes in this process for the same counts, depths and
tables (tests/test_assoc_gpu.py holds the library against the model), and the best rows are checked against the model fed the matrix
that the tool wrote.  `danbing-tk --cohort --pred|--dosage --assoc` on the small cohort of tests/test_cohort.py: byte for byte the files
of danbing-tk-pred --assoc over the cohort's count files, and the other outputs are the bytes of the run without the flags."""
import os
import subprocess
import sys

import numpy as np
import pytest

import assoc_model
import bind
import cases
from test_cohort import SETS, golden_ikmer_meta, make_samples, manifest, run
from test_pred import make_cohort

sys.path.insert(0, os.path.join(bind.ROOT, "oracle"))
import pred_oracle as PO  # noqa: E402

pkg = bind.pkg
PRED = os.path.join(bind.ROOT, "danbing-tk_amd", "bin", "danbing-tk-pred")
EXTS = (".assoc.best.tsv", ".assoc.hits.tsv")

pytestmark = pytest.mark.gpu


def write_table(fn, sample_of, pheno, names):
    with open(fn, "w") as f:
        f.write("id\t" + "\t".join(names) + "\n")
        for j, s in enumerate(sample_of):
            f.write(f"{s}\t" + "\t".join(repr(float(v)) for v in pheno[:, j]) + "\n")


def write_pairs(fn, off, idx, names):
    with open(fn, "w") as f:
        for l in range(len(off) - 1):
            for p in idx[off[l]:off[l + 1]]:
                f.write(f"{l}\t{names[p]}\n")
        first = next(l for l in range(len(off) - 1) if off[l + 1] > off[l])
        f.write(f"{first}\t{names[idx[0]]}\n")   # a line given twice counts once


def read_bytes(prefix):
    return [open(prefix + e, "rb").read() if os.path.exists(prefix + e) else None for e in EXTS]


def test_pred_tool_in_both_forms(tmp_path):
    tmp = str(tmp_path)
    meta, counts, depths = make_cohort(3, ns=37, ntr=50, max_k=160)
    ns, ntr, nk = 37, 50, meta["nk"]
    ik = os.path.join(tmp, "ikmer.meta")
    PO.write_ikmer_meta(ik, nk, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"])
    with open(os.path.join(tmp, "gt.meta"), "w") as f:
        for s in range(ns):
            fn = os.path.join(tmp, f"s{s}.trkmc.ar")
            with open(fn, "wb") as g:
                g.write(np.uint64(nk).tobytes() + counts[s].tobytes())
            f.write(f"{fn}\t{float(depths[s])!r}\n")
    rng = np.random.default_rng(4)
    sample_of = rng.permutation(np.arange(2, ns - 1))[:30]
    names = [f"gene{i}" for i in range(4)]
    tabs = []
    for i in range(2):
        pheno = rng.normal(0, 1, (4, 30)) + (counts[sample_of][:, [11 + i, 500 + i, 900 + i, 1500 + i]].T / depths[sample_of][None, :]) * 0.5
        tabs.append(pheno)
        write_table(os.path.join(tmp, f"t{i}.tsv"), sample_of, pheno, names)
    off, idx = [0], []
    for l in range(ntr):
        idx += sorted(int(v) for v in rng.choice(4, int(rng.integers(0, 3)), replace=False))
        off.append(len(idx))
    write_pairs(os.path.join(tmp, "pairs.tsv"), off, idx, names)
    t0, t1, pairs = (os.path.join(tmp, x) for x in ("t0.tsv", "t1.tsv", "pairs.tsv"))
    five = [os.path.join(tmp, "gt.meta"), ik] + [os.path.join(tmp, x) for x in ("raw.gt", "cor.gt", "bias.tsv")]
    # without the flags first: the three files that the flags must leave alone
    r = subprocess.run([PRED] + five, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    plain = [open(f, "rb").read() for f in five[2:]]
    o = [os.path.join(tmp, f"o{i}") for i in range(4)]
    r = subprocess.run([PRED, "--assoc", t0, o[0], "--assoc-p", "0.001", "--assoc", t1, o[1], "--assoc-pairs", pairs, "--assoc-p", "0.01",
                        "--assoc", t0, o[2], "--assoc-raw", "--assoc", t1, o[3], "--assoc-pairs", pairs, "--assoc-raw", "--assoc-p", "1"] + five, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [open(f, "rb").read() for f in five[2:]] == plain and r.stdout.count("association scan of") == 4
    # the library in this process
    lib = pkg.Dbtk()
    P = pkg.Pred(lib, ns, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"], nk=nk)
    P.load(0, counts, depths)
    mine = [os.path.join(tmp, f"m{i}") for i in range(4)]

    def scan(tab, prefix, with_pairs, p, target, how):
        A = pkg.Assoc(lib, ns, sample_of, tab, names=names)
        if with_pairs:
            A.set_pairs(off, idx)
        getattr(A, how)(target, p_threshold=p)
        A.write(prefix)
        best = A.best()
        A.close()
        return best

    scan(tabs[0], mine[2], False, -1.0, P, "scan_pred")
    scan(tabs[1], mine[3], True, 1.0, P, "scan_pred")
    P.correct()
    best0 = scan(tabs[0], mine[0], False, 0.001, P, "scan_pred")
    scan(tabs[1], mine[1], True, 0.01, P, "scan_pred")
    for a, b in zip(o, mine):
        x, y = read_bytes(a), read_bytes(b)
        assert x == y and x[0] is not None and len(x[0]) > 100, a
    assert read_bytes(o[2])[1] is None and read_bytes(o[0])[1].count(b"\n") > 1 and read_bytes(o[3])[1].count(b"\n") > 1000
    # the best rows of the first table against the model fed the corrected matrix as the tool wrote it
    cor = np.frombuffer(plain[1][8:], np.float32).reshape(nk, ns)
    m = assoc_model.scan(cor, sample_of, tabs[0], nk_cum=meta["nk_cum"])
    lines = open(o[0] + EXTS[0]).read().split("\n")[1:-1]
    for line, w, g in zip(lines, m["best"], best0):
        f = line.split("\t")
        assert (int(f[1]), int(f[2]), int(f[3]), int(f[4])) == (w["n_tests"], w["skipped"], w["locus"], w["row"]) and f[5] == "%.6e" % g["r"]
        assert abs(float(f[5]) - w["r"]) < 1e-6 and abs(float(f[8]) - w["p"]) <= 1e-5 * w["p"]
    P.close()
    # the dosage form: the rows are loci
    three = [five[0], ik, os.path.join(tmp, "dbias.tsv")]
    r = subprocess.run([PRED, "--assoc", t0, o[0] + "d", "--assoc-p", "0.05", "--assoc", t1, o[1] + "d", "--assoc-pairs", pairs, "--dosage", os.path.join(tmp, "dos.tsv")] + three,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(three[2], "rb").read() == plain[2]   # (the bias table of the dosage form has the bits of the matrix form's)
    D = pkg.Dosage(lib, ns, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"], nk=nk)
    D.load(0, counts, depths)
    D.finish()
    scan(tabs[0], mine[0] + "d", False, 0.05, D, "scan_dosage")
    scan(tabs[1], mine[1] + "d", True, -1.0, D, "scan_dosage")
    D.close()
    for i in range(2):
        x = read_bytes(o[i] + "d")
        assert x == read_bytes(mine[i] + "d") and x[0].count(b"\n") == 5
    assert read_bytes(o[1] + "d")[1] is None and read_bytes(o[0] + "d")[1] is not None
    # a pair file that names a locus the build does not have is refused with its line, once the build is known
    with open(os.path.join(tmp, "far.tsv"), "w") as f:
        f.write(f"0\tgene0\n{ntr}\tgene1\n")
    r = subprocess.run([PRED, "--assoc", t0, o[0] + "x", "--assoc-pairs", os.path.join(tmp, "far.tsv")] + five, capture_output=True, text=True)
    assert r.returncode == 1 and f"line 2: locus {ntr} >=" in r.stderr and not os.path.exists(o[0] + "x" + EXTS[0])


def test_cohort_assoc_equals_the_pred_tool(tmp_path):
    spec = SETS["g1"]
    gdir = os.path.join(cases.GOLDEN, spec["dir"])
    tmp = str(tmp_path)
    files = make_samples(gdir, tmp)
    ns = len(files)
    depths = [30.5, 0.75, 41.0, 17.25, 3.0, 55.125][:ns]
    ik = os.path.join(tmp, "ikmer.meta")
    meta = golden_ikmer_meta(gdir, ik)
    with open(os.path.join(tmp, "gt.meta.txt"), "w") as f:   # danbing-tk-pred reads the count files that the cohort run writes
        for i, d in enumerate(depths):
            f.write("%s.trkmc.ar\t%r\n" % (os.path.join(tmp, "coh", "c%d" % i), d))
    rng = np.random.default_rng(6)
    sample_of = [5, 0, 2, 3, 1]            # the sample whose reads hit nothing is masked out
    names = ["a", "b", "c"]
    pheno = rng.normal(0, 1, (3, len(sample_of)))
    table = os.path.join(tmp, "pheno.tsv")
    write_table(table, sample_of, pheno, names)
    off = list(range(meta["ntr"] + 1))   # one phenotype per locus
    idx = [l % 3 for l in range(meta["ntr"])]
    pairs = os.path.join(tmp, "pairs.tsv")
    write_pairs(pairs, off, idx, names)

    def groups(tag):
        return ["--assoc", table, os.path.join(tmp, tag + "0"), "--assoc-p", "0.2", "--assoc", table, os.path.join(tmp, tag + "1"), "--assoc-pairs", pairs, "--assoc-raw"]

    os.makedirs(os.path.join(tmp, "coh"))
    os.makedirs(os.path.join(tmp, "ref"))
    rows = lambda d: [(f, os.path.join(tmp, d, "c%d" % i), repr(dp)) for i, (f, dp) in enumerate(zip(files, depths))]  # noqa: E731
    coh = [os.path.join(tmp, "coh." + x) for x in ("raw.gt", "cor.gt", "bias.tsv")]
    ref = [os.path.join(tmp, "ref." + x) for x in ("raw.gt", "cor.gt", "bias.tsv")]
    r = run(spec["flags"] + ["--cohort", manifest(tmp_path / "m.tsv", rows("coh")), "--pred", ik] + coh + groups("c"), cwd=gdir)
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-3000:]
    two = [os.path.join(tmp, "two." + x) for x in ("raw.gt", "cor.gt", "bias.tsv")]
    r = subprocess.run([PRED] + groups("p") + [os.path.join(tmp, "gt.meta.txt"), ik] + two, capture_output=True)
    assert r.returncode == 0, r.stderr
    for i in range(2):
        x = read_bytes(os.path.join(tmp, "c%d" % i))
        assert x == read_bytes(os.path.join(tmp, "p%d" % i)) and x[0].count(b"\n") == 4, i
    assert read_bytes(os.path.join(tmp, "c0"))[1] is not None and read_bytes(os.path.join(tmp, "c1"))[1] is None
    # the pred and count outputs are the bytes of the run without the flags
    r = run(spec["flags"] + ["--cohort", manifest(tmp_path / "mr.tsv", rows("ref")), "--pred", ik] + ref, cwd=gdir)
    assert r.returncode == 0, r.stderr[-3000:]
    for a, b in zip(coh, ref):
        assert open(a, "rb").read() == open(b, "rb").read(), a
    for i in range(ns):
        for ext in (".trkmc.ar", ".tr.summary.txt"):
            assert open(os.path.join(tmp, "coh", "c%d" % i) + ext, "rb").read() == open(os.path.join(tmp, "ref", "c%d" % i) + ext, "rb").read()
    # the model on the matrix the run wrote: the rows, the counts of tests
    cb = open(coh[1], "rb").read()
    cor = np.frombuffer(cb[8:], np.float32).reshape(meta["nk"], ns)
    m = assoc_model.scan(cor, sample_of, pheno, nk_cum=meta["nk_cum"])
    for line, w in zip(open(os.path.join(tmp, "c0") + EXTS[0]).read().split("\n")[1:-1], m["best"]):
        f = line.split("\t")
        assert (int(f[1]), int(f[2])) == (w["n_tests"], w["skipped"]) and w["n_tests"] > 0
    # --dosage
    dd = [os.path.join(tmp, "d." + x) for x in ("dos.tsv", "bias.tsv")]
    r = run(spec["flags"] + ["--cohort", manifest(tmp_path / "md.tsv", rows("nowhere")), "--dosage", ik] + dd + ["--no-trkmc", "--assoc", table, os.path.join(tmp, "cd"), "--assoc-pairs", pairs, "--assoc-p", "0.5"],
            cwd=gdir)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([PRED, "--assoc", table, os.path.join(tmp, "pd"), "--assoc-pairs", pairs, "--assoc-p", "0.5", "--dosage", os.path.join(tmp, "pd.dos.tsv"), os.path.join(tmp, "gt.meta.txt"), ik,
                        os.path.join(tmp, "pd.bias.tsv")], capture_output=True)
    assert r.returncode == 0, r.stderr
    x = read_bytes(os.path.join(tmp, "cd"))
    assert x == read_bytes(os.path.join(tmp, "pd")) and x[0] is not None and x[1] is not None
    assert open(dd[0], "rb").read() == open(os.path.join(tmp, "pd.dos.tsv"), "rb").read()
