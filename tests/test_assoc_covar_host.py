"""The covariates of the association scan on the host (no device): dbtk_assoc_covar_basis through ctypes, the host header
csrc/dbtk_assoc_covar_host.h in a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer, the refusals of
`--assoc-covar` at parse time in both command lines, what the binding knows of include/dbtk_assoc_covar.h, and the kernel's shape
constants against the cases of tests/test_assoc_covar_gpu.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import assoc_covar_model as cm
import bind
import cases as golden_cases
from test_assoc_host import EXE, NO_GPU, PRED, kernel_constants, write_inputs

pkg, abi = bind.pkg, bind.abi
ROOT = bind.ROOT
U = 2.0 ** -53


def covariates(n, q, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4, (q, n)).astype(np.float64) + rng.normal(0, 0.5, (q, n)) + 10.0 * rng.normal(0, 1, (q, 1))


@pytest.mark.parametrize("n,q", [(4, 1), (40, 1), (40, 5), (40, 12), (300, 60), (131, 128)])
def test_basis_through_the_binding(n, q):
    """max |Q'Q - I| <= 8 q u (formed in extended precision, so that the bound is on Q and not on the check), every column orthogonal to
    the intercept (a column's entries are rounded to float64: |sum Q_i| <= u sum |Q_i| <= u sqrt(n), asserted with the factor 8 again),
    the columns span the centred covariates, and a second call gives the same bytes."""
    lib = pkg.Dbtk()
    c = covariates(n, q, seed=n + q)
    Q = pkg.assoc_covar_basis(lib, c)
    assert Q.shape == (q, n) and Q.dtype == np.float64
    Ql = Q.astype(np.longdouble)
    assert float(np.abs(Ql @ Ql.T - np.eye(q, dtype=np.longdouble)).max()) <= 8 * q * U
    assert float(np.abs(Ql.sum(axis=1)).max()) <= 8 * U * np.sqrt(n)
    centred = c - c.mean(axis=1, keepdims=True)
    coef, *_ = np.linalg.lstsq(Q.T, centred.T, rcond=None)
    left = np.linalg.norm(centred.T - Q.T @ coef, axis=0)
    assert (left <= 1e-12 * np.linalg.norm(centred, axis=1)).all()
    assert np.abs(np.triu(coef, 0) - coef).max() <= 1e-12 * np.abs(coef).max()     # column j needs Q_0 .. Q_j only: file order
    assert pkg.assoc_covar_basis(lib, c).tobytes() == Q.tobytes()
    own = cm.basis(c)                                                               # the model's QR spans the same space
    assert np.abs(np.abs(np.sum(own * Q, axis=1)) - 1.0).max() <= 1e-10


def test_basis_refusals_name_the_column():
    lib = pkg.Dbtk()
    n = 30
    c = covariates(n, 5, seed=1)
    bad = {
        "constant": (np.vstack([c[:2], np.full(n, 0.1), c[2:]]), 2),
        "twice": (np.vstack([c, c[1]]), 5),
        "sum": (np.vstack([c[:4], c[0] + c[3] - 2.0, c[4:]]), 4),
        "nan": (np.where(np.arange(5 * n).reshape(5, n) == 3 * n + 7, np.nan, c), 3),
        "inf": (np.where(np.arange(5 * n).reshape(5, n) == 0, np.inf, c), 0),
    }
    for name, (cv, col) in bad.items():
        with pytest.raises(pkg.DbtkError) as e:
            pkg.assoc_covar_basis(lib, cv)
        assert e.value.status == abi.ERR_ARG and e.value.bad_column == col and f"column {col}" in str(e.value), (name, str(e.value))
        assert ("not finite" in str(e.value)) == (name in ("nan", "inf"))
    # the threshold is a share of the centred squared norm: 1e-7 of it left is refused, 1e-5 passes
    for eps, ok in ((10 ** -3.5, False), (10 ** -2.5, True)):
        e0 = c[1] - c[1].mean()
        e0 -= (e0 @ (c[0] - c[0].mean())) / ((c[0] - c[0].mean()) @ (c[0] - c[0].mean())) * (c[0] - c[0].mean())
        v = c[0] - c[0].mean()
        near = np.vstack([c[0], 3.0 * v + eps * e0 * np.linalg.norm(3.0 * v) / np.linalg.norm(e0)])
        if ok:
            pkg.assoc_covar_basis(lib, near)
        else:
            with pytest.raises(pkg.DbtkError) as e:
                pkg.assoc_covar_basis(lib, near)
            assert e.value.bad_column == 1


def test_covar_host_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "assoc_covar_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "danbing-tk_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "assoc_covar_host_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout[-2000:] + r.stderr[-3000:]


def test_binding_knows_the_covariate_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dbtk_assoc_covar.h")).read()
    assert "#define DBTK_ASSOC_COVAR_API_VERSION 1u" in hdr and abi.ASSOC_COVAR_API_VERSION == 1
    assert re.search(r"#define\s+DBTK_ASSOC_COVAR_MAX\s+128u", hdr) and abi.ASSOC_COVAR_MAX == 128
    assert re.search(r"#define\s+DBTK_ASSOC_COVAR_COLLINEAR\s+1e-6\b", hdr) and abi.ASSOC_COVAR_COLLINEAR == 1e-6
    assert cm.COLLINEAR == abi.ASSOC_COVAR_COLLINEAR and cm.COVAR_MAX == abi.ASSOC_COVAR_MAX
    declared = set(re.findall(r"\b(dbtk_assoc_covar_\w+)\s*\(", hdr))
    assert declared == set(pkg.EXPORTS_ASSOC_COVAR), declared ^ set(pkg.EXPORTS_ASSOC_COVAR)
    lib = pkg.Dbtk()
    for s in pkg.EXPORTS_ASSOC_COVAR:
        assert hasattr(lib.L, s), s
        assert s not in pkg.EXPORTS and s not in pkg.EXPORTS_ASSOC
    lib.L.dbtk_assoc_covar_api_version.restype = bind.C.c_uint32
    assert lib.L.dbtk_assoc_covar_api_version() == 1
    assert callable(pkg.Assoc.set_covariates) and callable(pkg.Assoc.covariates) and callable(pkg.assoc_covar_basis)
    # the scan's own header did not move
    assert "#define DBTK_ASSOC_API_VERSION 1u" in open(os.path.join(ROOT, "include", "dbtk_assoc.h")).read() and abi.ASSOC_API_VERSION == 1 and abi.ABI_VERSION == 11
    host = open(os.path.join(ROOT, "danbing-tk_amd", "csrc", "dbtk_assoc_covar_host.h")).read()
    assert re.search(r"COVAR_MAX\s*=\s*128;", host) and re.search(r"COVAR_COLLINEAR\s*=\s*1e-6;", host)


def table(fn, samples, cols, names=None):
    names = names or [f"c{j}" for j in range(len(cols))]
    with open(fn, "w") as f:
        f.write("id\t" + "\t".join(names) + "\n")
        for i, s in enumerate(samples):
            f.write(f"{s}\t" + "\t".join(str(c[i]) for c in cols) + "\n")
    return str(fn)


def test_assoc_covar_refusals_at_parse_time(tmp_path):
    """Status 1 and a message that names the flag and, for text, the line, before any device is touched (every device is hidden) and before
    INPUT1 or INPUT2 is opened, through danbing-tk-pred and through danbing-tk --cohort --pred."""
    ph, meta = write_inputs(tmp_path)           # 2 phenotypes over the samples 0 .. 4
    s5 = list(range(5))
    good = table(tmp_path / "good.tsv", s5, [[1, 0, 1, 0, 0]], ["sex"])
    bad = {
        "na": ("id\tsex\n0\t1\n1\tNA\n2\t0\n3\t0\n4\t1\n", "line 3: phenotype sex: \"NA\""),
        "empty": ("id\tsex\n0\t1\n1\t\n2\t0\n3\t0\n4\t1\n", "line 3: phenotype sex: \"\""),
        "word": ("id\tsex\n0\t1\n1\t0\n2\t0\n3\tmale\n4\t1\n", "line 5: phenotype sex: \"male\""),
        "stranger": ("id\tsex\n0\t1\n1\t0\n2\t0\n3\t1\n4\t1\n9\t0\n", "sample 9 is not listed in the phenotype table"),
        "missing": ("id\tsex\n0\t1\n1\t0\n2\t0\n4\t1\n", "sample 3 of the phenotype table is missing"),
        "few": ("id\ta\tb\tc\n0\t1\t5\t2\n1\t0\t3\t2\n2\t0\t4\t7\n3\t1\t1\t1\n4\t1\t2\t0\n", "5 samples and 3 covariates"),
        "constant": ("id\tsex\tbatch\n0\t1\t0.1\n1\t0\t0.1\n2\t0\t0.1\n3\t1\t0.1\n4\t1\t0.1\n", "covariate batch is constant or collinear"),
        "collinear": ("id\tpc1\tpc2\n0\t1\t3\n1\t0\t1\n2\t0.5\t2\n3\t4\t9\n4\t2\t5\n", "covariate pc2 is constant or collinear"),
    }
    files = {}
    for name, (text, _) in bad.items():
        files[name] = str(tmp_path / f"{name}.tsv")
        open(files[name], "w").write(text)
    rng = np.random.default_rng(1)
    s140 = list(range(140))
    ph140 = table(tmp_path / "ph140.tsv", s140, [rng.normal(0, 1, 140)], ["g0"])
    wide = table(tmp_path / "wide.tsv", s140, list(rng.normal(0, 1, (129, 140))))
    out = str(tmp_path / "o")
    absent = str(tmp_path / "absent.tsv")
    cases = [
        (["--assoc-covar", good, "--assoc", ph, out], "needs --assoc"),
        (["--assoc", ph, out, "--assoc-covar", good, "--assoc-p", "0.1", "--assoc-covar", good], "given twice"),
        (["--assoc", ph, out, "--assoc-covar", absent], "cannot open"),
        (["--assoc", ph140, out, "--assoc-covar", wide], "holds 129 covariates: at most 128"),
    ] + [(["--assoc", ph, out, "--assoc-covar", files[name]], msg) for name, (_, msg) in bad.items()]
    files5 = [meta, str(tmp_path / "ik.meta"), str(tmp_path / "raw.gt"), str(tmp_path / "cor.gt"), str(tmp_path / "bias.tsv")]
    open(files5[1], "w").close()                # (danbing-tk --pred looks for IKMER.META first)
    fa = tmp_path / "r.fa"
    fa.write_text(">a/1\nACGT\n>a/2\nACGT\n")
    man = tmp_path / "m.tsv"
    man.write_text(f"{fa}\t{tmp_path}/s1\t30\n")
    gdir = os.path.join(golden_cases.GOLDEN, "g1_k21")
    head = [EXE, "-k", "21", "-qs", "pan", "-kf", "4", "1", "-cth", "45", "-ka", "--cohort", str(man), "--pred"] + files5[1:]
    for args, msg in cases:
        for cmd, cwd in (([PRED] + args + files5, None), (head + args, gdir)):
            r = subprocess.run(cmd, capture_output=True, text=True, env=NO_GPU, timeout=60, cwd=cwd)
            assert r.returncode == 1 and "--assoc-covar" in r.stderr and msg in r.stderr and r.stdout == "", (cmd, r.returncode, r.stderr[-400:], r.stdout[-200:])
            assert not os.path.exists(out + ".assoc.best.tsv")
    # a file name is missing behind the flag
    r = subprocess.run([PRED, "--assoc", ph, out, "--assoc-covar"], capture_output=True, text=True, env=NO_GPU, timeout=60)
    assert r.returncode == 1 and "--assoc-covar: expected COVAR.tsv" in r.stderr
    # a good covariate file passes the parse-time checks, also in a second group with its own file: the run then fails for want of its inputs
    r = subprocess.run([PRED, "--assoc", ph, out, "--assoc-covar", good, "--assoc", ph, out + "2", "--assoc-covar", good, meta, str(tmp_path / "no_ik.meta")] + files5[2:], capture_output=True, text=True, env=NO_GPU,
                       timeout=60)
    assert r.returncode != 0 and "--assoc-covar" not in r.stderr and "cannot open" in r.stderr
    for exe in (PRED, EXE):
        usage = subprocess.run([exe], capture_output=True, text=True).stderr
        assert "[--assoc-covar <COVAR.tsv>]" in usage and "--assoc <PHENO.tsv> <OUTPREF>" in usage


def test_gpu_cases_cross_the_covariate_constants():
    """The covariate chunk (= the phenotype chunk), the cap and the register-resident limit on n, read from the kernel's source: the cases
    of tests/test_assoc_covar_gpu.py must lie on both sides of each."""
    import test_assoc_covar_gpu as g

    c = kernel_constants()
    assert c["AS_CHUNK"] == 8 and c["AS_COVAR_MAX"] == 128 == abi.ASSOC_COVAR_MAX and c["AS_SEG"] == 512
    assert c["AS_ROWS"] * c["AS_COVAR_MAX"] * 8 == 32 * 1024                         # the a_j of a pass in LDS
    ch, cap, seg = c["AS_CHUNK"], c["AS_COVAR_MAX"], c["AS_SEG"]
    qs = {q for _, _, q, _ in g.CASES}
    ns = {n for n, _, _, _ in g.CASES}
    assert any(q < ch for q in qs) and ch in qs and ch + 1 in qs and any(q > 2 * ch and q % ch for q in qs) and cap in qs and max(qs) == cap
    assert seg in ns and seg + 1 in ns and any(n > 2 * seg for n in ns) and any(n < 64 for n in ns)
    assert any(n - 2 - q == 1 for n, _, q, _ in g.CASES)                              # one degree of freedom
    assert all(nsamp > n >= q + 3 for n, nsamp, q, _ in g.CASES)
    assert {(n, nsamp, q) for n, nsamp, q, _ in g.CASES} == {(12, 20, 9), (65, 70, 1), (65, 70, 8), (512, 520, 17), (513, 520, 128), (1100, 1111, 9)}
