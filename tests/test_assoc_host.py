"""The association scan on the host (no device): dbtk_assoc_pvalue and dbtk_assoc_bh through ctypes against recorded scipy results, the
host header csrc/dbtk_assoc_host.h in a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer, what the binding
knows of include/dbtk_assoc.h, the refusals of `--assoc` at parse time in both command lines, and the kernel's shape constants against
the cases of tests/test_assoc_gpu.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import assoc_model
import bind
import cases as golden_cases

pkg, abi = bind.pkg, bind.abi
ROOT = bind.ROOT
PRED = os.path.join(ROOT, "danbing-tk_amd", "bin", "danbing-tk-pred")
EXE = os.path.join(ROOT, "danbing-tk_amd", "bin", "danbing-tk")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
SMALLEST_NORMAL = 2.2250738585072014e-308


def golden():
    rows = []
    for line in open(os.path.join(ROOT, "tests", "golden", "assoc_pvalues.tsv")):
        if line[0] != "#":
            n, r, p = line.split("\t")
            rows.append((int(n), float(r), float(p)))
    return rows


def test_pvalue_against_the_recorded_t_tails():
    """tests/golden/assoc_pvalues.tsv: 2 * scipy.stats.t.sf (scipy 1.15.3) on n = 3, 4, 10, 100, 879, 4000 and |r| from 1e-6 to
    1 - 1e-12, both signs; p goes down to 1.6e-318 and to 0.  Measured where the file was made: the largest relative deviation of
    dbtk_assoc_pvalue from scipy on that grid is 2.2e-13 (scipy itself is 8.2e-14 from a 60-digit mpmath betainc there).  Asserted:
    ten times that, 2.2e-12, the margin being for libm differences between machines.  Below the normal range of float64 a relative
    bound means nothing (1.6e-318 has 20 bits): there the bound is relative to the smallest normal number."""
    lib = pkg.Dbtk()
    rows = golden()
    assert sorted({n for n, _, _ in rows}) == [3, 4, 10, 100, 879, 4000]
    assert min(abs(r) for _, r, _ in rows) == 1e-6 and max(abs(r) for _, r, _ in rows) == 1 - 1e-12
    assert 0 < min(p for _, _, p in rows if p > 0) < 1e-300 and any(p == 0 for _, _, p in rows)
    worst = 0.0
    for n, r, p in rows:
        got = pkg.assoc_pvalue(lib, r, n)
        dev = abs(got - p) / max(p, SMALLEST_NORMAL)
        worst = max(worst, dev)
        assert dev <= 2.2e-12, (n, r, p, got)
    print(f"largest relative deviation from the recorded values: {worst:.3e}")
    for r, n in ((1.0, 3), (-1.0, 100)):
        assert pkg.assoc_pvalue(lib, r, n) == 0.0
    for r, n in ((0.5, 2), (1.0000001, 10), (float("nan"), 10)):
        with pytest.raises(pkg.DbtkError) as e:
            pkg.assoc_pvalue(lib, r, n)
        assert e.value.status == abi.ERR_ARG


def test_bh_and_r2_threshold_through_the_binding():
    lib = pkg.Dbtk()
    rng = np.random.default_rng(3)
    for m in (0, 1, 2, 9, 500):
        p = rng.uniform(0, 1, m) ** 4 * 3  # (some above 1, as p_bonf may be)
        if m > 2:
            p[0] = p[1]
        got = pkg.assoc_bh(lib, p)
        assert got.tobytes() == assoc_model.bh(p).tobytes()
    for n in (3, 10, 130, 879):
        for pt in (0.9, 0.05, 1e-6):
            r2 = pkg.assoc_r2_threshold(lib, pt, n)
            assert pkg.assoc_pvalue(lib, np.sqrt(r2), n) <= pt < pkg.assoc_pvalue(lib, np.sqrt(r2 * (1 - 1e-9)), n)
    assert pkg.assoc_r2_threshold(lib, 1.0, 10) == 0.0 and pkg.assoc_r2_threshold(lib, 0.0, 10) == 1.0


def test_host_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "assoc_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "danbing-tk_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "assoc_host_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout[-2000:] + r.stderr[-3000:]


def test_binding_knows_the_entry_points_and_the_pinned_versions_did_not_move():
    hdr = open(os.path.join(ROOT, "include", "dbtk_assoc.h")).read()
    assert "#define DBTK_ASSOC_API_VERSION 1u" in hdr and abi.ASSOC_API_VERSION == 1
    assert abi.ABI_VERSION == 11 and abi.EVAL_API_VERSION == 1 and abi.SIM_API_VERSION == 1 and abi.KCP_API_VERSION == 1
    lib = pkg.Dbtk()
    declared = set(re.findall(r"\b(dbtk_assoc_\w+)\s*\(", hdr))
    assert declared == set(pkg.EXPORTS_ASSOC), declared ^ set(pkg.EXPORTS_ASSOC)
    for s in pkg.EXPORTS_ASSOC:
        assert hasattr(lib.L, s), s
        assert s not in pkg.EXPORTS
    lib.L.dbtk_assoc_api_version.restype = bind.C.c_uint32
    assert lib.L.dbtk_assoc_api_version() == 1
    assert hasattr(pkg, "Assoc") and pkg.Assoc.__init__ is not object.__init__
    assert bind.C.sizeof(abi.AssocBest) == 72 and bind.C.sizeof(abi.AssocHit) == 40
    assert abi.ASSOC_ALL_PAIRS_MAX == 64 and re.search(r"#define\s+DBTK_ASSOC_ALL_PAIRS_MAX\s+64u", hdr)


def write_inputs(tmp_path, P=2, n=5):
    ph = tmp_path / "pheno.tsv"
    ph.write_text("id\t" + "\t".join(f"g{i}" for i in range(P)) + "\n" + "".join(f"{s}\t" + "\t".join(str((s * 7 + i * 3) % 11) for i in range(P)) + "\n" for s in range(n)))
    meta = tmp_path / "gt.meta"
    meta.write_text("".join(f"{tmp_path}/s{s}.trkmc.ar\t30.0\n" for s in range(n)))
    return str(ph), str(meta)


def test_assoc_refusals_at_parse_time(tmp_path):
    """Status 1 and a message that names the flag and, for the two text files, the line, before any device is touched (every device is
    hidden: a run that got as far as a handle would fail differently) and before INPUT1 or INPUT2 is opened."""
    ph, meta = write_inputs(tmp_path)
    files5 = [meta, str(tmp_path / "ik.meta"), str(tmp_path / "raw.gt"), str(tmp_path / "cor.gt"), str(tmp_path / "bias.tsv")]
    dos = ["--dosage", str(tmp_path / "d.tsv")]
    files3 = [meta, str(tmp_path / "ik.meta"), str(tmp_path / "bias.tsv")]
    out = str(tmp_path / "o")
    bad = {}
    for name, text in (("na", "id\tg0\n0\t1\n1\tNA\n2\t3\n"), ("empty", "id\tg0\n0\t1\n1\t\n2\t3\n"), ("word", "id\tg0\n0\t1\n1\t2\n2\tx3\n"), ("dup", "id\tg0\n0\t1\n1\t2\n0\t3\n"),
                       ("two", "id\tg0\n0\t1\n1\t2\n"), ("wide", "id\t" + "\t".join(f"g{i}" for i in range(65)) + "\n" + "".join(f"{s}\t" + "\t".join(str(s * i % 5) for i in range(65)) + "\n" for s in range(4)))):
        bad[name] = str(tmp_path / f"{name}.tsv")
        open(bad[name], "w").write(text)
    pairs_unknown, pairs_form, pairs_ok = str(tmp_path / "pu.tsv"), str(tmp_path / "pf.tsv"), str(tmp_path / "pk.tsv")
    open(pairs_unknown, "w").write("0\tg0\n1\tg7\n")
    open(pairs_form, "w").write("0\tg0\n\n1\n")
    open(pairs_ok, "w").write("0\tg0\n0\tg0\n")
    cases = [
        (["--assoc", ph], "--assoc", "expected PHENO.tsv OUTPREF"),
        (["--assoc-p", "0.1", "--assoc", ph, out] + files5, "--assoc-p", "needs --assoc"),
        (["--assoc", ph, out, "--assoc-p", "1.5"] + files5, "--assoc-p", "not a p-value"),
        (["--assoc", ph, out, "--assoc-p", "x"] + files5, "--assoc-p", "not a p-value"),
        (["--assoc", str(tmp_path / "absent.tsv"), out] + files5, "--assoc", "cannot open"),
        (["--assoc", bad["na"], out] + files5, "--assoc", "line 3: phenotype g0: \"NA\""),
        (["--assoc", bad["empty"], out] + files5, "--assoc", "line 3: phenotype g0: \"\""),
        (["--assoc", bad["word"], out] + files5, "--assoc", "line 4: phenotype g0: \"x3\""),
        (["--assoc", bad["dup"], out] + files5, "--assoc", "line 4: sample 0 is given twice"),
        (["--assoc", bad["two"], out] + files5, "--assoc", "lists 2 samples"),
        (["--assoc", bad["wide"], out] + files5, "--assoc", "holds 65 phenotypes"),
        (["--assoc", ph, out, "--assoc-pairs", pairs_unknown] + files5, "--assoc-pairs", "line 2: unknown phenotype g7"),
        (["--assoc", ph, out, "--assoc-pairs", pairs_form] + files5, "--assoc-pairs", "line 3: expected LOCUS"),
        (["--assoc", ph, out, "--assoc-pairs", str(tmp_path / "absent.tsv")] + files5, "--assoc-pairs", "cannot open"),
        (["--assoc", ph, str(tmp_path / "nodir" / "o")] + files5, "--assoc", "cannot create"),
        (["--assoc", ph, out, "--window-rows", "8"] + files5, "--assoc", "a window holds a part of the rows"),
        (["--window-bytes", "4096", "--assoc", ph, out] + files5, "--assoc", "a window holds a part of the rows"),
        (dos + ["--assoc", ph, out, "--assoc-raw"] + files3, "--assoc-raw", "dosage"),
    ]
    for args, flag, msg in cases:
        r = subprocess.run([PRED] + args, capture_output=True, text=True, env=NO_GPU, timeout=60)
        assert r.returncode == 1 and flag in r.stderr and msg in r.stderr and r.stdout == "", (args, r.returncode, r.stderr[-400:], r.stdout[-200:])
        assert not os.path.exists(out + ".assoc.best.tsv")
    # 65 phenotypes WITH a pair list pass the parse-time checks: the run then fails for want of its input files, not for the table
    r = subprocess.run([PRED, "--assoc", bad["wide"], out, "--assoc-pairs", pairs_ok] + files5, capture_output=True, text=True, env=NO_GPU, timeout=60)
    assert r.returncode != 0 and "phenotypes" not in r.stderr and "cannot open" in r.stderr
    usage = subprocess.run([PRED], capture_output=True, text=True).stderr
    assert "--assoc <PHENO.tsv> <OUTPREF>" in usage and "--assoc-pairs" in usage and "--assoc-raw" in usage
    # danbing-tk: outside --cohort, and in --cohort without --pred / --dosage
    fa = tmp_path / "r.fa"
    fa.write_text(">a/1\nACGT\n>a/2\nACGT\n")
    man = tmp_path / "m.tsv"
    man.write_text(f"{fa}\t{tmp_path}/s1\t30\n")
    gdir = os.path.join(golden_cases.GOLDEN, "g1_k21")   # (an RPGG that exists: its files are looked for before the flags are weighed)
    head = [EXE, "-k", "21", "-qs", "pan", "-kf", "4", "1", "-cth", "45", "-ka"]
    open(files5[1], "w").close()  # (--pred and --dosage look for IKMER.META first)
    for args, msg in ((["-o", str(tmp_path / "x"), "-fa", str(fa), "--assoc", ph, out], "--assoc needs --cohort"),
                      (["--cohort", str(man), "--assoc", ph, out], "--assoc needs --pred or --dosage"),
                      (["--cohort", str(man), "--kms", str(tmp_path / "k.kms"), "--assoc", ph, out], "--assoc needs --pred or --dosage"),
                      (["--cohort", str(man), "--dosage", files5[1], str(tmp_path / "d.tsv"), str(tmp_path / "b.tsv"), "--assoc", ph, out, "--assoc-raw"], "--assoc-raw"),
                      (["--cohort", str(man), "--pred"] + files5[1:] + ["--assoc", bad["na"], out], "line 3: phenotype g0"),
                      (["--cohort", str(man), "--pred"] + files5[1:] + ["--assoc", bad["wide"], out], "holds 65 phenotypes")):
        r = subprocess.run(head + args, capture_output=True, text=True, env=NO_GPU, timeout=60, cwd=gdir)
        assert r.returncode == 1 and msg in r.stderr and r.stdout == "", (args, r.returncode, r.stderr[-400:])
    assert "--assoc <PHENO.tsv> <OUTPREF>" in subprocess.run([EXE], capture_output=True, text=True).stderr


def kernel_constants():
    src = open(os.path.join(ROOT, "danbing-tk_amd", "csrc", "dbtk_assoc.hip")).read()
    env = {}
    for name, expr in re.findall(r"constexpr\s+uint(?:32|64)_t\s+(AS_\w+)\s*=\s*([^;]+);", src):
        env[name] = eval(re.sub(r"(\d+)ull\b", r"\1", expr), {}, dict(env))
    return env


def test_gpu_cases_cross_every_shape_constant():
    """The row tile, the phenotype chunk, the registers-resident limit on n (= the LDS segment), the rows of a workgroup's pass and of a
    work item and the hit-buffer default, read from the kernel's source; the cases of tests/test_assoc_gpu.py must lie on both sides."""
    import test_assoc_gpu as g

    c = kernel_constants()
    assert c["AS_TILE"] == 4 and c["AS_CHUNK"] == 8 and c["AS_SEG"] == 512 and c["AS_ROWS"] == 32 and c["AS_ITEM_ROWS"] == 256 and c["AS_HITS_DEFAULT"] == 1 << 20
    t, ch, seg = c["AS_TILE"], c["AS_CHUNK"], c["AS_SEG"]
    sizes = set(g.LOCUS_ROWS)
    assert {0, 1, t - 1, t, t + 1} <= sizes and any(v > c["AS_ROWS"] for v in sizes) and any(v > c["AS_ITEM_ROWS"] for v in sizes)
    assert 0 in g.LOCUS_PHENOS and ch + 1 in g.LOCUS_PHENOS and any(0 < v < ch for v in g.LOCUS_PHENOS)
    ns_of = dict(g.MASKS)
    assert {3, 63, 64, 65, 130} <= set(ns_of) and all(ns > n for n, ns in g.MASKS) and max(ns_of.values()) <= 4131
    assert seg in ns_of and seg + 1 in ns_of and any(n > 2 * seg for n in ns_of)   # the last resident n, the first that is not, a third segment
    assert g.HITS_SMALL < c["AS_HITS_DEFAULT"] and g.HITS_SMALL & (g.HITS_SMALL - 1) == 0
