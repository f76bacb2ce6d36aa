"""The permutation p-values of the association scan on the host (no device): dbtk_assoc_perm_generate through ctypes against the model's
generator, the host header csrc/dbtk_assoc_perm_host.h in a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer,
what the binding knows of include/dbtk_assoc_perm.h, the refusals of `--assoc-perm` / `--assoc-seed` at parse time in both command lines,
the kernel's shape constants against the cases of tests/test_assoc_perm_gpu.py, and the margins that make the exact comparisons of those
cases honest."""
import os
import re
import subprocess

import numpy as np
import pytest

import assoc_perm_model as pm
import bind
import cases as golden_cases
from test_assoc_host import EXE, NO_GPU, PRED, kernel_constants, write_inputs

pkg, abi = bind.pkg, bind.abi
ROOT = bind.ROOT


@pytest.mark.parametrize("n,B", [(1, 3), (2, 5), (3, 7), (64, 3), (1100, 2)])
def test_generator_equals_the_model_byte_for_byte(n, B):
    lib = pkg.Dbtk()
    seen = []
    for seed in (0, 1, 2 ** 64 - 1):
        got = pkg.assoc_perm_generate(lib, n, B, seed)
        assert got.dtype == np.uint32 and got.shape == (B, n) and got.tobytes() == pm.generate(n, B, seed).tobytes()
        assert all(pm.is_permutation(row, n) for row in got)
        longer = pkg.assoc_perm_generate(lib, n, B + 4, seed)
        assert longer[:B].tobytes() == got.tobytes()                  # the first B' rows of a B-run are the B'-run
        seen.append(got.tobytes())
    assert n < 3 or len(set(seen)) == 3                               # different seeds differ
    assert pkg.assoc_perm_generate(lib, n, 0, 1).shape == (0, n)


def test_perm_host_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "assoc_perm_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "danbing-tk_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "assoc_perm_host_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout[-2000:] + r.stderr[-3000:]


def test_binding_knows_the_permutation_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dbtk_assoc_perm.h")).read()
    assert "#define DBTK_ASSOC_PERM_API_VERSION 1u" in hdr and abi.ASSOC_PERM_API_VERSION == 1
    assert re.search(r"#define\s+DBTK_ASSOC_PERM_MAX\s+1000000u", hdr) and abi.ASSOC_PERM_MAX == 1000000 == pm.PERM_MAX
    declared = set(re.findall(r"\b(dbtk_assoc_perm_\w+)\s*\(", hdr))
    assert declared == set(pkg.EXPORTS_ASSOC_PERM), declared ^ set(pkg.EXPORTS_ASSOC_PERM)
    lib = pkg.Dbtk()
    for s in pkg.EXPORTS_ASSOC_PERM:
        assert hasattr(lib.L, s), s
        assert s not in pkg.EXPORTS and s not in pkg.EXPORTS_ASSOC and s not in pkg.EXPORTS_ASSOC_COVAR
    lib.L.dbtk_assoc_perm_api_version.restype = bind.C.c_uint32
    assert lib.L.dbtk_assoc_perm_api_version() == 1
    assert bind.C.sizeof(abi.AssocPermResult) == 48
    for name in ("set_permutations", "permutations", "perm_scan_device", "perm_scan_pred", "perm_scan_dosage", "perm_results", "perm_stats", "perm_write"):
        assert callable(getattr(pkg.Assoc, name)), name
    assert callable(pkg.assoc_perm_generate)
    # the headers beside it did not move
    assert "#define DBTK_ASSOC_API_VERSION 1u" in open(os.path.join(ROOT, "include", "dbtk_assoc.h")).read() and abi.ASSOC_API_VERSION == 1
    assert "#define DBTK_ASSOC_COVAR_API_VERSION 1u" in open(os.path.join(ROOT, "include", "dbtk_assoc_covar.h")).read() and abi.ASSOC_COVAR_API_VERSION == 1
    assert abi.ABI_VERSION == 11 and bind.C.sizeof(abi.AssocBest) == 72 and bind.C.sizeof(abi.AssocHit) == 40
    assert not re.search(r"dbtk_assoc_perm_\w+\s*\(", open(os.path.join(ROOT, "include", "dbtk_assoc.h")).read())
    host = open(os.path.join(ROOT, "danbing-tk_amd", "csrc", "dbtk_assoc_perm_host.h")).read()
    assert re.search(r"PERM_MAX\s*=\s*1000000;", host)
    for word in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", ">> 64"):
        assert word in hdr, word                                       # the header states the generator word for word


def test_assoc_perm_refusals_at_parse_time(tmp_path):
    """Status 1 and a message that names the flag, before any device is touched (every device is hidden) and before INPUT1 or INPUT2 is
    opened, through danbing-tk-pred and through danbing-tk --cohort --pred."""
    ph, meta = write_inputs(tmp_path)
    out = str(tmp_path / "o")
    cases = [
        (["--assoc-perm", "9", "--assoc", ph, out], "--assoc-perm", "needs --assoc"),
        (["--assoc", ph, out, "--assoc-perm", "9", "--assoc-p", "0.1", "--assoc-perm", "9"], "--assoc-perm", "given twice"),
        (["--assoc", ph, out, "--assoc-perm", "0"], "--assoc-perm", "not an integer in 1 .. 1000000"),
        (["--assoc", ph, out, "--assoc-perm", "1000001"], "--assoc-perm", "not an integer in 1 .. 1000000"),
        (["--assoc", ph, out, "--assoc-perm", "1e3"], "--assoc-perm", "not an integer in 1 .. 1000000"),
        (["--assoc", ph, out, "--assoc-perm", "-4"], "--assoc-perm", "not an integer in 1 .. 1000000"),
        (["--assoc", ph, out, "--assoc-perm", "2.5"], "--assoc-perm", "not an integer in 1 .. 1000000"),
        (["--assoc", ph, out, "--assoc-seed", "5"], "--assoc-seed", "needs --assoc-perm"),
        (["--assoc", ph, out, "--assoc-perm", "9", "--assoc", ph, out + "2", "--assoc-seed", "5"], "--assoc-seed", "needs --assoc-perm"),
        (["--assoc-seed", "5", "--assoc", ph, out, "--assoc-perm", "9"], "--assoc-seed", "needs --assoc"),
        (["--assoc", ph, out, "--assoc-perm", "9", "--assoc-seed", "18446744073709551616"], "--assoc-seed", "not an unsigned 64-bit integer"),
        (["--assoc", ph, out, "--assoc-perm", "9", "--assoc-seed", "-1"], "--assoc-seed", "not an unsigned 64-bit integer"),
        (["--assoc", ph, out, "--assoc-perm", "9", "--assoc-seed", "x"], "--assoc-seed", "not an unsigned 64-bit integer"),
        (["--assoc", ph, str(tmp_path / "nodir" / "o"), "--assoc-perm", "9"], "--assoc", "cannot create"),
    ]
    files5 = [meta, str(tmp_path / "ik.meta"), str(tmp_path / "raw.gt"), str(tmp_path / "cor.gt"), str(tmp_path / "bias.tsv")]
    open(files5[1], "w").close()                # (danbing-tk --pred looks for IKMER.META first)
    fa = tmp_path / "r.fa"
    fa.write_text(">a/1\nACGT\n>a/2\nACGT\n")
    man = tmp_path / "m.tsv"
    man.write_text(f"{fa}\t{tmp_path}/s1\t30\n")
    gdir = os.path.join(golden_cases.GOLDEN, "g1_k21")
    head = [EXE, "-k", "21", "-qs", "pan", "-kf", "4", "1", "-cth", "45", "-ka", "--cohort", str(man), "--pred"] + files5[1:]
    for args, flag, msg in cases:
        for cmd, cwd in (([PRED] + args + files5, None), (head + args, gdir)):
            r = subprocess.run(cmd, capture_output=True, text=True, env=NO_GPU, timeout=60, cwd=cwd)
            assert r.returncode == 1 and flag in r.stderr and msg in r.stderr and r.stdout == "", (cmd, r.returncode, r.stderr[-400:], r.stdout[-200:])
            assert not os.path.exists(out + ".assoc.best.tsv") and not os.path.exists(out + ".assoc.perm.tsv")
    # --window-rows stays refused as for --assoc
    r = subprocess.run([PRED, "--assoc", ph, out, "--assoc-perm", "9", "--window-rows", "8"] + files5, capture_output=True, text=True, env=NO_GPU, timeout=60)
    assert r.returncode == 1 and "a window holds a part of the rows" in r.stderr
    # a value is missing behind the flag
    for flag, front in (("--assoc-perm", []), ("--assoc-seed", ["--assoc-perm", "3"])):
        r = subprocess.run([PRED, "--assoc", ph, out] + front + [flag], capture_output=True, text=True, env=NO_GPU, timeout=60)
        assert r.returncode == 1 and f"{flag}: expected" in r.stderr
    # good flags pass the parse-time checks (the largest seed and the largest B too): the run then fails for want of its inputs
    r = subprocess.run([PRED, "--assoc", ph, out, "--assoc-perm", "1000000", "--assoc-seed", "18446744073709551615", "--assoc", ph, out + "2", "--assoc-perm", "1", meta,
                        str(tmp_path / "no_ik.meta")] + files5[2:], capture_output=True, text=True, env=NO_GPU, timeout=60)
    assert r.returncode != 0 and "--assoc-perm" not in r.stderr and "--assoc-seed" not in r.stderr and "cannot open" in r.stderr
    for exe in (PRED, EXE):
        usage = subprocess.run([exe], capture_output=True, text=True).stderr
        assert "[--assoc-perm <B> [--assoc-seed <S>]]" in usage and "--assoc <PHENO.tsv> <OUTPREF>" in usage


def perm_constants():
    src = open(os.path.join(ROOT, "danbing-tk_amd", "csrc", "dbtk_assoc_perm_dev.h")).read()
    return {name: int(v) for name, v in re.findall(r"constexpr\s+uint32_t\s+(PM_\w+)\s*=\s*(\d+);", src)}


def test_gpu_cases_cross_the_permutation_constants():
    """Columns per chunk (a phenotype's B + 1 columns: one chunk short, full, one over, many), the register-resident limit on n, the rows
    of a pass and of a work item, read from the source; the cases of tests/test_assoc_perm_gpu.py lie on both sides of each.  The table
    of permutations is uint32 at every n: there is no uint16 form and so no boundary to cross."""
    import test_assoc_gpu as base
    import test_assoc_perm_gpu as g

    c, pc = kernel_constants(), perm_constants()
    assert pc["PM_CHUNK"] == g.CHUNK == c["AS_CHUNK"] == 8 and pc["PM_BUF"] == 2
    ch, seg = pc["PM_CHUNK"], c["AS_SEG"]
    Bs = {B for _, _, B, _ in g.MODEL_CASES}
    assert Bs == {1, ch - 1, ch, ch + 1, 65}
    assert any(B + 1 < ch for B in Bs) and ch - 1 in Bs and ch in Bs and any(B + 1 > 2 * ch and (B + 1) % ch for B in Bs)   # B + 1 columns: short, exact, one over, many with a rest
    ns = [n for n, _, _, _ in g.MODEL_CASES]
    assert {(n, nsamp) for n, nsamp, _, _ in g.MODEL_CASES} == {(3, 9), (64, 70), (65, 70), (512, 520), (513, 520), (1100, 1111)}
    assert seg in ns and seg + 1 in ns and any(n > 2 * seg for n in ns) and any(n < 64 for n in ns) and 64 in ns and 65 in ns
    assert {(n, nsamp, q) for n, nsamp, q, _, _ in g.COVAR_CASES} == {(12, 20, 9), (65, 70, 8), (513, 520, 128), (1100, 1111, 9)}
    sizes = set(base.LOCUS_ROWS)   # the matrix is test_assoc_gpu's: loci under and over a pass and a work item
    assert {0, 1, c["AS_TILE"] - 1, c["AS_TILE"], c["AS_TILE"] + 1} <= sizes and any(c["AS_ROWS"] < v <= c["AS_ITEM_ROWS"] for v in sizes) and any(v > c["AS_ITEM_ROWS"] for v in sizes)
    assert sum(base.LOCUS_ROWS) + base.TRAILING > c["AS_ITEM_ROWS"] and g.ALL_ROWS_CASE[0] <= seg   # without a pair list: a second work item
    assert g.NOISE == 4 and max(base.LOCUS_PHENOS) + g.NOISE > ch                                   # a locus whose phenotypes pass a chunk's count


def test_the_inputs_keep_their_margins_without_a_gpu():
    """For every case of tests/test_assoc_perm_gpu.py that is built without a device the model asserts (assoc_perm_model.assert_margins,
    inside model_of) that every |T_b - T_0| is exactly 0 with y o pi_b byte-equal to y, or at least 1000 times the bound: the seeds are
    good wherever the suite runs.  (The two cohort cases take their matrices from the device; the GPU test asserts the same of them
    before it compares.)"""
    import test_assoc_perm_gpu as g

    lib = pkg.Dbtk()
    for n, ns, B, seed in g.MODEL_CASES:
        c = g.plain_case(n, ns, seed)
        g.model_of(c, pm.generate(n, B, seed), c["pairs"])
    for n, ns, q, B, seed in g.COVAR_CASES:
        c = g.covariate_case(n, ns, q, seed)
        order = np.argsort(c["sample_of"], kind="stable")
        g.model_of(c, pm.generate(n, B, seed), c["pairs"], Q=pkg.assoc_covar_basis(lib, c["covar"][:, order]))
    n, ns, B, seed = g.ALL_ROWS_CASE
    g.model_of(g.hand_made(n, ns, seed=300 + 7 * seed + n), pm.generate(n, B, seed), None)
    n, ns, B, seed = g.ORACLE_CASE
    c = g.plain_case(n, ns, seed)
    g.model_of(c, pm.generate(n, B, seed), c["pairs"])
    c, n, ns, swap = g.tie_case()
    T, _, _, _ = g.model_of(c, np.tile(np.arange(n, dtype=np.uint32), (5, 1)), c["pairs"])
    assert (T[:, 1:] == T[:, :1]).all()
    T, _, _, _ = g.model_of(c, np.vstack([pm.generate(n, 3, 11), swap[None, :]]), c["pairs"])
    assert T[g.NPHENO, 4] == T[g.NPHENO, 0] and T[g.NPHENO + 1, 4] != T[g.NPHENO + 1, 0]
    n, ns, B, seed = 65, 70, 7, 1   # test_perm_refusals_and_the_file compares n_ge through the file
    c = g.plain_case(n, ns, seed)
    g.model_of(c, pm.generate(n, B, seed), c["pairs"])
