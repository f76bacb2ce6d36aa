"""The genotype score on the host (no device): the per-window and per-locus bodies of csrc/dbtk_eval.h in a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer against the model of tests/eval_model.py; dbtk_eval_columns against the model's
doubles and text; what the binding knows of include/dbtk_eval.h; and every refusal of `danbing-tk --eval` at parse time."""
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

import bind
import eval_cases
import eval_model
import sim_cases
import sim_model

pkg, abi = bind.pkg, bind.abi
ROOT = bind.ROOT
EXE = os.path.join(ROOT, "danbing-tk_amd", "bin", "danbing-tk")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("evalcheck") / "eval_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "danbing-tk_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "eval_check.cpp")], check=True)
    return exe


def hand_made_counts(beg, seed):
    """x up to 2^20 and y up to 2^31 (products above 32 bits), zeros in both, an all-zero truth in locus 2; locus 4: one term
    x = 2^31, y = 2^33 (x * y = 2^64); locus 6: five times y = 2^31 (no product overflows, their sum Syy = 5 * 2^62 does)"""
    rng = random.Random(seed)
    nk = beg[-1]
    x = [rng.choice((0, 0, 1, 2, 3, rng.randrange(1 << 20), 1 << 20)) for _ in range(nk)]
    y = [rng.choice((0, 1, rng.randrange(1 << 12), rng.randrange(1 << 24))) for _ in range(nk)]
    for l in range(len(beg) - 1):  # (two counts of 2^31 a locus: Syy stays below 2^64, three more would not)
        for i, v in zip(range(beg[l], beg[l + 1]), ((1 << 31) - 1, 1 << 31)):
            x[i], y[i] = 1 << 20, v
    x[beg[2]:beg[3]] = [0] * (beg[3] - beg[2])
    x[beg[4]], y[beg[4]] = 1 << 31, 1 << 33
    for i in range(5):
        x[beg[6] + i], y[beg[6] + i] = 1, 1 << 31
    return x, y


@pytest.mark.parametrize("k", [21, 20])
def test_kernel_bodies_under_sanitizers(checker, tmp_path, k):
    case = eval_cases.TruthCase(k)
    a = case.arrays
    nloci, nk = eval_cases.NLOCI, len(a["tr_ks"])
    beg = [0] + [int(v) for v in np.cumsum(a["tr_cnt"])]
    fbeg = [0] + [int(v) for v in np.cumsum(a["fl_cnt"])]
    slots = [{int(a["tr_ks"][i]): i for i in range(beg[l], beg[l + 1])} for l in range(nloci)]   # (this program's own counter order: file order)
    flank = [{int(v) for v in a["fl_ks"][fbeg[l]:fbeg[l + 1]]} for l in range(nloci)]
    cls = {}   # (locus, k-mer) -> (class as the class table has it: flank beats TR; the counter of a k-mer in both sets)
    for l in range(nloci):
        for km, s in slots[l].items():
            cls[(l, km)] = (s, -1)
        for km in flank[l]:
            cls[(l, km)] = (-1, slots[l].get(km, -1))
    assert sum(1 for c, b in cls.values() if b >= 0) >= 3   # the case has k-mers in both sets
    ivs = []
    for asm in range(2):
        seqs = {sim_model.name_of(h): s for h, s in case.contigs[asm]}
        ivs += [(l, seqs[c][st:min(en, len(seqs[c]))]) for c, st, en, l in case.beds[asm]]
    assert beg[5] - beg[4] >= 1 and beg[7] - beg[6] >= 5 and beg[12] - beg[11] == 7  # (locus 11 is the pure 7-base repeat)
    x, y = hand_made_counts(beg, seed=k)
    inp = tmp_path / "case.txt"
    inp.write_text(f"{k} {nloci} {nk}\n{len(ivs)}\n" + "".join(f"{l} {s}\n" for l, s in ivs) + f"{len(cls)}\n" + "".join(f"{l} {km} {c} {b}\n" for (l, km), (c, b) in cls.items()) +
                   " ".join(map(str, x)) + "\n" + " ".join(map(str, y)) + "\n" + " ".join(map(str, beg)) + "\n")
    r = subprocess.run([checker, str(inp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    out = r.stdout.split("\n")
    wt, ww = eval_model.truth(case.window_counts(), slots, nk)
    assert sum(wt) > 3000 and sum(ww) > sum(wt) and sum(wt[b] for c, b in cls.values() if b >= 0) > 0
    assert out[0] == "truth " + " ".join(map(str, wt))
    assert out[1] == "windows " + " ".join(map(str, ww))
    want = eval_model.sums(x, y, beg)
    over = [l for l in range(nloci) if not eval_model.fits64(want[l])]
    assert over == [4, 6]
    for l in range(nloci):
        s = want[l]
        line = f"sums {l} overflow" if l in over else "sums %d %d %d %d %d %d %d %d %d" % (l, s["n1"], s["Sx"], s["Sy"], s["Sy1"], s["Sxy"], s["Sxx"], s["Syy"], s["Syy1"])
        assert out[2 + l] == line, l
    assert max(s["Sxy"] for l, s in enumerate(want) if l not in over) > 1 << 40


def f64(v):
    return struct.pack("<d", v)


def test_columns_equal_the_models_doubles_and_text():
    lib = pkg.Dbtk()
    rng = random.Random(11)
    base = dict(nk=9, windows=12, n1=3, Sx=7, Sy=0, Sy1=0, Sxy=0, Sxx=0, Syy=0, Syy1=0)
    cases = [
        dict(base),                                                     # nothing at all
        dict(base, Sxx=13, Sy=40, Syy=900),                             # Sxy == 0 with a truth and counts: every column 0
        dict(base, Sxy=1, Sxx=8, Sy=1, Sy1=1, Syy=4, Syy1=4),           # slope 0.125 (%.2f on a tie), pred 8.0, r2 1/32 = 0.03125 (%.4f on a tie)
        dict(base, Sxy=3, Sxx=8, Sy=3, Sy1=3, Syy=36, Syy1=36),         # slope 0.375 (a tie that rounds up to even 0.38)
        dict(base, Sxy=1001, Sxx=8000, Sy=1, Sy1=1, Syy=4, Syy1=5),     # beside the ties
        dict(base, Sxy=999, Sxx=8000, Sy=1, Sy1=1, Syy=4, Syy1=3),
        dict(base, Sxy=4, Sxx=1, Sy=1, Sy1=3, Syy=32, Syy1=16),         # pred 0.25 (%.1f on a tie: 0.2) and 0.75 (0.8)
        dict(base, Sxy=4, Sxx=1, Sy=5, Sy1=7, Syy=32, Syy1=16),         # pred 1.25, 1.75
        dict(base, Sxy=(1 << 53) + 1, Sxx=(1 << 60) + 3, Sy=(1 << 54) + 1, Sy1=(1 << 54) - 1, Syy=(1 << 63) + 1025, Syy1=(1 << 62) + 511),  # the conversions round
        dict(base, Sxy=(1 << 64) - 1, Sxx=(1 << 64) - 1, Sy=(1 << 64) - 1, Sy1=(1 << 64) - 1, Syy=(1 << 64) - 1, Syy1=(1 << 64) - 1),
    ]
    for _ in range(200):
        b = rng.choice((8, 20, 40, 60, 64))
        v = lambda: rng.randrange(1, 1 << b)
        cases.append(dict(base, Sxy=v(), Sxx=v(), Sy=v(), Sy1=v(), Syy=v(), Syy1=v()))
    got = pkg.eval_columns(lib, cases)
    for s, g in zip(cases, got):
        w = eval_model.columns(s)
        assert [f64(v) for v in g] == [f64(v) for v in w], (s, g, w)
        assert "%.2f\t%.1f\t%.4f\t%.1f\t%.4f" % g == "%.2f\t%.1f\t%.4f\t%.1f\t%.4f" % w
    assert got[1] == (0.0,) * 5 and got[0] == (0.0,) * 5
    assert "%.2f %.4f" % (got[2][0], got[2][2]) == "0.12 0.0312" and "%.2f" % got[3][0] == "0.38" and "%.1f %.1f" % (got[6][1], got[6][3]) == "0.2 0.8"
    assert "%.2f" % got[4][0] == "0.13" and "%.2f" % got[5][0] == "0.12"
    assert eval_model.tsv_text(cases[:3]).count("\n") == 4 and pkg.eval_columns(lib, []) == []


def test_binding_knows_the_entry_points_and_the_pinned_versions_did_not_move():
    hdr = open(os.path.join(ROOT, "include", "dbtk_eval.h")).read()
    assert "#define DBTK_EVAL_API_VERSION 1u" in hdr and abi.EVAL_API_VERSION == 1
    assert abi.ABI_VERSION == 11 and abi.SIM_API_VERSION == 1 and abi.KCP_API_VERSION == 1
    for name, v in (("dbtk.h", "DBTK_ABI_VERSION 11u"), ("dbtk_sim.h", "DBTK_SIM_API_VERSION 1u"), ("dbtk_kcp.h", "DBTK_KCP_API_VERSION 1u")):
        assert re.search(r"#define\s+" + v.replace(" ", r"\s+") + r"\b", open(os.path.join(ROOT, "include", name)).read()), name
    lib = pkg.Dbtk()
    declared = set(re.findall(r"\b(dbtk_eval_\w+)\s*\(", hdr))
    assert declared == set(pkg.EXPORTS_EVAL), declared ^ set(pkg.EXPORTS_EVAL)
    for s in pkg.EXPORTS_EVAL:
        assert hasattr(lib.L, s), s
    for s in ("dbtk_eval_create", "dbtk_eval_truth_sim", "dbtk_eval_truth_set", "dbtk_eval_truth", "dbtk_eval_truth_reset", "dbtk_eval_score_ctx", "dbtk_eval_score_device",
              "dbtk_eval_sums", "dbtk_eval_columns", "dbtk_eval_write", "dbtk_eval_times", "dbtk_eval_free"):
        assert s in pkg.EXPORTS_EVAL
    lib.L.dbtk_eval_api_version.restype = bind.C.c_uint32
    assert lib.L.dbtk_eval_api_version() == 1
    assert hasattr(pkg, "Eval") and pkg.Eval.__init__ is not object.__init__
    for n, ver in (("dbtk_abi_version", 11), ("dbtk_sim_api_version", 1), ("dbtk_kcp_api_version", 1)):
        getattr(lib.L, n).restype = bind.C.c_uint32
        assert getattr(lib.L, n)() == ver


def test_eval_refusals_at_parse_time_and_usage(tmp_path):
    """Status 1 and a message naming the flag, before any device is touched (every device is hidden: a run that got as far as a context
    would fail differently).  The nk of an --eval-truth file is checked once the RPGG is loaded, still before any batch."""
    case = sim_cases.AsmCase(str(tmp_path))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    fa = tmp_path / "r.fa"
    fa.write_text(">a:0-500:0/1\nACGT\n>a:0-500:0/2\nACGT\n")
    man = tmp_path / "m.tsv"
    man.write_text(f"{fa}\t{tmp_path}/s1\n")
    nk = len(case_arrays_tr(case))
    good, short, other = tmp_path / "t.ar", tmp_path / "short.ar", tmp_path / "other.ar"
    good.write_bytes(struct.pack("<Q", nk) + bytes(8 * nk))
    short.write_bytes(struct.pack("<Q", nk) + bytes(8 * nk - 8))
    other.write_bytes(struct.pack("<Q", nk + 1) + bytes(8 * nk + 8))
    head = [EXE, "-k", str(sim_cases.K), "-qs", case.pref, "-cth", str(sim_cases.CTH), "-p", "1", "-ka"]
    out = ["-o", str(tmp_path / "o")]
    sim = ["--sim", case.fa[0], case.bed[0], "--sim-ml", "1"]
    reads = ["-fa", str(fa)]
    ev, truth = ["--eval", str(tmp_path / "e")], ["--eval-truth", str(good)]
    cases = [
        (head + out + reads + ev, "--eval", "needs a truth"),
        (head + out + sim + ev + truth, "--eval", "not from both"),
        (head + out + reads + truth, "--eval-truth", "needs --eval"),
        (head + out + sim + ["--eval-dump-truth", str(tmp_path / "d.ar")], "--eval-dump-truth", "needs --eval"),
        (head + out + reads + ev + truth + ["--eval-dump-truth", str(tmp_path / "d.ar")], "--eval-dump-truth", "needs --sim"),
        (head + ["--cohort", str(man)] + ev + truth, "--eval", "--cohort"),
        (head + out + ["--bait-fps", str(tmp_path / "f"), "--genome", "g0"] + sim + ev, "--eval", "--genome"),
        (head + out + reads + ev + truth + ["-e", "1"], "--eval", "-e"),
        (head + out + reads + ev + truth + ["--gpus", "2"], "--eval", "--gpus > 1"),
        (head + out + reads + ev + truth + ["--ingest-shards", "2"], "--eval", "--ingest-shards"),
        (head + out + reads + ev + truth + ["--parse-only"], "--eval", "--parse-only"),
        (head + out + reads + ev + ["--eval-truth", str(tmp_path / "absent.ar")], "--eval-truth", "cannot open"),
        (head + out + reads + ev + ["--eval-truth", str(other)], "--eval-truth", f"holds {nk + 1} counts, the RPGG has {nk}"),
        (head + out + reads + ev + ["--eval-truth", str(short)], "--eval-truth", "ends before"),
    ]
    for cmd, flag, msg in cases:
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=60)
        assert r.returncode == 1 and flag in r.stderr and msg in r.stderr and r.stdout == "", (cmd[-5:], r.returncode, r.stderr[-400:])
        assert "Buffered reading" not in r.stderr and not os.path.exists(str(tmp_path / "e.pred"))
    usage = subprocess.run([EXE], capture_output=True, text=True).stderr
    assert "--eval <PREF>" in usage and "--eval-truth <FILE>" in usage and "--eval-dump-truth <FILE>" in usage


def case_arrays_tr(case):
    return [line for line in open(case.pref + ".tr.kmers") if line[0] != ">"]
