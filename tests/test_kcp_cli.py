"""`danbing-tk --bait-profile`: what it refuses at parse time (no device needed), and on the GPU the whole chain on a 4-locus RPGG:
profile files == the model over the kam lines of the same run, -ka writes the same files and no kam text, the counts do not move,
and `ktools fps` -> `ktools serialize-bt` makes a bait database that a -b run loads."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bind
import kcp_model
import synth

abi = bind.abi
ROOT = bind.ROOT
EXE = os.path.join(ROOT, "danbing-tk_amd", "bin", "danbing-tk")
KTOOLS = os.path.join(ROOT, "danbing-tk_amd", "bin", "ktools")
K, NLOCI, NPAIRS = 21, 4, 600


def test_bait_profile_refusals_at_parse_time(tmp_path):
    """Status 1 and a message before any device is touched (HIP_VISIBLE_DEVICES hides every device: a run that got as far as a
    context would fail differently)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    pref = str(tmp_path / "pan")
    synth.write_rpgg_files(synth.build_rpgg_arrays(synth.make_loci(nloci=2, nhap=1, flank=100, seed=3), K), pref)
    fa = tmp_path / "r.fa"
    fa.write_text(">0.a/1\nACGT\n>0.a/2\nACGT\n")
    man = tmp_path / "m.tsv"
    man.write_text(f"{fa}\t{tmp_path}/s1\n")
    base = [EXE, "-k", str(K), "-qs", pref, "-fa", str(fa), "-o", str(tmp_path / "o"), "-p", "1"]
    prof = ["--bait-profile", str(tmp_path / "pf")]
    cases = [
        (base + prof, "needs -s 1 or -s 2"),
        (base + prof + ["-s", "3"], "needs -s 1 or -s 2"),
        (base + ["-s", "1", "--tp-only"], "--tp-only needs --bait-profile"),
        (base + prof + ["-s", "1", "-e", "1"], "cannot be combined with -e"),
        (base + prof + ["-s", "1", "--gpus", "2"], "--gpus > 1"),
        (base + prof + ["-s", "2", "--ingest-shards", "2"], "--ingest-shards"),
        (base + ["-s", "1", "-g", "80"] + prof, "-g/-gc/-gcc"),
        ([EXE, "-k", str(K), "-qs", pref, "-ka", "-p", "1", "-s", "1", "--cohort", str(man)] + prof, "cannot be combined with --cohort"),
    ]
    for cmd, msg in cases:
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=60)
        assert r.returncode == 1 and "--bait-profile" in r.stderr and msg in r.stderr and r.stdout == "", (cmd[-4:], r.returncode, r.stderr[-300:])
    assert not any(f.name.startswith("pf.") for f in tmp_path.iterdir())
    assert "--bait-profile <PREF>" in subprocess.run([EXE], capture_output=True, text=True).stderr


def test_create_without_a_device_is_no_device(tmp_path):
    code = ("import sys; sys.path.insert(0, %r); import bind; pkg = bind.pkg\n"
            "try:\n    pkg.Kcp(pkg.Dbtk(), 21, 4)\nexcept pkg.DbtkError as e:\n    print(e.status)\n") % os.path.join(ROOT, "tests")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120, cwd=ROOT)
    assert r.stdout.strip() == str(abi.ERR_NO_DEVICE), r.stdout + r.stderr


# ---- the 4-locus case: reads titled >LOCUS.rP for -s 1, every fifth pair titled with the next locus
class Case:
    def __init__(self, d):
        self.dir = d
        self.loci = synth.make_loci(nloci=NLOCI, nhap=2, flank=300, seed=41)
        os.makedirs(os.path.join(d, "g"), exist_ok=True)
        self.pref = os.path.join(d, "g", "pan")
        synth.write_rpgg_files(synth.build_rpgg_arrays(self.loci, K), self.pref)
        reads = synth.sim_reads(self.loci, npairs=NPAIRS, seed=42, sub=0.01, nrate=0.001, lower=0.02)
        self.src = []
        for p, t in enumerate(reads.titles):
            l = int(t.split(":l")[1].split("h")[0])
            self.src.append((l + 1) % NLOCI if p % 5 == 0 else l)
            reads.titles[p] = f"{self.src[-1]}.r{p}"
        self.reads = reads
        self.fa = os.path.join(d, "reads.fa")
        synth.write_fasta(reads, self.fa)

    def run(self, out, *flags, ok=True):
        r = subprocess.run([EXE, "-s", "1", "-k", str(K), "-qs", self.pref, "-fa", self.fa, "-o", os.path.join(self.dir, out), "-p", "1", *flags], capture_output=True,
                           text=True, timeout=300)
        assert (r.returncode == 0) == ok, r.stderr[-2000:]
        return r

    def files(self, out):
        return tuple(open(os.path.join(self.dir, out + ext), "rb").read() for ext in (".trkmc.ar", ".tr.summary.txt"))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return Case(str(tmp_path_factory.mktemp("kcpcli")))


def test_the_oracle_assigns_pairs_of_both_classes(case):
    """On the CPU, before any GPU run: the reads give true and false positives whatever the device does."""
    oracle = bind.Oracle()
    go = oracle.load(case.pref, K)
    seq, off = case.reads.packed()
    o = oracle.align(go, abi.default_params(ksize=K, cthreshold=10, simmode=1), seq, off)
    dst = {r.pair: r.dst for r in o["recs"][:NPAIRS] if r.stage in (abi.STAGE_ASGN, abi.STAGE_COUNTED)}
    tp = sum(1 for p, d in dst.items() if d < NLOCI and d == case.src[p])
    fp = sum(1 for p, d in dst.items() if d < NLOCI and d != case.src[p])
    assert tp > 100 and fp > 20, (tp, fp)


@pytest.fixture(scope="module")
def runs(case):
    plain = case.run("plain")
    prof = case.run("prof", "--bait-profile", os.path.join(case.dir, "pf"))
    ka = case.run("ka", "-ka", "--bait-profile", os.path.join(case.dir, "pfka"))
    return plain, prof, ka


@pytest.mark.gpu
def test_profile_files_equal_the_model_over_the_kam_lines_of_the_same_run(case, runs):
    plain, prof, _ = runs
    assert prof.stdout == plain.stdout and prof.stdout.count("\n") > 300, "stdout is what it was"
    tab = kcp_model.from_kam(prof.stdout.split("\n"), K, NLOCI)
    tp, fp = open(os.path.join(case.dir, "pf.TP_pf.txt")).read(), open(os.path.join(case.dir, "pf.FP_pf.txt")).read()
    assert len(tp) > 10000 and len(fp) > 1000, "both files hold entries"
    assert tp == kcp_model.profile_text(tab, 0)
    assert fp == kcp_model.profile_text(tab, 1)
    assert "writing k-mer count profiles" in prof.stderr


@pytest.mark.gpu
def test_ka_writes_the_same_profiles_and_no_kam_text_and_the_counts_do_not_move(case, runs):
    plain, prof, ka = runs
    assert ka.stdout == ""
    for ext in (".TP_pf.txt", ".FP_pf.txt"):
        assert open(os.path.join(case.dir, "pfka" + ext), "rb").read() == open(os.path.join(case.dir, "pf" + ext), "rb").read()
    assert case.files("plain") == case.files("prof") == case.files("ka")
    assert len(case.files("plain")[0]) > 0


@pytest.mark.gpu
def test_tp_only_then_fps_then_serialize_bt_then_a_run_with_the_bait_database(case, runs):
    tpo = case.run("tpo", "-ka", "--tp-only", "--bait-profile", os.path.join(case.dir, "pftp"))
    assert tpo.stdout == "" and not os.path.exists(os.path.join(case.dir, "pftp.FP_pf.txt"))
    assert open(os.path.join(case.dir, "pftp.TP_pf.txt"), "rb").read() == open(os.path.join(case.dir, "pf.TP_pf.txt"), "rb").read()
    fps = os.path.join(case.dir, "fps.txt")
    r = subprocess.run([KTOOLS, "fps", str(NLOCI), str(K), fps, os.path.join(case.dir, "pf.FP_pf.txt"), os.path.join(case.dir, "pf.TP_pf.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    kept, _ = kcp_model.parse_profile(open(fps).read())
    nkept = sum(len(v) for v in kept.values())
    assert nkept > 0
    r = subprocess.run([KTOOLS, "serialize-bt", fps, str(NLOCI), os.path.join(case.dir, "made")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    bt = os.path.join(case.dir, "made.bt.kmdb")
    a = np.fromfile(bt, np.uint64, count=2 + NLOCI)
    assert int(a[0]) == NLOCI and int(a[1 + NLOCI]) == nkept
    withb = case.run("withb", "-ka", "-b", bt)
    assert "reads removed by bait locus" in withb.stderr and len(case.files("withb")[0]) == len(case.files("plain")[0])
