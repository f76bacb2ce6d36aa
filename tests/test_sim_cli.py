"""`danbing-tk --sim ASSEMBLY BED`: what it refuses at parse time (no device needed), and on the GPU a two-haplotype assembly over a
4-locus RPGG: every output of the run equals, byte for byte, that of `-s 2 -fa` over the annotated FASTA the reference's workflow
(sim_reads | bedtools map | awk) would have written for the same assemblies — kam text, counts, profiles, and a -b run with the bait
database made from those profiles."""
import os
import subprocess

import pytest

import bind
import sim_cases

abi = bind.abi
ROOT = bind.ROOT
EXE = os.path.join(ROOT, "danbing-tk_amd", "bin", "danbing-tk")
KTOOLS = os.path.join(ROOT, "danbing-tk_amd", "bin", "ktools")
K, NLOCI, CTH = sim_cases.K, sim_cases.NLOCI, sim_cases.CTH


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return sim_cases.AsmCase(str(tmp_path_factory.mktemp("simcli")))


def test_sim_refusals_at_parse_time_and_usage(case, tmp_path):
    """Status 1 and a message naming --sim before any device is touched (HIP_VISIBLE_DEVICES hides every device: a run that got as
    far as a context would fail differently)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    fa = tmp_path / "r.fa"
    fa.write_text(">a:0-500:0/1\nACGT\n>a:0-500:0/2\nACGT\n")
    man = tmp_path / "m.tsv"
    man.write_text(f"{fa}\t{tmp_path}/s1\n")
    head = [EXE, "-k", str(K), "-qs", case.pref, "-cth", str(CTH), "-p", "1"]
    out = ["-o", str(tmp_path / "o")]
    sim = ["--sim", case.fa[0], case.bed[0], "--sim-ml", "1"]
    cases = [
        (head + out + sim + ["-fa", str(fa)], "-fa/-fq"),
        (head + out + ["-fq", str(fa)] + sim, "-fa/-fq"),
        (head + out + sim + ["-s", "1"], "-s 1"),
        (head + out + sim + ["-e", "1"], "-e"),
        (head + out + sim + ["-a"], "-a/-ae"),
        (head + out + sim + ["-ae"], "-a/-ae"),
        (head + out + ["-g", "80"] + sim, "-g/-gc/-gcc"),
        (head + out + ["-gc", "80", "3"] + sim, "-g/-gc/-gcc"),
        (head + out + ["-gcc", "80"] + sim, "-g/-gc/-gcc"),
        (head + out + sim + ["-tb"], "-tb"),
        (head + out + sim + ["-bu"], "-bu"),
        (head + ["-ka", "--cohort", str(man)] + sim, "--cohort"),
        (head + out + sim + ["--gpus", "2"], "--gpus > 1"),
        (head + out + sim + ["--ingest-shards", "2"], "--ingest-shards"),
        (head + out + ["-fa", str(fa), "--sim-fs", "400"], "--sim-fs needs --sim"),
        (head + out + ["-fa", str(fa), "--sim-rlen", "100"], "--sim-rlen needs --sim"),
        (head + out + ["-fa", str(fa), "--sim-c", "10"], "--sim-c needs --sim"),
        (head + out + ["-fa", str(fa), "--sim-ml", "10"], "--sim-ml needs --sim"),
        (head + out + sim + ["--sim-rlen", "500"], "--sim-rlen 500"),                 # RLEN >= FLEN
        (head + out + sim + ["--sim-fs", "150"], "--sim-fs 150"),
        (head + out + sim + ["--sim-fs", "600", "--sim-rlen", "257"], "--sim-rlen 257"),  # RLEN > DBTK_MAX_READ_LEN
        (head + out + sim + ["--sim-c", "0"], "--sim-c"),
        (head + out + sim + ["--sim-c", "301"], "--sim-c"),                           # cv > 2 * RLEN: the step would be 0
        (head + out + sim + ["--sim-rlen", "64"], "-cth + -k - 1 = 65"),             # the reader would drop every pair
        (head + out + ["--sim", str(tmp_path / "absent.fa"), case.bed[0]], "cannot open"),
        (head + out + ["--sim", case.fa[0], str(tmp_path / "absent.bed")], "cannot open"),
    ]
    for cmd, msg in cases:
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=60)
        assert r.returncode == 1 and "--sim" in r.stderr and msg in r.stderr and r.stdout == "", (cmd[-4:], r.returncode, r.stderr[-300:])
    assert "use baitDB" not in r.stderr  # (the refusals come before anything is loaded)
    usage = subprocess.run([EXE], capture_output=True, text=True).stderr
    assert "--sim <FASTA> <BED>" in usage and "--sim-fs <INT> [500]" in usage and "--sim-rlen <INT> [150]" in usage and "--sim-c <INT> [15]" in usage and \
        "--sim-ml <INT> [50000]" in usage


def test_the_oracle_assigns_pairs_of_both_classes(case):
    """On the CPU, before any GPU run, for this seed: true positives, false positives, false positives without a source ('.') and
    fragments under two labels — a case without them would let the comparisons below pass empty."""
    oracle = bind.Oracle()
    go = oracle.load(case.pref, K)
    seq, off, src, labels = case.batch()
    npairs = len(src)
    o = oracle.align(go, abi.default_params(ksize=K, cthreshold=CTH, simmode=2), seq, off)
    dst = {r.pair: r.dst for r in o["recs"][:npairs] if r.stage in (abi.STAGE_ASGN, abi.STAGE_COUNTED)}
    tp = sum(1 for p, d in dst.items() if d < NLOCI and d == src[p])
    fp = sum(1 for p, d in dst.items() if d < NLOCI and d != src[p])
    fp_dot = sum(1 for p, d in dst.items() if d < NLOCI and src[p] == NLOCI)
    two = sum(1 for l in labels if len(l) >= 2)
    print(f"pairs {npairs}, tp {tp}, fp {fp}, '.'-sourced fp {fp_dot}, two-label fragments {two}")
    assert tp >= 40 and fp >= 10 and fp_dot >= 5 and two >= 20, (npairs, tp, fp, fp_dot, two)


class Runs:
    def __init__(self, case):
        self.case = case
        self.annot = case.annotated_fasta(os.path.join(case.dir, "annot.fa"))

    def run(self, out, how, *flags):
        c = self.case
        src = ["-s", "2", "-fa", self.annot] if how == "fa" else ["--sim", c.fa[0], c.bed[0], "--sim", c.fa[1], c.bed[1], "--sim-ml", "1"]
        env = dict(os.environ, DBTK_SIM_BATCH_PAIRS="97")
        r = subprocess.run([EXE, "-k", str(K), "-qs", c.pref, "-o", os.path.join(c.dir, out), "-cth", str(CTH), "-p", "1", *src, *flags], capture_output=True, text=True,
                           timeout=300, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        return r

    def read(self, name):
        return open(os.path.join(self.case.dir, name), "rb").read()

    def same(self, a, b, exts):
        for ext in exts:
            x, y = self.read(a + ext), self.read(b + ext)
            assert x == y and len(x) > 0, (a, b, ext, len(x), len(y))


@pytest.fixture(scope="module")
def runs(case):
    return Runs(case)


COUNTS = (".trkmc.ar", ".tr.summary.txt")
PROFILES = (".TP_pf.txt", ".FP_pf.txt")


@pytest.mark.gpu
def test_sim_equals_the_fa_run_over_the_annotated_fasta(runs):
    d = runs.case.dir
    fa = runs.run("fa", "fa", "--bait-profile", os.path.join(d, "pf_fa"))
    sim = runs.run("sim", "sim", "--bait-profile", os.path.join(d, "pf_sim"))
    assert sim.stdout == fa.stdout and sim.stdout.count("\n") > 50
    assert any("," in line.split("\t")[-5] for line in sim.stdout.split("\n") if line), "a kam line of a fragment under two labels"
    runs.same("fa", "sim", COUNTS)
    runs.same("pf_fa", "pf_sim", PROFILES)
    assert "k_sim_tile wrote" in sim.stderr and "reads processed in total" in sim.stderr
    tot = [l for l in fa.stderr.split("\n") if "reads processed in total" in l or "reads assigned to TR region" in l]
    assert tot == [l for l in sim.stderr.split("\n") if "reads processed in total" in l or "reads assigned to TR region" in l] and len(tot) == 2


@pytest.mark.gpu
def test_ka_writes_the_same_files_and_no_kam_text(runs):
    d = runs.case.dir
    if not os.path.exists(os.path.join(d, "pf_fa.TP_pf.txt")):
        runs.run("fa", "fa", "--bait-profile", os.path.join(d, "pf_fa"))
    ka = runs.run("simka", "sim", "-ka", "--bait-profile", os.path.join(d, "pf_simka"))
    assert ka.stdout == ""
    runs.same("fa", "simka", COUNTS)
    runs.same("pf_fa", "pf_simka", PROFILES)
    # without records at all (-ka alone): the asynchronous path, batch i + 1 tiled while batch i is aligned
    plain = runs.run("simplain", "sim", "-ka")
    assert plain.stdout == ""
    runs.same("fa", "simplain", COUNTS)


@pytest.mark.gpu
def test_tp_only_and_a_run_with_the_bait_database_made_from_the_profiles(runs):
    d = runs.case.dir
    if not os.path.exists(os.path.join(d, "pf_fa.TP_pf.txt")):
        runs.run("fa", "fa", "--bait-profile", os.path.join(d, "pf_fa"))
    tpo = runs.run("simtp", "sim", "-ka", "--tp-only", "--bait-profile", os.path.join(d, "pf_simtp"))
    assert tpo.stdout == "" and not os.path.exists(os.path.join(d, "pf_simtp.FP_pf.txt"))
    assert runs.read("pf_simtp.TP_pf.txt") == runs.read("pf_fa.TP_pf.txt")
    sim = runs.run("simp", "sim", "-ka", "--bait-profile", os.path.join(d, "pf_simp"))
    fps = os.path.join(d, "fps.txt")
    r = subprocess.run([KTOOLS, "fps", str(NLOCI), str(K), fps, os.path.join(d, "pf_simp.FP_pf.txt"), os.path.join(d, "pf_simp.TP_pf.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([KTOOLS, "serialize-bt", fps, str(NLOCI), os.path.join(d, "made")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    bt = os.path.join(d, "made.bt.kmdb")
    fab = runs.run("fab", "fa", "-b", bt)
    simb = runs.run("simb", "sim", "-b", bt)
    assert simb.stdout == fab.stdout and len(simb.stdout) > 0
    runs.same("fab", "simb", COUNTS)
    bl = [l for l in fab.stderr.split("\n") if "reads removed by bait locus" in l]
    assert bl == [l for l in simb.stderr.split("\n") if "reads removed by bait locus" in l] and len(bl) == 1
    assert sim.stdout == ""
