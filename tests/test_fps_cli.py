"""`danbing-tk --bait-fps OUT [--genome NAME ...]`: what it refuses at parse time (no device needed), and on the GPU, byte for byte, the
file `ktools fps` makes from the profile text of --bait-profile runs over the same assemblies — one genome (the two-haplotype case
of the --sim tests) and three genomes with entries of all three fates."""
import os
import re
import subprocess

import numpy as np
import pytest

import bind
import kcp_model
import sim_cases
import synth

ROOT = bind.ROOT
EXE = os.path.join(ROOT, "danbing-tk_amd", "bin", "danbing-tk")
KTOOLS = os.path.join(ROOT, "danbing-tk_amd", "bin", "ktools")
K, NLOCI, CTH = sim_cases.K, sim_cases.NLOCI, sim_cases.CTH
COUNTS = (".trkmc.ar", ".tr.summary.txt")


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return sim_cases.AsmCase(str(tmp_path_factory.mktemp("fpscli")))


def test_refusals_at_parse_time_and_usage(case, tmp_path):
    """Status 1 and a message naming the flag before any device is touched (HIP_VISIBLE_DEVICES hides every device: a run that got as
    far as a context would fail differently)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    fa = tmp_path / "r.fa"
    fa.write_text(">0.a/1\nACGT\n>0.a/2\nACGT\n")
    man = tmp_path / "m.tsv"
    man.write_text(f"{fa}\t{tmp_path}/s1\n")
    out = str(tmp_path / "fps.txt")
    head = [EXE, "-k", str(K), "-qs", case.pref, "-cth", str(CTH), "-p", "1"]
    o = ["-o", str(tmp_path / "o")]
    reads = ["-fa", str(fa)]
    fps = ["--bait-fps", out]
    s0, s1 = ["--sim", case.fa[0], case.bed[0]], ["--sim", case.fa[1], case.bed[1]]
    cases = [
        (head + o + reads + fps, "--bait-fps needs -s 1 or -s 2"),
        (head + o + reads + fps + ["-s", "3"], "--bait-fps needs -s 1 or -s 2"),
        (head + o + reads + fps + ["-s", "1", "--tp-only"], "--bait-fps cannot be combined with --tp-only"),
        (head + o + reads + fps + ["-s", "1", "--tp-only", "--bait-profile", str(tmp_path / "pf")], "--bait-fps cannot be combined with --tp-only"),
        (head + o + reads + fps + ["-s", "1", "-e", "1"], "--bait-fps cannot be combined with -e"),
        (head + o + reads + fps + ["-s", "1", "--gpus", "2"], "--gpus > 1"),
        (head + o + reads + fps + ["-s", "2", "--ingest-shards", "2"], "--bait-fps cannot be combined with --ingest-shards"),
        (head + o + reads + ["-s", "1", "-g", "80"] + fps, "-g/-gc/-gcc"),
        (head + ["-ka", "-s", "1", "--cohort", str(man)] + fps, "--bait-fps cannot be combined with --cohort"),
        (head + o + ["--genome", "X"] + s0, "--genome needs --bait-fps"),
        (head + o + reads + ["-s", "1", "--genome", "X"] + fps, "--genome needs --sim"),
        (head + o + fps + s0 + ["--genome", "X"] + s1, "the first --sim stands before the first --genome"),
        (head + o + fps + ["--genome", "X", "--genome", "Y"] + s0, "--genome X has no --sim"),
        (head + o + fps + ["--genome", "X"] + s0 + ["--genome", "Y"], "--genome Y has no --sim"),
        (head + o + fps + ["--genome", "X"] + s0 + ["--bait-profile", str(tmp_path / "pf")], "--genome cannot be combined with --bait-profile"),
        (head + o + fps + ["--genome", "X"] + s0 + ["--gpus", "2"], "--gpus > 1"),
    ]
    for cmd, msg in cases:
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=60)
        assert r.returncode == 1 and msg in r.stderr and r.stdout == "", (cmd[-5:], r.returncode, r.stderr[-300:])
        assert "use baitDB" not in r.stderr and "total number of loci" not in r.stderr  # (before anything is loaded)
    assert not os.path.exists(out) and not any(f.name.startswith("pf.") for f in tmp_path.iterdir())
    usage = subprocess.run([EXE], capture_output=True, text=True).stderr
    assert "--bait-fps <OUT>" in usage and "--genome <NAME>" in usage


class Runs:
    def __init__(self, case):
        self.case = case
        self.d = case.dir

    def path(self, name):
        return os.path.join(self.d, name)

    def run(self, out, *flags):
        env = dict(os.environ, DBTK_SIM_BATCH_PAIRS="97")
        r = subprocess.run([EXE, "-k", str(K), "-qs", self.case.pref, "-o", self.path(out), "-cth", str(CTH), "-p", "1", *flags], capture_output=True,
                           text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        return r

    def ktools_fps(self, out, fp, *tps):
        r = subprocess.run([KTOOLS, "fps", str(NLOCI), str(K), self.path(out), self.path(fp)] + [self.path(t) for t in tps], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        return open(self.path(out), "rb").read()

    def read(self, name):
        return open(self.path(name), "rb").read()

    def same_counts(self, a, b):
        for ext in COUNTS:
            x, y = self.read(a + ext), self.read(b + ext)
            assert x == y and len(x) > 0, (a, b, ext, len(x), len(y))


@pytest.fixture(scope="module")
def runs(case):
    return Runs(case)


def sim_of(case, h):
    return ["--sim", case.fa[h], case.bed[h], "--sim-ml", "1"]


@pytest.mark.gpu
def test_one_genome_equals_ktools_fps_over_the_profiles_of_the_same_run(case, runs):
    both = sim_of(case, 0) + sim_of(case, 1)
    plain = runs.run("one_plain", *both)
    prof = runs.run("one_prof", *both, "--bait-fps", runs.path("one_a.fps"), "--bait-profile", runs.path("one_pf"))
    want = runs.ktools_fps("one_ref.fps", "one_pf.FP_pf.txt", "one_pf.TP_pf.txt")
    kept, order = kcp_model.parse_profile(want.decode())
    assert len(order) >= 2 and sum(len(v) for v in kept.values()) > 0, "the file holds loci and survivors"
    assert runs.read("one_a.fps") == want
    alone = runs.run("one_alone", *both, "--bait-fps", runs.path("one_b.fps"))
    assert runs.read("one_b.fps") == want and not os.path.exists(runs.path("one_b.fps.TP_pf.txt"))
    assert prof.stdout == plain.stdout == alone.stdout and plain.stdout.count("\n") > 50, "the kam text is what it was"
    ka = runs.run("one_ka", *both, "-ka", "--bait-fps", runs.path("one_c.fps"))
    assert ka.stdout == "" and runs.read("one_c.fps") == want
    # ... and from a file of reads: -s 2 over the annotated FASTA of the same assemblies, the profile fed from host buffers
    fa = runs.run("one_fa", "-s", "2", "-fa", case.annotated_fasta(runs.path("annot.fa")), "--bait-fps", runs.path("one_d.fps"))
    assert runs.read("one_d.fps") == want and fa.stdout == plain.stdout
    for name in ("one_prof", "one_alone", "one_ka", "one_fa"):
        runs.same_counts("one_plain", name)
    assert "writing FP-specific bait k-mers" in alone.stderr and "writing k-mer count profiles" not in alone.stderr and "writing k-mer count profiles" in prof.stderr


def genome_x(case):
    """Every locus' haplotype-0 allele with its TR six times over, between 400-base random spacers (seed 7), each labelled with the
    next locus: its pairs are false positives of the loci they are assigned to, with counts per read unlike the haplotypes'."""
    rng = np.random.default_rng(7)
    fl = case.loci.flank
    parts, bed, pos = [], [], 0
    for l in range(NLOCI):
        parts.append(synth.BASES[rng.integers(0, 4, 400)])
        pos += 400
        s = case.loci.haps[0][l]
        x = np.concatenate([s[:fl]] + [s[fl:len(s) - fl]] * 6 + [s[len(s) - fl:]])
        bed.append(("asmx", pos + fl, pos + len(x) - fl, (l + 1) % NLOCI))
        parts.append(x)
        pos += len(x)
    parts.append(synth.BASES[rng.integers(0, 4, 400)])
    fa, bd = os.path.join(case.dir, "asmx.fa"), os.path.join(case.dir, "asmx.bed")
    with open(fa, "w") as f:
        f.write(">asmx\n" + np.concatenate(parts).tobytes().decode() + "\n")
    with open(bd, "w") as f:
        f.write("".join(f"{c}\t{s}\t{e}\t{l}\n" for c, s, e, l in bed))
    return ["--sim", fa, bd, "--sim-ml", "1"]


@pytest.mark.gpu
def test_three_genomes_equal_ktools_fps_over_three_profile_runs(case, runs):
    """X in both classes, then hap0 and hap1 as under --tp-only.  The reference side — three --bait-profile runs and `ktools fps` —
    is looked at first: dropped, kept as 255 0 and widened entries, at least 20 of each, and a locus whose header stands alone."""
    x, h0, h1 = genome_x(case), sim_of(case, 0), sim_of(case, 1)
    runs.run("g_x", *x, "-ka", "--bait-profile", runs.path("g_px"))
    runs.run("g_h0", *h0, "-ka", "--tp-only", "--bait-profile", runs.path("g_p0"))
    runs.run("g_h1", *h1, "-ka", "--tp-only", "--bait-profile", runs.path("g_p1"))
    want = runs.ktools_fps("g_ref.fps", "g_px.FP_pf.txt", "g_px.TP_pf.txt", "g_p0.TP_pf.txt", "g_p1.TP_pf.txt")
    fp, _ = kcp_model.parse_profile(runs.read("g_px.FP_pf.txt").decode())
    kept, order = kcp_model.parse_profile(want.decode())
    nfp, nkept = sum(len(v) for v in fp.values()), sum(len(v) for v in kept.values())
    plain = sum(1 for v in kept.values() for line in v if line.endswith("\t255\t0"))
    print(f"FP entries {nfp}: dropped {nfp - nkept}, kept as 255 0 {plain}, widened {nkept - plain}; header-only loci {[l for l in order if not kept[l]]}")
    assert nfp - nkept >= 20 and plain >= 20 and nkept - plain >= 20, (nfp, nkept, plain)
    assert order == sorted(fp) and any(not kept[l] for l in order), "a locus all of whose candidates died keeps its header"

    names = ["--genome", "X"] + x + ["--genome", "H0"] + h0 + ["--genome", "H1"] + h1
    plain_run = runs.run("g_plain", *x, *h0, *h1)
    g = runs.run("g_fps", *names, "--bait-fps", runs.path("g.fps"))
    assert runs.read("g.fps") == want
    assert g.stdout == plain_run.stdout and g.stdout.count("\n") > 50
    runs.same_counts("g_plain", "g_fps")
    tot = [l for l in plain_run.stderr.split("\n") if "reads processed in total" in l or "reads assigned to TR region" in l]
    assert tot == [l for l in g.stderr.split("\n") if "reads processed in total" in l or "reads assigned to TR region" in l] and len(tot) == 2
    lines = re.findall(r"^# genome (\d+) (\S+): (\d+) candidates, (\d+) alive$", g.stderr, re.M)
    assert [(a, b, int(c)) for a, b, c, _ in lines] == [("0", "X", nfp), ("1", "H0", nfp), ("2", "H1", nfp)]
    alive = [int(l[3]) for l in lines]
    assert nfp >= alive[0] >= alive[1] >= alive[2] == nkept
    ka = runs.run("g_ka", *names, "-ka", "--bait-fps", runs.path("g_ka.fps"))
    assert ka.stdout == "" and runs.read("g_ka.fps") == want
    runs.same_counts("g_plain", "g_ka")
