"""`danbing-tk --eval PREF` on the GPU: a two-haplotype --sim run over a 4-locus RPGG whose BED lines are the loci's own TR intervals.
PREF.eval.tsv and PREF.pred equal the model's text computed from the run's own OUT.trkmc.ar and the model's truth; the dumped truth
is the model's; every other output is that of the same command without the flags; and a -fa run over the annotated FASTA of the same
pairs, scored against the dumped truth, writes the same two files."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bind
import eval_cases
import eval_model
import sim_cases
import sim_model

pkg = bind.pkg
ROOT = bind.ROOT
EXE = os.path.join(ROOT, "danbing-tk_amd", "bin", "danbing-tk")
K, NLOCI, CTH = sim_cases.K, sim_cases.NLOCI, sim_cases.CTH
pytestmark = pytest.mark.gpu


class Case:
    def __init__(self, d):
        self.asm = a = sim_cases.AsmCase(d)
        self.dir = d
        # every locus under its own label, and nothing else: each window of an interval is then a TR k-mer of its locus (windows = Sx),
        # which is what a truth file, holding no windows, lets a later run assume
        self.beds, self.bed = [], []
        for h in range(2):
            extra = a.beds[h][2]   # (sim_cases: the second label over the start of locus 1)
            assert extra[2] - extra[1] == 80 and len(a.beds[h]) == NLOCI + 1
            main = [b for i, b in enumerate(a.beds[h]) if i != 2]
            self.beds.append([(c, s, e, l) for l, (c, s, e, _) in enumerate(main)])
            fn = os.path.join(d, f"clean{h}.bed")
            with open(fn, "w") as f:
                f.write("".join(f"{c}\t{s}\t{e}\t{l}\n" for c, s, e, l in self.beds[h]))
            self.bed.append(fn)
        self.annot = os.path.join(d, "annot.fa")
        with open(self.annot, "w") as f:
            for h in range(2):
                f.write(sim_model.annotated_fasta(a.contigs[h], self.beds[h], sim_cases.FLEN, sim_cases.RLEN, sim_cases.CV, 1))
        g = pkg.Dbtk().load(a.pref, K)
        slots, flank, self.beg = eval_cases.order_of(g)
        self.nk = g.ntrkmers
        g.close()
        wc = [dict() for _ in range(NLOCI)]
        for h in range(2):
            wc = eval_model.add_counts(wc, eval_model.window_counts(a.contigs[h], self.beds[h], K, NLOCI))
        self.x, self.w = eval_model.truth(wc, slots, self.nk)
        assert sum(self.x) > 500

    def run(self, out, how, *flags, ok=True):
        a = self.asm
        src = ["-s", "2", "-fa", self.annot] if how == "fa" else ["--sim", a.fa[0], self.bed[0], "--sim", a.fa[1], self.bed[1], "--sim-ml", "1"]
        env = dict(os.environ, DBTK_SIM_BATCH_PAIRS="97")
        r = subprocess.run([EXE, "-k", str(K), "-qs", a.pref, "-o", os.path.join(self.dir, out), "-cth", str(CTH), "-p", "1", *src, *flags], capture_output=True, text=True,
                           timeout=300, env=env)
        assert (r.returncode == 0) == ok, r.stderr[-2000:]
        return r

    def read(self, name):
        return open(os.path.join(self.dir, name), "rb").read()

    def counts(self, out):
        b = self.read(out + ".trkmc.ar")
        assert struct.unpack("<Q", b[:8])[0] == self.nk and len(b) == 8 + 8 * self.nk
        return np.frombuffer(b[8:], np.uint64).tolist()

    def want_text(self, out, windows):
        s = eval_model.sums(self.x, self.counts(out), self.beg, windows=windows)
        return eval_model.tsv_text(s).encode(), eval_model.pred_text(s).encode()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return Case(str(tmp_path_factory.mktemp("evalcli")))


TOTALS = ("reads processed in total", "reads assigned to TR region", "reads removed by kmer-filter", "reads removed during locus assignment")


def totals(r):
    return [l for l in r.stderr.split("\n") if any(t in l for t in TOTALS)]


def test_sim_eval_writes_the_models_text_and_changes_no_other_output(case):
    d = case.dir
    P, T = os.path.join(d, "P"), os.path.join(d, "T.ar")
    plain = case.run("plain", "sim")
    ev = case.run("ev", "sim", "--eval", P, "--eval-dump-truth", T)
    assert ev.stdout == plain.stdout and ev.stdout.count("\n") > 50   # the kam text
    for ext in (".trkmc.ar", ".tr.summary.txt"):
        assert case.read("ev" + ext) == case.read("plain" + ext) and len(case.read("ev" + ext)) > 0
    assert totals(ev) == totals(plain) and len(totals(ev)) == len(TOTALS)
    tsv, pred = case.want_text("ev", case.w)
    assert case.read("P.eval.tsv") == tsv and case.read("P.pred") == pred
    assert case.read("T.ar") == struct.pack("<Q", case.nk) + np.array(case.x, np.uint64).tobytes()
    assert case.w == [sum(case.x[case.beg[l]:case.beg[l + 1]]) for l in range(NLOCI)]   # (this case: every window is a TR k-mer of its locus)
    rows = tsv.decode().split("\n")[1:-1]
    assert len(rows) == NLOCI and sum(float(r.split("\t")[11]) > 0 for r in rows) >= 2       # loci with a slope
    line = [l for l in ev.stderr.split("\n") if l.startswith("--eval:")]
    assert len(line) == 1 and f"{NLOCI} loci scored, {sum(case.w)} windows, {sum(case.w)} look-ups" in line[0] and "k_eval_truth" in line[0] and "k_eval_sums" in line[0]
    assert "--eval" not in plain.stderr
    # -ka alone: the asynchronous batches
    ka = case.run("ka", "sim", "-ka", "--eval", os.path.join(d, "Pka"))
    assert ka.stdout == "" and case.read("ka.trkmc.ar") == case.read("plain.trkmc.ar")
    assert case.read("Pka.eval.tsv") == tsv and case.read("Pka.pred") == pred


def test_reads_from_a_file_scored_against_the_dumped_truth(case):
    d = case.dir
    T = os.path.join(d, "T.ar")
    if not os.path.exists(T):
        case.run("ev", "sim", "--eval", os.path.join(d, "P"), "--eval-dump-truth", T)
    fa = case.run("fa", "fa", "--eval", os.path.join(d, "P2"), "--eval-truth", T)
    assert case.read("fa.trkmc.ar") == case.read("ev.trkmc.ar")
    assert case.read("P2.eval.tsv") == case.read("P.eval.tsv") and case.read("P2.pred") == case.read("P.pred")
    tsv, pred = case.want_text("fa", None)   # (a truth file holds no windows: windows = Sx)
    assert case.read("P2.eval.tsv") == tsv and case.read("P2.pred") == pred
    # a truth file of another RPGG build
    other = os.path.join(d, "other.ar")
    with open(other, "wb") as f:
        f.write(struct.pack("<Q", case.nk - 1) + bytes(8 * (case.nk - 1)))
    r = case.run("bad", "fa", "--eval", os.path.join(d, "P3"), "--eval-truth", other, ok=False)
    assert r.returncode == 1 and "--eval-truth" in r.stderr and f"holds {case.nk - 1} counts" in r.stderr and "Buffered reading" not in r.stderr
    # (nothing was scored or counted: the count file is the empty one the parser leaves, as the reference's does)
    assert not os.path.exists(os.path.join(d, "P3.pred")) and case.read("bad.trkmc.ar") == b"" and not os.path.exists(os.path.join(d, "bad.tr.summary.txt"))
