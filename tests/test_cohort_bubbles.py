"""`danbing-tk -ka --cohort MANIFEST -bu --bu-table` (plain `--cohort -bu` stays refused, tests/test_cohort.py): every sample's PREFIX.bub.kmdb from the context's device table (dbtk_bubtab.h), written
by the finisher beside the sample's other files.  Byte-identical to a single `-bu --bu-table` run of the sample, the same set per
locus as the single plain `-bu` run (whose order inside a locus is the reference's hash map's), and the count files are those of
the cohort run without -bu."""
import os

import numpy as np
import pytest

import cases
from test_cohort import fasta_records, manifest, run

pytestmark = pytest.mark.gpu
G4 = os.path.join(cases.GOLDEN, "g4_bait_bubbles")
FLAGS = ["-k", "21", "-cth", "45", "-qs", "pan", "-ka"]


def parse_bub(fn):
    a = np.fromfile(fn, np.uint64)
    nl = int(a[0]); nk = int(a[1 + nl])
    assert a[2 + nl] == 8 and len(a) == 3 + nl + 2 * nk
    got, i, asc = {}, 0, True
    for l in range(nl):
        ks = [int(x) for x in a[3 + nl + i:3 + nl + i + int(a[1 + l])]]
        asc = asc and ks == sorted(ks)
        for j, e in enumerate(ks):
            got[(l, e)] = int(a[3 + nl + nk + i + j])
        i += len(ks)
    return got, asc


def test_cohort_with_bu_writes_each_samples_table(tmp_path):
    tmp = str(tmp_path)
    src = os.path.join(G4, "reads.fa")
    recs = fasta_records(src)
    half = os.path.join(tmp, "half.fa")
    with open(half, "wb") as f:
        for t, s in recs[:(len(recs) // 4) * 2]:
            f.write(t + b"\n" + s + b"\n")
    again = os.path.join(tmp, "again.fa")
    with open(again, "wb") as f:
        f.write(open(src, "rb").read())
    files = [src, half, again]  # (the half between the two whole ones: what a sample leaves in the table would show in the next)
    single_tab, single_log = [], []
    for i, fn in enumerate(files):
        for extra, out in ((["-bu", "--bu-table"], single_tab), (["-bu"], single_log)):
            o = os.path.join(tmp, ("t%d" if extra[-1] == "--bu-table" else "l%d") % i)
            r = run(FLAGS + extra + ["-fa", fn, "-o", o], cwd=G4)
            assert r.returncode == 0, r.stderr[-2000:]
            out.append(o)
    # the single plain -bu run of the golden's own input is the reference binary's file, byte for byte (the existing g4 comparison)
    assert open(single_log[0] + ".bub.kmdb", "rb").read() == open(os.path.join(G4, "refbu.bub.kmdb"), "rb").read()

    def cohort(tag, bu, env=None):
        pre = [os.path.join(tmp, "%s%d" % (tag, i)) for i in range(len(files))]
        m = manifest(tmp_path / (tag + ".tsv"), list(zip(files, pre)))
        r = run(FLAGS + (["-bu", "--bu-table"] if bu else []) + ["--cohort", m], cwd=G4, env=env)
        assert r.returncode == 0 and r.stdout == b"", r.stderr[-3000:]
        return pre

    plain = cohort("p", False)
    for tag, env in (("c", None), ("d", {"DBTK_COHORT_CONTEXTS": "1"})):
        pre = cohort(tag, True, env)
        for i, p in enumerate(pre):
            b = open(p + ".bub.kmdb", "rb").read()
            assert b == open(single_tab[i] + ".bub.kmdb", "rb").read(), (tag, i)
            got, asc = parse_bub(p + ".bub.kmdb")
            want, _ = parse_bub(single_log[i] + ".bub.kmdb")
            assert asc and got == want and (i == 1 or len(got) > 0), (tag, i)
            for ext in (".trkmc.ar", ".tr.summary.txt"):
                x = open(p + ext, "rb").read()
                assert len(x) > 8 and x == open(plain[i] + ext, "rb").read(), (tag, i, ext)
    assert not os.path.exists(plain[0] + ".bub.kmdb")
