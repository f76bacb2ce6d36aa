"""`danbing-tk --cohort MANIFEST --kms OUT.kms` / `--dosage IKMER.META OUT.dosage.tsv OUT.bias.tsv` and `danbing-tk-pred --dosage`:
the per-locus tables of a cohort run without the genotype matrix, on the fixtures of tests/test_cohort.py.

CPU: what the flags refuse at parse time (exit status 1, the flag named, nothing loaded).
GPU: OUT.kms against the segment sums of every sample's single-run OUT.trkmc.ar (integers: exact); the bias TSV byte-identical to
--pred's (the same operations in the same order, the same normalisation kernel); danbing-tk-pred --dosage on the per-sample files
writes the same three tables byte for byte (the same kernels over the same counts).  No tolerance in this file."""
import os
import subprocess

import numpy as np
import pytest

import bind
from test_cohort import CLI, G1, G1_FLAGS, GOLDEN, PRED, SETS, golden_ikmer_meta, make_samples, manifest, run, single_runs

KT = os.path.join(bind.ROOT, "danbing-tk_amd", "bin", "ktools")


# ------------------------------------------------------------------- CPU ---
def test_usage_lists_the_table_flags():
    r = run([])
    assert r.returncode == 0
    for flag in (b"--kms <OUT.kms>", b"--dosage <IKMER.META> <OUT.dosage.tsv> <OUT.bias.tsv>"):
        assert flag in r.stderr, flag
    r = subprocess.run([PRED], capture_output=True)
    assert r.returncode == 0 and b"--dosage <OUT.dosage.tsv> [--kms <OUT.kms>]" in r.stderr


def test_refusals_at_parse_time(tmp_path):
    ik = tmp_path / "ikmer.meta"
    ik.write_bytes(b"\0" * 24)
    three = manifest(tmp_path / "m3.tsv", [("reads.fa", tmp_path / "s0", 30)])
    two = manifest(tmp_path / "m2.tsv", [("reads.fa", tmp_path / "s0")])
    dos = [str(ik), str(tmp_path / "dos.tsv"), str(tmp_path / "bias.tsv")]
    nodir = str(tmp_path / "no_such_dir" / "x")

    def refused(args, *words):
        r = run(G1_FLAGS + args, cwd=G1)
        assert r.returncode == 1, (args, r.stderr[-500:])
        for w in words:
            assert w in r.stderr, (args, w, r.stderr[-500:])
        assert b"danbing-tk:" in r.stderr and r.stdout == b"" and b"total number of loci" not in r.stderr   # nothing was loaded
        assert sorted(os.listdir(str(tmp_path))) == ["ikmer.meta", "m2.tsv", "m3.tsv", "single"]

    # without --cohort (-o empties its OUT.trkmc.ar while the flags are read, like the reference: it gets a directory of its own)
    os.makedirs(str(tmp_path / "single"))
    refused(["-fa", "reads.fa", "-o", str(tmp_path / "single" / "x"), "--kms", str(tmp_path / "o.kms")], b"--kms", b"--cohort")
    refused(["-fa", "reads.fa", "-o", str(tmp_path / "single" / "x"), "--dosage"] + dos, b"--dosage", b"--cohort")
    # --dosage needs the depth column; --kms alone does not (it fails later, on the reads file, not on the manifest)
    refused(["--cohort", two, "--dosage"] + dos, b"line 1", b"depth", b"--dosage")
    refused(["--cohort", two, "--kms", str(tmp_path / "o.kms"), "--dosage"] + dos, b"line 1", b"depth")
    # files: IKMER.META readable, every output creatable
    refused(["--cohort", three, "--dosage", str(tmp_path / "none.meta")] + dos[1:], b"--dosage: cannot open", b"none.meta")
    refused(["--cohort", three, "--dosage", dos[0], nodir, dos[2]], b"--dosage: cannot create", b"no_such_dir")
    refused(["--cohort", three, "--dosage", dos[0], dos[1], nodir], b"--dosage: cannot create", b"no_such_dir")
    refused(["--cohort", three, "--kms", nodir], b"--kms: cannot create", b"no_such_dir")
    refused(["--cohort", two, "--kms", nodir], b"--kms: cannot create")      # (two columns pass the manifest check with --kms alone)
    # --no-trkmc still needs something to write
    refused(["--cohort", three, "--no-trkmc"], b"--no-trkmc", b"--kms")
    # danbing-tk-pred
    r = subprocess.run([PRED, "--kms", str(tmp_path / "o.kms"), "a", "b", "c", "d", "e"], capture_output=True)
    assert r.returncode == 1 and b"--kms needs --dosage" in r.stderr
    r = subprocess.run([PRED, "--dosage", str(tmp_path / "d.tsv"), "a", "b"], capture_output=True)
    assert r.returncode == 1 and b"3 file arguments" in r.stderr


# ------------------------------------------------------------------- GPU ---
def kms_rows(fn):
    text = open(fn).read()
    assert text.endswith("\n")
    return [[int(x) for x in row.split("\t")] for row in text.split("\n")[:-1]]


def segment_rows(prefixes, nk_cum):
    rows = []
    for p in prefixes:
        a = np.fromfile(p + ".trkmc.ar", np.uint64)
        assert a[0] == len(a) - 1 == nk_cum[-1]
        c = np.concatenate([np.zeros(1, np.uint64), np.cumsum(a[1:], dtype=np.uint64)])
        e = np.asarray(nk_cum, np.int64)
        rows.append([int(x) for x in c[e] - c[np.concatenate([np.zeros(1, np.int64), e[:-1]])]])
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["g1", "g5"])
def test_cohort_kms_equals_segment_sums_of_single_runs(name, tmp_path):
    spec = SETS[name]
    gdir = os.path.join(GOLDEN, spec["dir"])
    tmp = str(tmp_path)
    files = make_samples(gdir, tmp)
    ns = len(files)
    sep = single_runs(spec, gdir, files, os.path.join(tmp, "sep"))
    meta = golden_ikmer_meta(gdir, os.path.join(tmp, "ikmer.meta"))      # (only for the loci's k-mer counts: OUT.trkmc.ar is locus by locus)
    want = segment_rows(sep, meta["nk_cum"])
    assert any(any(r) for r in want) and not any(want[4])
    os.makedirs(os.path.join(tmp, "coh"))
    pre = [os.path.join(tmp, "coh", "c%d" % i) for i in range(ns)]
    kms = os.path.join(tmp, "coh.kms")
    r = run(spec["flags"] + ["--cohort", manifest(tmp_path / "m.tsv", list(zip(files, pre))), "--kms", kms], cwd=gdir)   # no depth column
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == b"" and kms_rows(kms) == want
    for i, p in enumerate(pre):
        assert open(p + ".trkmc.ar", "rb").read() == open(sep[i] + ".trkmc.ar", "rb").read()
    # the table `ktools sum -f` makes from the same counts as text, with the index `ktools ksi` makes from the RPGG
    ksi = os.path.join(tmp, "pan.ksi")
    open(ksi, "wb").write(subprocess.run([KT, "ksi", os.path.join(gdir, "pan.tr.kmers")], stdout=subprocess.PIPE, check=True).stdout)
    with open(os.path.join(tmp, "files.txt"), "w") as f:
        for i, p in enumerate(sep):
            fn = os.path.join(tmp, "t%d.txt" % i)
            open(fn, "w").write("".join("%d\n" % int(c) for c in np.fromfile(p + ".trkmc.ar", np.uint64)[1:]))
            f.write(fn + "\n")
    if [int(x) for x in open(ksi).read().split()] == [int(x) for x in meta["nk_cum"]]:   # (no duplicate k-mer lines within a locus)
        assert subprocess.run([KT, "sum", "-f", ksi, os.path.join(tmp, "files.txt"), os.path.join(tmp, "kt.kms")], capture_output=True).returncode == 0
        assert open(os.path.join(tmp, "kt.kms"), "rb").read() == open(kms, "rb").read()
    # --no-trkmc: the same table, no per-sample file; the prefix column is ignored
    kms2 = os.path.join(tmp, "nt.kms")
    rows = [(f, os.path.join(tmp, "nowhere", "c%d" % i)) for i, f in enumerate(files)]
    r = run(spec["flags"] + ["--cohort", manifest(tmp_path / "mnt.tsv", rows), "--kms", kms2, "--no-trkmc"], cwd=gdir)
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(kms2, "rb").read() == open(kms, "rb").read()
    assert not os.path.exists(os.path.join(tmp, "nowhere")) and r.stderr.decode().count("reads processed in total.") == ns


@pytest.mark.gpu
def test_cohort_dosage_beside_pred_and_the_pred_tool(tmp_path):
    spec = SETS["g1"]
    gdir = os.path.join(GOLDEN, spec["dir"])
    tmp = str(tmp_path)
    files = make_samples(gdir, tmp)
    ns = len(files)
    depths = [30.5, 0.75, 41.0, 17.25, 3.0, 55.125][:ns]
    ik = os.path.join(tmp, "ikmer.meta")
    meta = golden_ikmer_meta(gdir, ik)
    sep = single_runs(spec, gdir, files, os.path.join(tmp, "sep"))
    os.makedirs(os.path.join(tmp, "coh"))
    pre = [os.path.join(tmp, "coh", "c%d" % i) for i in range(ns)]
    mat = [os.path.join(tmp, "coh." + x) for x in ("raw.gt", "cor.gt", "bias.tsv")]
    tab = [os.path.join(tmp, "coh." + x) for x in ("dosage.tsv", "dbias.tsv", "kms")]
    m = manifest(tmp_path / "m.tsv", [(f, p, repr(d)) for f, p, d in zip(files, pre, depths)])
    r = run(spec["flags"] + ["--cohort", m, "--pred", ik] + mat + ["--dosage", ik, tab[0], tab[1], "--kms", tab[2]], cwd=gdir)
    assert r.returncode == 0, r.stderr[-3000:]
    bias = open(tab[1], "rb").read()
    assert bias == open(mat[2], "rb").read() and len(bias) > 20          # byte-identical to --pred's bias table
    want = segment_rows(sep, meta["nk_cum"])
    assert kms_rows(tab[2]) == want
    # the dosage table: %g of float32(kms / depth / Bias), uncorrected at the locus without invariant k-mers (locus 1)
    dos = [[float(x) for x in row.split("\t")] for row in open(tab[0]).read().split("\n")]
    assert len(dos) == ns and all(len(row) == meta["ntr"] for row in dos)
    for s in range(ns):
        assert dos[s][1] == float("%g" % (np.float32(want[s][1]) / np.float32(depths[s])))
    # the sample that hits nothing: its Bias is exactly 0, so 0 / 0 at the corrected loci (the IEEE result, include/dbtk_pred.h), 0 where uncorrected
    assert dos[4][1] == 0.0 and all(np.isnan(v) for t, v in enumerate(dos[4]) if t != 1)
    # danbing-tk-pred --dosage on the per-sample files: the same three tables, byte for byte
    with open(os.path.join(tmp, "gt.meta.txt"), "w") as f:
        for p, d in zip(sep, depths):
            f.write("%s.trkmc.ar\t%r\n" % (p, d))
    two = [os.path.join(tmp, "two." + x) for x in ("dosage.tsv", "dbias.tsv", "kms")]
    r = subprocess.run([PRED, "--dosage", two[0], "--kms", two[2], os.path.join(tmp, "gt.meta.txt"), ik, two[1]], capture_output=True)
    assert r.returncode == 0, r.stderr
    for a, b in zip(two, tab):
        assert open(a, "rb").read() == open(b, "rb").read(), a
    assert sorted(x for x in os.listdir(tmp) if x.startswith("two.")) == ["two.dbias.tsv", "two.dosage.tsv", "two.kms"]   # no matrix file
    # tables only
    nt = [os.path.join(tmp, "nt." + x) for x in ("dosage.tsv", "dbias.tsv")]
    rows = [(f, "", repr(d)) for f, d in zip(files, depths)]
    r = run(spec["flags"] + ["--cohort", manifest(tmp_path / "mnt.tsv", rows), "--dosage", ik, nt[0], nt[1], "--no-trkmc"], cwd=gdir)
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(nt[0], "rb").read() == open(tab[0], "rb").read() and open(nt[1], "rb").read() == open(tab[1], "rb").read()


@pytest.mark.gpu
def test_failing_sample_writes_no_table(tmp_path):
    spec = SETS["g1"]
    gdir = os.path.join(GOLDEN, spec["dir"])
    tmp = str(tmp_path)
    files = make_samples(gdir, tmp)[:4]
    files[2] = os.path.join(tmp, "missing.fa")
    ik = os.path.join(tmp, "ikmer.meta")
    golden_ikmer_meta(gdir, ik)
    rows = [(f, "", 30) for f in files]
    outs = [os.path.join(tmp, x) for x in ("o.dosage.tsv", "o.bias.tsv", "o.kms")]
    r = run(spec["flags"] + ["--cohort", manifest(tmp_path / "m.tsv", rows), "--dosage", ik, outs[0], outs[1], "--kms", outs[2], "--no-trkmc"], cwd=gdir)
    assert r.returncode != 0 and ("sample 2 (%s): " % files[2]) in r.stderr.decode()
    assert not any(os.path.exists(x) for x in outs)
