"""bin/ktools ksi and bin/ktools sum (host only): the index and the per-locus k-mer sums of the reference's tool
(src/kmertools.cpp:38-137), byte for byte against the reference binary where oracle/_ref holds it, and against numpy's segment sums
where it does not.  Integer sums: no tolerance anywhere.

Compatibility is asked for .ksi files with at least two loci whose first locus is non-empty: the reference indexes past its vector
(or writes nothing) otherwise.  What this tool does there is stated in its usage texts and checked at the end of this file."""
import os
import subprocess

import numpy as np
import pytest

import bind
import cases
import synth

KT = os.path.join(bind.ROOT, "danbing-tk_amd", "bin", "ktools")
G1 = os.path.join(cases.GOLDEN, "g1_k21")
need_ref = pytest.mark.skipif(not synth.have_ref(), reason="oracle/_ref not built")


def run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def kmers_file(path, nks, rng):
    """A pan.tr.kmers-like file: `>locus` lines and one k-mer (a number) per line."""
    with open(path, "w") as f:
        for t, n in enumerate(nks):
            f.write(">%d\n" % t)
            for v in rng.integers(0, 1 << 42, n):
                f.write("%d\n" % v)
    return str(path)


def counts_file(path, counts):
    with open(path, "w") as f:
        f.write("".join("%d\n" % int(c) for c in counts))
    return str(path)


def segment_sums(counts, ksi):
    c = np.concatenate([np.zeros(1, np.uint64), np.cumsum(np.asarray(counts, np.uint64), dtype=np.uint64)])   # (all uint64: exact)
    ksi = np.asarray(ksi, np.int64)
    return c[ksi] - c[np.concatenate([np.zeros(1, np.int64), ksi[:-1]])]


def golden_counts():
    """The second column of the golden -on output: one count per TR k-mer of g1, locus by locus."""
    return [int(l.split()[1]) for l in open(os.path.join(G1, "refon.tr.kmers")) if not l.startswith(">")]


def my_ksi(fn):
    r = run(KT, "ksi", fn)
    assert r.returncode == 0, r.stderr
    return r.stdout


# ---- against the reference binary
@need_ref
def test_ksi_is_the_reference_ksi(tmp_path):
    ref = synth.ref_tool("ktools")
    fn = os.path.join(G1, "pan.tr.kmers")
    want = run(ref, "ksi", fn)
    assert want.returncode == 0 and want.stdout.count(b"\n") == 6          # six loci, all non-empty
    assert len(set(want.stdout.split())) == 6 and want.stdout.split()[0] != b"0"
    assert my_ksi(fn) == want.stdout
    fn = kmers_file(tmp_path / "holes.tr.kmers", [5, 0, 3, 0, 0, 7, 0], np.random.default_rng(1))   # empty loci in the middle and at the end
    want = run(ref, "ksi", fn)
    assert want.stdout == b"5\n5\n8\n8\n8\n15\n15\n"
    assert my_ksi(fn) == want.stdout


@need_ref
@pytest.mark.parametrize("which", ["golden", "random", "holes"])
def test_sum_is_the_reference_sum(which, tmp_path):
    ref = synth.ref_tool("ktools")
    rng = np.random.default_rng(7)
    if which == "holes":
        kf = kmers_file(tmp_path / "h.tr.kmers", [5, 0, 3, 0, 0, 7, 0], rng)
    else:
        kf = os.path.join(G1, "pan.tr.kmers")
    ksi_fn = str(tmp_path / "x.ksi")
    open(ksi_fn, "wb").write(my_ksi(kf))
    ksi = [int(x) for x in open(ksi_fn).read().split()]
    nk = ksi[-1]
    if which == "golden":
        samples = [golden_counts(), [c // 2 for c in golden_counts()], [0] * nk]
        assert len(samples[0]) == nk and any(samples[0])
    else:
        samples = [rng.integers(0, (1 << 40) + 1, nk) for _ in range(3)]
        samples[1][:3] = 1 << 40
    files = [counts_file(tmp_path / ("s%d.txt" % i), c) for i, c in enumerate(samples)]
    # one file, one column
    a, b = str(tmp_path / "a.kms"), str(tmp_path / "b.kms")
    assert run(ref, "sum", ksi_fn, files[0], a).returncode == 0
    r = run(KT, "sum", ksi_fn, files[0], b)
    assert r.returncode == 0, r.stderr
    got = open(b, "rb").read()
    assert got == open(a, "rb").read() and got.count(b"\n") == len(ksi)
    # -f: three samples, a row each
    fofn = str(tmp_path / "files.txt")
    open(fofn, "w").write("".join(f + "\n" for f in files))
    assert run(ref, "sum", "-f", ksi_fn, fofn, a).returncode == 0
    r = run(KT, "sum", "-f", ksi_fn, fofn, b)
    assert r.returncode == 0, r.stderr
    got = open(b, "rb").read()
    assert got == open(a, "rb").read()
    rows = got.decode().split("\n")
    assert rows[-1] == "" and len(rows) == 4 and all(len(x.split("\t")) == len(ksi) for x in rows[:3])
    assert b"3 samples" in r.stderr and b"%d loci" % len(ksi) in r.stderr


@need_ref
def test_usage_texts_are_the_reference_texts():
    ref = synth.ref_tool("ktools")
    for cmd in ("ksi", "sum"):
        want, got = run(ref, cmd), run(KT, cmd)
        assert want.returncode == 0 and got.returncode == 0 and got.stdout == b""
        assert got.stderr.startswith(want.stderr) and len(want.stderr) > 40     # the reference's text, then what differs here
    assert run(KT).returncode == 0 and run(ref).returncode == 0


# ---- without the reference
def test_sum_equals_numpy_segment_sums(tmp_path):
    rng = np.random.default_rng(3)
    for case, nks in enumerate(([4, 1, 9, 2], [3, 0, 0, 5, 1, 0], list(rng.integers(0, 40, 60)) + [0])):
        nks[0] = max(nks[0], 1)
        kf = kmers_file(tmp_path / ("c%d.tr.kmers" % case), nks, rng)
        ksi_txt = my_ksi(kf)
        ksi = [int(x) for x in ksi_txt.split()]
        assert ksi == list(np.cumsum(nks))
        ksi_fn = str(tmp_path / ("c%d.ksi" % case))
        open(ksi_fn, "wb").write(ksi_txt)
        samples = [rng.integers(0, (1 << 40) + 1, ksi[-1]).astype(np.uint64) for _ in range(3)]
        samples[2][:] = np.uint64((1 << 64) - 1) // np.uint64(max(ksi[-1], 1))          # large sums, still below 2^64
        files = [counts_file(tmp_path / ("c%d_s%d.txt" % (case, i)), c) for i, c in enumerate(samples)]
        out = str(tmp_path / "o.kms")
        r = run(KT, "sum", ksi_fn, files[0], out)
        assert r.returncode == 0, r.stderr
        assert [int(x) for x in open(out).read().split("\n")[:-1]] == [int(x) for x in segment_sums(samples[0], ksi)]
        fofn = str(tmp_path / "files.txt")
        open(fofn, "w").write("".join(f + "\n" for f in files))
        r = run(KT, "sum", "-f", ksi_fn, fofn, out)
        assert r.returncode == 0, r.stderr
        rows = open(out).read().split("\n")
        assert rows[-1] == "" and len(rows) == 4
        for row, c in zip(rows, samples):
            assert [int(x) for x in row.split("\t")] == [int(x) for x in segment_sums(c, ksi)]


def test_where_the_reference_is_undefined(tmp_path):
    """A single-locus index, a leading empty locus, a count file of the wrong length: what the usage texts say."""
    rng = np.random.default_rng(5)
    u = run(KT, "sum")
    assert u.returncode == 0 and b"single-locus" in u.stderr and b"leading empty locus" in u.stderr and b"refused" in u.stderr
    assert b"single locus" in run(KT, "ksi").stderr
    one = kmers_file(tmp_path / "one.tr.kmers", [6], rng)
    assert my_ksi(one) == b"6\n"
    open(str(tmp_path / "one.ksi"), "w").write("6\n")
    c = counts_file(tmp_path / "c.txt", [1, 2, 3, 4, 5, 1 << 40])
    out = str(tmp_path / "o.kms")
    assert run(KT, "sum", tmp_path / "one.ksi", c, out).returncode == 0
    assert open(out).read() == "%d\n" % (15 + (1 << 40))
    open(str(tmp_path / "lead.ksi"), "w").write("0\n0\n4\n6\n")
    assert run(KT, "sum", tmp_path / "lead.ksi", c, out).returncode == 0
    assert open(out).read() == "0\n0\n10\n%d\n" % (5 + (1 << 40))
    for bad in ([1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 6, 7]):
        r = run(KT, "sum", tmp_path / "lead.ksi", counts_file(tmp_path / "bad.txt", bad), out)
        assert r.returncode == 1 and b"expects 6 counts" in r.stderr and not os.path.exists(out)
    assert run(KT, "sum", tmp_path / "nope.ksi", c, out).returncode == 134            # the reference asserts on a file it cannot open
    assert run(KT, "frobnicate").returncode == 1
