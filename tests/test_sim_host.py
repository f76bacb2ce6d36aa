"""The host part of include/dbtk_sim.h (no device): the model of tests/sim_model.py against the compiled `sim_reads`, and
dbtk_sim_info / dbtk_sim_describe / dbtk_sim_labels against the model — fragments, source loci, and what dbtk_sim_open refuses."""
import os
import random
import re
import subprocess

import pytest

import bind
import sim_model
import synth

pkg = bind.pkg
abi = bind.abi

# contigs of 499, 500, 501, 519, 520 and 1234 bases: single- and multi-line, lower case, N, a header with blanks
SIZES = (499, 500, 501, 519, 520, 1234)
PARAMS = ((500, 150, 15, 500), (500, 150, 7, 0), (40, 17, 34, 30), (300, 150, 15, 1), (500, 250, 300, 1))  # (FLEN, RLEN, cv, ML)


def six_contigs(seed=7):
    rng = random.Random(seed)
    out = []
    for i, n in enumerate(SIZES):
        s = [rng.choice("ACGT") for _ in range(n)]
        for j in range(n):
            x = rng.random()
            if x < 0.05:
                s[j] = s[j].lower()
            elif x < 0.08:
                s[j] = "N"
            elif x < 0.09:
                s[j] = "n"
        for j in (0, n - 1):  # the first and last base of a contig reach the first base of /1 and of /2
            s[j] = s[j].lower() if i % 2 else "N"
        out.append((f">ctg{i} len={n} some words" if i % 3 == 0 else f">ctg{i}", "".join(s)))
    return out


def fasta_text(contigs, width=(0, 60, 0, 61, 70, 100)):
    out = []
    for (h, s), w in zip(contigs, (width * (len(contigs) // len(width) + 1))[:len(contigs)]):
        out.append(h)
        out += [s] if not w else [s[i:i + w] for i in range(0, len(s), w)]
    return "".join(x + "\n" for x in out)


def test_fasta_round_trip_of_the_model():
    c = six_contigs()
    assert sim_model.parse_fasta(fasta_text(c)) == c


@pytest.mark.ref
@pytest.mark.parametrize("flen,rlen,cv,ml", PARAMS)
def test_model_equals_the_compiled_sim_reads(tmp_path, flen, rlen, cv, ml):
    exe = os.path.join(synth.REFDIR, "sim_reads")
    if not synth.have_ref() or not os.path.exists(exe):
        pytest.skip("oracle/_ref/sim_reads is not built")
    c = six_contigs()
    fa = tmp_path / "a.fa"
    fa.write_text(fasta_text(c))
    # (no -o: the records go to stdout, src/sim_reads.cpp:225-231; it still creates an empty ".allctgs.reads.fa" where it runs)
    r = subprocess.run([exe, "-i", str(fa), "-pe", "-no-err", "-fs", str(flen), "-rlen", str(rlen), "-c", str(cv), "-ml", str(ml)], capture_output=True, text=True,
                       timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    want = sim_model.sim_reads_text(c, flen, rlen, cv, ml)
    assert r.stdout == want and want.count("\n") % 4 == 0
    for h, s in c:
        assert (f"Contig {h} ignored, size = {len(s)} < MIN_CTG_LEN" in r.stderr) == (len(s) < ml)


# ---- the BED: every rule of the source locus on contig ctg5 (1234 bases), FLEN 500, SHFT 20 (begs 0, 20, ..., 720)
NLOCI = 9
BED = [
    ("ctg5", 0, 3, 8),          # an interval at position 0
    ("ctg5", 600, 640, 5),      # overlapping ...
    ("ctg5", 620, 700, 2),      # ... the one before, and holding
    ("ctg5", 630, 650, 7),      # ... a nested one
    ("ctg5", 500, 520, 4),      # ends exactly at beg = 520: must not count there; starts exactly at beg + FLEN for beg = 0: must not count there
    ("ctg5", 1100, 1234, 1),
    ("ctg5", 1200, 1220, 0),
    ("ctg0", 10, 20, 3),        # a skipped contig (499 bases < ML 500)
    ("nosuch", 10, 20, 3),      # an unknown contig
    ("ctg3", 100, 101, 6),      # one base, on a contig with one fragment (519 bases)
    ("ctg4", 519, 520, 6),      # the last base of a contig with two fragments (begs 0, 20)
]


def bed_text(bed):
    return "".join(f"{c}\t{s}\t{e}\t{l}\n" for c, s, e, l in bed)


def open_sim(tmp_path, contigs, bed, nloci, flen, rlen, cv, ml, name="a"):
    fa, bd = tmp_path / (name + ".fa"), tmp_path / (name + ".bed")
    fa.write_text(fasta_text(contigs))
    bd.write_text(bed if isinstance(bed, str) else bed_text(bed))
    return pkg.Sim(pkg.Dbtk(), str(fa), str(bd), nloci, flen, rlen, cv, ml)


def test_binding_knows_the_entry_points_and_the_versions():
    hdr = open(os.path.join(bind.ROOT, "include", "dbtk_sim.h")).read()
    assert "#define DBTK_SIM_API_VERSION 1u" in hdr and abi.SIM_API_VERSION == 1 and abi.ABI_VERSION == 11
    lib = pkg.Dbtk()
    for s in pkg.EXPORTS_SIM:
        assert hasattr(lib.L, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    khdr = open(os.path.join(bind.ROOT, "include", "dbtk_kcp.h")).read()
    assert "dbtk_kcp_add_device" in pkg.EXPORTS_KCP and hasattr(lib.L, "dbtk_kcp_add_device") and re.search(r"\bdbtk_kcp_add_device\s*\(", khdr)


@pytest.mark.parametrize("flen,rlen,cv,ml", PARAMS)
def test_info_and_describe_equal_the_model(tmp_path, capfd, flen, rlen, cv, ml):
    c = six_contigs()
    s = open_sim(tmp_path, c, BED, NLOCI, flen, rlen, cv, ml)
    err = capfd.readouterr().err
    for h, q in c:
        assert (f"Contig {h} ignored, size = {len(q)} < MIN_CTG_LEN\n" in err) == (len(q) < ml)
    bed = sim_model.parse_bed(bed_text(BED))
    ctg, beg, src = sim_model.describe(c, bed, NLOCI, flen, rlen, cv, ml)
    f = s.info()
    kept = sim_model.kept(c, ml)
    assert (f.ncontigs, f.nskipped, f.nfrags, f.arena_bytes) == (len(kept), len(c) - len(kept), len(ctg), sum(len(q) for _, q in kept))
    assert (f.flen, f.rlen, f.shft, f.ngroups) == (flen, rlen, 2 * rlen // cv, 0) and f.nbreaks >= f.ncontigs
    gc, gb, gs = s.describe()
    assert gc.tolist() == ctg and gb.tolist() == beg and gs.tolist() == src
    # any sub-range, and one fragment at a time
    for first, n in ((0, 1), (len(ctg) // 3, len(ctg) // 2), (len(ctg) - 1, 1), (len(ctg), 0)):
        a, b, d = s.describe(first, n)
        assert a.tolist() == ctg[first:first + n] and b.tolist() == beg[first:first + n] and d.tolist() == src[first:first + n]
    first = 0
    for i, (h, q) in enumerate(kept):
        hdr, bases, ff = s.contig(i)
        assert (hdr, bases.decode(), ff) == (h, q, first)
        first += ctg.count(i)
    for fr in range(0, len(ctg), 3):
        assert s.labels(fr) == sim_model.labels_of(bed, sim_model.name_of(kept[ctg[fr]][0]), beg[fr], flen)
    s.close()


def test_the_bed_rules_one_by_one(tmp_path):
    """FLEN 500, SHFT 20, ML 500: ctg0 (499 bases) is skipped; on ctg5 the fragments start at 0, 20, ..., 720"""
    c = six_contigs()
    s = open_sim(tmp_path, c, BED, NLOCI, 500, 150, 15, 500)
    ctg, beg, src = s.describe()
    at = {(int(a), int(b)): int(d) for a, b, d in zip(ctg, beg, src)}
    k5 = 4  # ctg5 is the fifth kept contig
    assert at[(k5, 0)] == 8                       # [0, 3) at position 0 — and [500, 520) starts at beg + FLEN: not counted (else 4)
    assert at[(k5, 20)] == 4                      # [500, 520) overlaps [20, 520) by its whole length
    assert at[(k5, 500)] == 2 and at[(k5, 520)] == 2   # [500, 520) ends exactly at beg = 520: not counted; the lowest of 5, 2, 7 is
    assert at[(k5, 100)] == 4 and at[(k5, 120)] == 4   # [600, 640) starts at beg + FLEN for beg = 100: only 4 there; at 120 also 5
    assert at[(k5, 140)] == 2                          # ... and at 140 all of 4, 5, 2, 7
    assert at[(k5, 600)] == 2 and at[(k5, 620)] == 1   # [1100, 1234) starts at beg + FLEN for beg = 600
    assert at[(k5, 700)] == 1 and at[(k5, 720)] == 0
    assert s.labels(next(i for i, (a, b) in enumerate(zip(ctg, beg)) if (a, b) == (k5, 140))) == [2, 4, 5, 7]
    k3, k4 = 2, 3
    assert at[(k3, 0)] == 6 and at[(k4, 0)] == NLOCI and at[(k4, 20)] == 6
    assert set(src.tolist()) == {0, 1, 2, 4, 6, 8, NLOCI}
    s.close()


def refused(tmp_path, contigs, bed, status, *words, nloci=NLOCI, flen=500, rlen=150, cv=15, ml=1, fasta=None):
    try:
        if fasta is not None:
            fa, bd = tmp_path / "x.fa", tmp_path / "x.bed"
            fa.write_text(fasta)
            bd.write_text(bed_text(bed))
            pkg.Sim(pkg.Dbtk(), str(fa), str(bd), nloci, flen, rlen, cv, ml)
        else:
            open_sim(tmp_path, contigs, bed, nloci, flen, rlen, cv, ml, name="x")
    except pkg.DbtkError as e:
        assert e.status == status and all(w in str(e) for w in words), str(e)
    else:
        raise AssertionError("accepted: " + " ".join(words))


def test_refusals(tmp_path):
    c = six_contigs()
    # a bad base, with contig and offset (the offset counts bases, not bytes of the file: the contig is multi-line)
    bad = list(c)
    h, q = bad[4]
    bad[4] = (h, q[:300] + "R" + q[301:])
    refused(tmp_path, bad, [], abi.ERR_FORMAT, "contig >ctg4", "offset 300", "byte 82")
    bad[4] = (h, q[:77] + "-" + q[78:])
    refused(tmp_path, bad, [], abi.ERR_FORMAT, "contig >ctg4", "offset 77", "byte 45")
    refused(tmp_path, c, [], abi.ERR_ARG, "RLEN 500", flen=500, rlen=500)       # the reference segfaults
    refused(tmp_path, c, [], abi.ERR_ARG, "RLEN 501", flen=500, rlen=501)
    refused(tmp_path, c, [], abi.ERR_ARG, "DBTK_MAX_READ_LEN", flen=500, rlen=257)
    refused(tmp_path, c, [], abi.ERR_ARG, "cv 301", flen=500, rlen=150, cv=301)  # SHFT = 0: the reference never ends
    refused(tmp_path, c, [], abi.ERR_ARG, "cv 0", cv=0)
    refused(tmp_path, c, [("ctg5", 30, 30, 1)], abi.ERR_FORMAT, "line 1", "START 30", "END 30")
    refused(tmp_path, c, [("ctg5", 1, 2, 1), ("ctg5", 31, 30, 1)], abi.ERR_FORMAT, "line 2", "START 31")
    refused(tmp_path, c, [("ctg5", 1, 2, NLOCI)], abi.ERR_FORMAT, "line 1", f"LOCUS {NLOCI}")
    refused(tmp_path, c, [("nosuch", 1, 2, NLOCI)], abi.ERR_FORMAT, f"LOCUS {NLOCI}")  # (checked before the contig is looked up)
    refused(tmp_path, None, [], abi.ERR_FORMAT, "'>'", fasta="ACGT\n>c\nACGT\n")
    try:
        pkg.Sim(pkg.Dbtk(), str(tmp_path / "absent.fa"), str(tmp_path / "x.bed"), NLOCI)
    except pkg.DbtkError as e:
        assert e.status == abi.ERR_IO
    else:
        raise AssertionError("an absent FASTA was accepted")


def test_crlf_and_a_last_line_without_newline(tmp_path):
    c = [(">a x", "ACGTNacgtn" * 6), (">b", "TTTTGGGGCC" * 7)]
    fa, bd = tmp_path / "w.fa", tmp_path / "w.bed"
    fa.write_bytes(b">a x\r\n" + c[0][1][:25].encode() + b"\r\n" + c[0][1][25:].encode() + b"\r\n>b\r\n" + c[1][1].encode())
    bd.write_bytes(b"a\t0\t5\t1\r\nb\t69\t70\t0")
    s = pkg.Sim(pkg.Dbtk(), str(fa), str(bd), 2, 40, 17, 34, 1)
    bed = [("a", 0, 5, 1), ("b", 69, 70, 0)]
    assert [x.tolist() for x in s.describe()] == [list(x) for x in sim_model.describe(c, bed, 2, 40, 17, 34, 1)]
    assert s.contig(0)[:2] == (">a x", c[0][1].encode()) and s.contig(1)[:2] == (">b", c[1][1].encode())
    s.close()
