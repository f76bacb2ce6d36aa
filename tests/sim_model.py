"""Model of `sim_reads -pe -no-err` (the reference's src/sim_reads.cpp:225-231, records as printed to stdout) and of the source
locus that `bedtools map -o distinct_sort_num` + the aligner's stoull give a fragment — both written naively, for the tests of
include/dbtk_sim.h."""
import numpy as np

COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def parse_fasta(text):
    """[(header line with '>', concatenated sequence lines)]"""
    out = []
    for line in text.split("\n"):
        line = line.rstrip("\r")
        if line.startswith(">"):
            out.append([line, []])
        elif line and out:
            out[-1][1].append(line)
    return [(h, "".join(s)) for h, s in out]


def kept(contigs, ml):
    return [(h, s) for h, s in contigs if len(s) >= ml]


def fragments(contigs, flen=500, rlen=150, cv=15, ml=50000):
    """[(kept contig index, beg)] in output order"""
    shft = 2 * rlen // cv
    assert 0 < rlen < flen and shft > 0
    out = []
    for ci, (_, s) in enumerate(kept(contigs, ml)):
        beg = 0
        while beg + flen <= len(s):
            out.append((ci, beg))
            beg += shft
    return out


def mates(seq, beg, flen, rlen):
    """(/1 read, /2 read) of the fragment at beg"""
    r1 = seq[beg:beg + rlen].upper()
    r2 = "".join(COMP[c] for c in reversed(seq[beg + flen - rlen:beg + flen].upper()))
    return r1, r2


def sim_reads_text(contigs, flen=500, rlen=150, cv=15, ml=50000):
    """What the reference prints: HEADER:beg-end/1, read, HEADER:beg-end/2, read"""
    k = kept(contigs, ml)
    out = []
    for ci, beg in fragments(contigs, flen, rlen, cv, ml):
        h, s = k[ci]
        r1, r2 = mates(s, beg, flen, rlen)
        out += [f"{h}:{beg}-{beg + flen}/1", r1, f"{h}:{beg}-{beg + flen}/2", r2]
    return "".join(x + "\n" for x in out)


def parse_bed(text):
    """[(contig name, start, end, locus)]"""
    out = []
    for line in text.split("\n"):
        if line.strip():
            f = line.split("\t")
            out.append((f[0], int(f[1]), int(f[2]), int(f[3])))
    return out


def name_of(header):
    return header[1:].split(" ")[0].split("\t")[0]


def labels_of(bed, name, beg, flen):
    """the loci of the intervals of contig `name` that overlap [beg, beg + flen) by at least one base"""
    return sorted({l for c, s, e, l in bed if c == name and s < beg + flen and beg < e})


def src_of(bed, name, beg, flen, nloci):
    lab = labels_of(bed, name, beg, flen)
    return min(lab) if lab else nloci


def describe(contigs, bed, nloci, flen=500, rlen=150, cv=15, ml=50000):
    """(contig, beg, src) of every fragment, as dbtk_sim_describe answers"""
    k = kept(contigs, ml)
    fr = fragments(contigs, flen, rlen, cv, ml)
    return ([c for c, _ in fr], [b for _, b in fr], [src_of(bed, name_of(k[c][0]), b, flen, nloci) for c, b in fr])


def batch(contigs, bed, nloci, first, n, flen=500, rlen=150, cv=15, ml=50000):
    """The batch arrays dbtk_sim_batch makes for fragments first .. first + n - 1: (seq bytes, offsets, src); read 2p = /2, 2p + 1 = /1"""
    k = kept(contigs, ml)
    fr = fragments(contigs, flen, rlen, cv, ml)[first:first + n]
    reads = []
    for c, b in fr:
        r1, r2 = mates(k[c][1], b, flen, rlen)
        reads += [r2, r1]
    seq = np.frombuffer("".join(reads).encode(), np.uint8)
    off = np.arange(2 * len(fr) + 1, dtype=np.uint64) * np.uint64(rlen)
    src = np.array([src_of(bed, name_of(k[c][0]), b, flen, nloci) for c, b in fr], np.uint32)
    return seq, off, src


def annotated_fasta(contigs, bed, flen=500, rlen=150, cv=15, ml=50000):
    """The interleaved FASTA the reference's workflow hands to `danbing-tk -s 2`: titles >CTG:beg-end:LOCI/1 then /2, LOCI as
    distinct_sort_num prints them ('.' for none)"""
    k = kept(contigs, ml)
    out = []
    for ci, beg in fragments(contigs, flen, rlen, cv, ml):
        h, s = k[ci]
        r1, r2 = mates(s, beg, flen, rlen)
        lab = labels_of(bed, name_of(h), beg, flen)
        t = f"{h}:{beg}-{beg + flen}:{','.join(map(str, lab)) if lab else '.'}"
        out += [t + "/1", r1, t + "/2", r2]
    return "".join(x + "\n" for x in out)
