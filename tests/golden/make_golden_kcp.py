#!/usr/bin/env python3
"""Makes tests/golden/kcp/: a hand-made kam file and what the reference's baitBuilder makes of it.

    python tests/golden/make_golden_kcp.py REFERENCE_SRC_DIR

REFERENCE_SRC_DIR holds the reference's bait.cpp (and kmer.hpp).  It is compiled into a temporary directory outside the repository;
only data goes into tests/golden/kcp/:
    in.kam           120 kam lines (danbing-tk -s): 3 loci, reads cut from short motifs with about 1 % substitutions, some N and
                     lower-case bases, lengths 20 / 21 / 100 / 150 / 256, a third of the pairs with src != dst or dst == nloci
    ref.TP_pf.txt    baitBuilder v1.pf in.kam 3 21 ref
    ref.FP_pf.txt
    tp.TP_pf.txt     baitBuilder v1.pf in.kam 3 21 tp -tp
    ref.fps.txt      baitBuilder v2 3 21 ref.fps.txt ref.FP_pf.txt ref.TP_pf.txt tp.TP_pf.txt
The tests need none of this script: they read the files."""
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "kcp")
K, NLOCI, NLINES = 21, 3, 120
MOTIFS = ["ACGTTGCAGT", "AAAG", "CAGCAGCAT"]
LENGTHS = [20, 21, 100, 150, 256]
MARKERS = ["GATTACAGGCTTAACCGTATCGGATCCTAG", "TCGGCATTAGCCATGCAAGTCTGACGTTAC", "CCATAGGTCAAGTCTGGATACGCTTAGACG"]


def cut(rng, motif, length):
    s = (motif * (length // len(motif) + 3))
    at = rng.randrange(len(motif))
    r = list(s[at:at + length])
    for i in range(length):
        if rng.random() < 0.01:
            r[i] = rng.choice("ACGT")
    return r


def make_kam():
    rng = random.Random(20250921)
    lines = []
    for i in range(NLINES):
        dst = i % NLOCI
        kind = i % 10  # 0-5: true positive; 6, 7, 8: false positive; 9: not assigned
        if kind < 6:
            src, motif_of = dst, [dst, dst]
        elif kind == 6:
            src, motif_of = (dst + 1) % NLOCI, [dst, (dst + 1) % NLOCI]      # one mate looks like the locus it went to
        elif kind == 7:
            src, motif_of = (dst + 2) % NLOCI, [(dst + 2) % NLOCI] * 2
        elif kind == 8:
            src, motif_of = (dst + 1) % NLOCI, [dst, dst]
        else:
            src, dst, motif_of = dst, NLOCI, [dst, dst]
        reads = []
        for m in range(2):
            r = cut(rng, MOTIFS[motif_of[m]], LENGTHS[(i // 3 + 2 * m) % len(LENGTHS)])
            # the locus' marker once in some true positives and twice in some false positives: k-mers whose FP mean (2) lies outside
            # the TP profile's mean +- 2 sd (1 +- 0), the ones baitBuilder v2 keeps with the TP profile's min / max
            if kind == 0 and len(r) >= 100:
                r[40:70] = MARKERS[dst]
            if kind == 8 and len(r) >= 100:
                r[10:40] = MARKERS[dst]
                r[50:80] = MARKERS[dst]
            if i % 7 == 3 and len(r) > 40:
                r[rng.randrange(len(r))] = "N"
            if i % 11 == 5 and len(r) > 40:
                j = rng.randrange(len(r))
                r[j] = r[j].lower()
            if i % 13 == 6 and len(r) > 40:
                r[0] = "N"
            reads.append("".join(r))
        # src dst dst0 n2 n1 names mate2 mate1 annot2 annot1 title seq2 qual2 seq1 qual1 (the fields baitBuilder skips are placeholders)
        lines.append("\t".join([str(src), str(dst), "-1", "0", "0", "kf:hf", "0:0", "0:0", "*", "*", f"{src}.r{i}", reads[0], ".", reads[1], "."]))
    return "\n".join(lines) + "\n"


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "bait.cpp")):
        sys.exit(__doc__)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "in.kam"), "w") as f:
        f.write(make_kam())
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "baitBuilder")
        subprocess.run(["g++", "-std=c++11", "-O2", "-o", exe, os.path.join(sys.argv[1], "bait.cpp")], check=True)
        run = lambda *a: subprocess.run([exe, *a], check=True, cwd=OUT, stderr=subprocess.DEVNULL)
        run("v1.pf", "in.kam", str(NLOCI), str(K), "ref")
        run("v1.pf", "in.kam", str(NLOCI), str(K), "tp", "-tp")
        run("v2", str(NLOCI), str(K), "ref.fps.txt", "ref.FP_pf.txt", "ref.TP_pf.txt", "tp.TP_pf.txt")
    for fn in sorted(os.listdir(OUT)):
        print(fn, os.path.getsize(os.path.join(OUT, fn)))


if __name__ == "__main__":
    main()
