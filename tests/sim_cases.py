"""The two-haplotype assembly case of the --sim tests: a 4-locus RPGG and, per haplotype, one contig that holds the loci between
random spacers, with a BED that gives true positives, false positives (mislabelled loci), pairs without a source ('.') that are
assigned all the same (a copy of locus 0 without a BED line) and fragments under two labels."""
import os

import numpy as np

import sim_model
import synth

K, NLOCI, CTH = 21, 4, 45
FLEN, RLEN, CV, ML = 500, 150, 15, 50000


class AsmCase:
    def __init__(self, d, ml=1):
        self.dir = d
        self.ml = ml
        self.loci = synth.make_loci(nloci=NLOCI, nhap=2, flank=500, seed=41)
        os.makedirs(os.path.join(d, "g"), exist_ok=True)
        self.pref = os.path.join(d, "g", "pan")
        synth.write_rpgg_files(synth.build_rpgg_arrays(self.loci, K), self.pref)
        rng = np.random.default_rng(43)
        self.contigs, self.beds, self.fa, self.bed = [], [], [], []
        for h in range(2):
            name = f"hap{h}"
            parts, bed, pos = [], [], 0

            def put(s):
                nonlocal pos
                parts.append(s)
                pos += len(s)

            def spacer():
                put(synth.BASES[rng.integers(0, 4, int(rng.integers(100, 701)))])
            for l in range(NLOCI):
                spacer()
                s = self.loci.haps[h][l]
                trs, tre = pos + self.loci.flank, pos + len(s) - self.loci.flank
                # haplotype 1 labels its even loci with the next locus' index: their pairs are false positives
                bed.append((name, trs, tre, (l + 1) % NLOCI if h == 1 and l % 2 == 0 else l))
                if l == 1:
                    bed.append((name, trs - 50, trs + 30, NLOCI - 1))  # a second label over the start of locus 1
                put(s)
            spacer()
            put(self.loci.haps[h][0])  # locus 0 once more, without a BED line: assigned pairs whose source is '.'
            spacer()
            seq = np.concatenate(parts).tobytes().decode()
            self.contigs.append([(">" + name + (" synthetic haplotype" if h else ""), seq)])
            self.beds.append(bed)
            fa, bd = os.path.join(d, f"{name}.fa"), os.path.join(d, f"{name}.bed")
            with open(fa, "w") as f:
                f.write(self.contigs[h][0][0] + "\n")
                f.write(seq + "\n" if h == 0 else "".join(seq[i:i + 70] + "\n" for i in range(0, len(seq), 70)))
            with open(bd, "w") as f:
                f.write("".join(f"{c}\t{s}\t{e}\t{l}\n" for c, s, e, l in bed))
            self.fa.append(fa)
            self.bed.append(bd)

    def batch(self):
        """The model's reads of both haplotypes in the order --sim tiles them: (seq, off, src) and the labels of every fragment"""
        seqs, srcs, labels = [], [], []
        for h in range(2):
            n = len(sim_model.fragments(self.contigs[h], FLEN, RLEN, CV, self.ml))
            s, _, src = sim_model.batch(self.contigs[h], self.beds[h], NLOCI, 0, n, FLEN, RLEN, CV, self.ml)
            seqs.append(s)
            srcs.append(src)
            for _, beg in sim_model.fragments(self.contigs[h], FLEN, RLEN, CV, self.ml):
                labels.append(sim_model.labels_of(self.beds[h], f"hap{h}", beg, FLEN))
        seq = np.concatenate(seqs)
        off = np.arange(len(seq) // RLEN + 1, dtype=np.uint64) * np.uint64(RLEN)
        return np.concatenate([seq, np.zeros(16, np.uint8)]), off, np.concatenate(srcs), labels

    def annotated_fasta(self, fn):
        with open(fn, "w") as f:
            for h in range(2):
                f.write(sim_model.annotated_fasta(self.contigs[h], self.beds[h], FLEN, RLEN, CV, self.ml))
        return fn
