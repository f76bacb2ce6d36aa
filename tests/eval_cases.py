"""The cases of the --eval tests: a 16-locus RPGG with two assemblies whose BED intervals hold every edge the truth pass has
(TruthCase), and an RPGG whose loci have the sizes at which the sums pass changes its path (sized_rpgg)."""
import os

import numpy as np

import eval_model
import sim_model
import synth

NLOCI = 16
FLANK = 60
FLEN, RLEN, CV = 500, 150, 15


def _s(a):
    return a.tobytes().decode()


class TruthCase:
    """Loci 0..15 (two haplotypes each; TR = the haplotype without its flanks) and two assemblies.  Assembly 0, contig cA:
      locus 0   its TR at position 0 of the contig (an interval that starts at 0)
      locus 1   an interval of k - 1 bases (no window)             locus 2   one of exactly k bases (one window)
      locus 3   its TR with N, n and lower-case bases inside
      loci 4, 5 intervals that overlap by 2 k bases; the TR of 5 begins with the last 40 bases of the TR of 4 (shared TR k-mers)
      locus 6   two lines: both haplotypes' TRs                    locus 7   an interval that begins 30 bases inside its left flank
      locus 8   an interval over the TR of locus 9 (TR k-mers of another locus only)
      locus 10  an interval over a random spacer (k-mers in no table)
      locus 11  3 000 bases of a pure 7-base tandem repeat (three work items; a whole wave adds to one counter)
      locus 12  (ACGT)^12: at even k every window is its own reverse complement
      locus 13  its TR as the contig's last bases (an interval that ends at the last base)
    contigs cB, cC, cD: the TRs of loci 14, 15, 9; on cB the END of locus 14 lies 37 bases past the contig (clipped).
    Assembly 1, contigs dA and dB: the second haplotypes of loci 0, 6, 11 and 3, 12."""

    def __init__(self, k=21, seed=7):
        self.k = k
        rng = np.random.default_rng(seed)
        loci = synth.make_loci(nloci=NLOCI, nhap=2, flank=FLANK, tr_min=60, tr_max=300, seed=seed)
        fl = FLANK

        def tr(h, l):
            return loci.haps[h][l][fl:len(loci.haps[h][l]) - fl]

        def set_tr(h, l, t):
            s = loci.haps[h][l]
            loci.haps[h][l] = np.concatenate([s[:fl], t, s[len(s) - fl:]])
        for h in range(2):
            set_tr(h, 5, np.concatenate([tr(h, 4)[-40:], tr(h, 5)]))
            set_tr(h, 11, np.tile(np.frombuffer(b"ACCTGAT", np.uint8), 429 - 20 * h)[:3000 - 140 * h])
            set_tr(h, 12, np.concatenate([np.tile(np.frombuffer(b"ACGT", np.uint8), 12), tr(h, 12)]))
        self.loci = loci
        self.arrays = synth.build_rpgg_arrays(loci, k)

        def spacer(n=None):
            return _s(synth.BASES[rng.integers(0, 4, int(n or rng.integers(30, 90)))])
        contigs, bed = [], []

        class Ctg:
            def __init__(s, name):
                s.name, s.parts, s.pos = name, [], 0

            def put(s, text):
                s.parts.append(text)
                s.pos += len(text)
                return s.pos - len(text)

            def iv(s, text, locus, lead=0, tail=0):
                at = s.put(text)
                bed.append((s.name, at + lead, s.pos + tail, locus))

            def done(s, desc=""):
                contigs.append((">" + s.name + desc, "".join(s.parts)))
        c = Ctg("cA")
        c.iv(_s(tr(0, 0)), 0)
        c.put(spacer())
        c.iv(_s(tr(0, 1))[:k - 1], 1)
        c.put(spacer())
        c.iv(_s(tr(0, 2))[:k], 2)
        c.put(spacer())
        t3 = list(_s(tr(0, 3)))
        t3[10], t3[11], t3[30] = "N", "n", "n"
        for i in (0, 5, 40, 41, 42, len(t3) - 1):
            t3[i] = t3[i].lower()
        c.iv("".join(t3), 3)
        c.put(spacer())
        a4 = c.put(_s(tr(0, 4)))
        e4 = c.pos
        c.put(_s(tr(0, 5))[40:])   # (the TR of 5 begins with the last 40 bases of the TR of 4: they lie there already)
        bed.append(("cA", a4, min(e4 + 2 * k - 40, c.pos), 4))
        bed.append(("cA", e4 - 40, c.pos, 5))
        c.put(spacer())
        c.iv(_s(tr(0, 6)), 6)
        c.put(spacer())
        c.iv(_s(tr(1, 6)), 6)
        c.put(spacer())
        c.iv(_s(loci.haps[0][7][:len(loci.haps[0][7]) - fl]), 7, lead=30)
        c.put(spacer())
        c.iv(_s(tr(0, 9)), 8)
        c.put(spacer())
        c.iv(spacer(120), 10)
        c.put(spacer())
        c.iv(_s(tr(0, 11)), 11)
        c.put(spacer())
        c.iv(_s(tr(0, 12)), 12)
        c.put(spacer())
        c.iv(_s(tr(0, 13)), 13)
        c.done(" first assembly")
        for name, l in (("cB", 14), ("cC", 15), ("cD", 9)):
            c = Ctg(name)
            c.put(spacer(2000))
            c.iv(_s(tr(0, l)), l, tail=37 if l == 14 else 0)
            if l != 14:
                c.put(spacer(10))
            c.done()
        self.contigs, self.beds = [contigs], [bed]
        contigs, bed = [], []
        c = Ctg("dA")
        c.put(spacer())
        for l in (0, 6, 11):
            c.iv(_s(tr(1, l)), l)
            c.put(spacer())
        c.done()
        c = Ctg("dB")
        c.put(spacer(600))
        for l in (3, 12):
            c.iv(_s(tr(1, l)).lower() if l == 3 else _s(tr(1, l)), l)
            c.put(spacer())
        c.done()
        self.contigs.append(contigs)
        self.beds.append(bed)
        self.arena = len(self.contigs[0][0][1])  # DBTK_SIM_ARENA_BYTES for [cA] [cB cC] [cD]
        n = [len(s) for _, s in self.contigs[0]]
        assert n[1] + n[2] <= self.arena < n[1] + n[2] + n[3] and sum(len(s) for _, s in self.contigs[1]) <= self.arena
        assert sum(len(s) for _, s in self.contigs[0] + self.contigs[1]) < 100000

    def write(self, d):
        """(FASTA, BED) per assembly"""
        out = []
        for a in range(2):
            fa, bd = os.path.join(d, f"asm{a}.fa"), os.path.join(d, f"asm{a}.bed")
            with open(fa, "w") as f:
                for h, s in self.contigs[a]:
                    f.write(h + "\n" + "".join(s[i:i + 80] + "\n" for i in range(0, len(s), 80)))
            with open(bd, "w") as f:
                f.write("".join(f"{c}\t{s}\t{e}\t{l}\n" for c, s, e, l in self.beds[a]))
            out.append((fa, bd))
        return out

    def window_counts(self, asms=(0, 1)):
        w = [dict() for _ in range(NLOCI)]
        for a in asms:
            w = eval_model.add_counts(w, eval_model.window_counts(self.contigs[a], self.beds[a], self.k, NLOCI))
        return w


def order_of(g):
    """(slots, flank, beg) of an RPGG handle: slots[l] = {TR k-mer: OUT.trkmc.ar position}, flank[l] = set of flank k-mers, beg[nloci + 1]"""
    v = g.view()
    order = g.output_order()
    slots, flank, beg = [], [], [0]
    i = j = 0
    for l in range(g.nloci):
        n, m = int(v.tr_cnt[l]), int(v.fl_cnt[l])
        slots.append({int(v.tr_ks[i + q]): int(order[i + q]) for q in range(n)})
        flank.append({int(v.fl_ks[j + q]) for q in range(m)})
        i += n
        j += m
        beg.append(beg[-1] + n)
    for l in range(g.nloci):  # (the counters of a locus are contiguous)
        assert sorted(slots[l].values()) == list(range(beg[l], beg[l + 1]))
    return slots, flank, beg


SIZES = [0, 1, 63, 64, 65, 5000, 511, 512, 513, 7, 0, 1300]  # the wave / workgroup split lies at 512 k-mers


def sized_rpgg(lib, k=21, sizes=SIZES, seed=3):
    """An RPGG whose locus l has sizes[l] TR k-mers (distinct random canonical k-mers, each unique to its locus) and no flank k-mers"""
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    ks = set()
    while len(ks) < n:
        for v in rng.integers(0, 1 << (2 * k - 2), n - len(ks), dtype=np.uint64):
            s = "".join("ACGT"[(int(v) >> (2 * (k - 1 - i))) & 3] for i in range(k))
            ks.add(eval_model.canon(s, k))
    ks = np.array(sorted(ks), np.uint64)
    rng.shuffle(ks)
    loc = np.concatenate([np.full(m, l, np.uint32) for l, m in enumerate(sizes)])
    return lib.from_arrays(k, ks, loc << np.uint32(1), np.zeros(0, np.uint32), np.zeros(len(sizes), np.uint64), np.zeros(0, np.uint64), np.array(sizes, np.uint64), ks)
