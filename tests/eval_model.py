"""A plain Python model of the genotype score (include/dbtk_eval.h): the truth counts and windows of an assembly's BED intervals, the
eight regression sums per locus with Python integers, the derived columns and the text of PREFIX.eval.tsv and PREFIX.pred.  Written
naively; test_eval_model.py pins its counts to the compiled fa2kmers."""
import sim_model

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
FIELDS = ("nk", "windows", "n1", "Sx", "Sy", "Sy1", "Sxy", "Sxx", "Syy", "Syy1")
TSV_HEADER = "#locus\tnk\tnk_present\twindows\tSx\tSy\tSy_present\tSxy\tSxx\tSyy\tSyy_present\tslope\tpred\tr2\tpred_present\tr2_present\n"
PRED_HEADER = "# TrueDosage\tPredDosage\tSlope\tr^2\n"


def canon(s, k):
    """canonical k-mer of the k bases s (upper-cased), None when one of them is not ACGT"""
    s = s.upper()
    assert len(s) == k
    if any(c not in CODE for c in s):
        return None
    fw = rc = 0
    for c in s:
        fw = fw << 2 | CODE[c]
    for c in reversed(s):
        rc = rc << 2 | (3 - CODE[c])
    return min(fw, rc)


def window_counts(contigs, bed, k, nloci, ml=1):
    """Per locus {canonical k-mer: windows}: every position p of a kept contig with START <= p and p + k <= min(END, size) for a BED
    line (name, START, END, locus) of that contig, whose k bases are all ACGTacgt; summed over the lines of a locus."""
    out = [dict() for _ in range(nloci)]
    for h, s in sim_model.kept(contigs, ml):
        name = sim_model.name_of(h)
        for c, st, en, l in bed:
            if c != name:
                continue
            for p in range(st, min(en, len(s)) - k + 1):
                km = canon(s[p:p + k], k)
                if km is not None:
                    out[l][km] = out[l].get(km, 0) + 1
    return out


def add_counts(a, b):
    return [{km: x.get(km, 0) + y.get(km, 0) for km in set(x) | set(y)} for x, y in zip(a, b)]


def truth(counts, slots, nk):
    """(truth[nk], windows[nloci]) from window_counts: slots[l] = {TR k-mer of locus l: its OUT.trkmc.ar position} (whether or not the
    k-mer is a flank k-mer of the locus as well); windows count every k-mer."""
    x = [0] * nk
    for l, d in enumerate(counts):
        for km, n in d.items():
            if km in slots[l]:
                x[slots[l][km]] += n
    return x, [sum(d.values()) for d in counts]


def sums(x, y, beg, windows=None):
    """per locus the dict of dbtk_eval_sums_t; beg[nloci + 1] = the loci's first positions; windows None: Sx"""
    out = []
    for l in range(len(beg) - 1):
        xs, ys = [int(v) for v in x[beg[l]:beg[l + 1]]], [int(v) for v in y[beg[l]:beg[l + 1]]]
        s = dict(nk=len(xs), n1=sum(1 for v in xs if v), Sx=sum(xs), Sy=sum(ys), Sy1=sum(b for a, b in zip(xs, ys) if a),
                 Sxy=sum(a * b for a, b in zip(xs, ys)), Sxx=sum(a * a for a in xs), Syy=sum(b * b for b in ys),
                 Syy1=sum(b * b for a, b in zip(xs, ys) if a))
        s["windows"] = s["Sx"] if windows is None else int(windows[l])
        out.append(s)
    return out


def fits64(s):
    return all(v < 1 << 64 for v in s.values())


def columns(s):
    """(slope, pred, r2, pred_present, r2_present) in double, by the formulas of the header; all 0 where Sxy == 0"""
    if s["Sxy"] == 0:
        return 0.0, 0.0, 0.0, 0.0, 0.0
    sxy, sxx = float(s["Sxy"]), float(s["Sxx"])
    slope = sxy / sxx
    return slope, float(s["Sy"]) / slope, (sxy * sxy) / (sxx * float(s["Syy"])), float(s["Sy1"]) / slope, (sxy * sxy) / (sxx * float(s["Syy1"]))


def tsv_text(all_sums):
    out = [TSV_HEADER]
    for l, s in enumerate(all_sums):
        c = columns(s)
        out.append("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.2f\t%.1f\t%.4f\t%.1f\t%.4f\n" % (
            l, s["nk"], s["n1"], s["windows"], s["Sx"], s["Sy"], s["Sy1"], s["Sxy"], s["Sxx"], s["Syy"], s["Syy1"], c[0], c[1], c[2], c[3], c[4]))
    return "".join(out)


def pred_text(all_sums):
    out = [PRED_HEADER]
    for s in all_sums:
        c = columns(s)
        out.append("%d\t%.1f\t%.2f\t%.4f\n" % (s["windows"], c[3], c[0], c[4]))
    return "".join(out)
