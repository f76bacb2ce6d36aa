"""A plain Python model of the FP-specific bait k-mer filter (include/dbtk_kcp.h: dbtk_kcp_fps_*; the reference's baitBuilder v2 and
`ktools fps`) over kcp_model tables or over profile text.  The comparison runs on the floats that strtof makes of the "%.4f" text of
MEAN and SD: np.float32("%.4f" % x), with sd by the host's formula sqrt(float(num) / (float(n) * float(n))).
tests/test_fps_model.py pins it to `ktools fps`; the GPU tests compare the library and the command line with it."""
import math

import numpy as np

import kcp_model

TWO = np.float32(2)


def f32(x: float) -> np.float32:
    """the float `ktools fps` parses from the "%.4f" text of x"""
    return np.float32("%.4f" % x)


def text_floats(n: int, s: int, q: int):
    """(mean, sd) of an entry with these moments as float32: kcp_mean / kcp_sd (csrc/dbtk_kcp.h), printed and parsed"""
    return f32(float(s) / float(n)), f32(math.sqrt(float(n * q - s * s) / (float(n) * float(n))))


def stats_of(tab: dict, cls: int):
    """{(locus, kmer): (min, max, mean32, sd32)} of one class of a kcp_model table"""
    return {(l, km): (v[3], v[4]) + text_floats(v[0], v[1], v[2]) for (c, l, km), v in tab.items() if c == cls}


def stats_of_text(text: str):
    """the same from a profile file"""
    out, cur = {}, None
    for line in text.split("\n"):
        if not line:
            continue
        if line[0] == ">":
            cur = int(line[1:])
            continue
        km, mi, ma, mean, sd = line.split("\t")
        out[(cur, int(km))] = (int(mi), int(ma), np.float32(mean), np.float32(sd))
    return out


def inside(fp_mean, tp_mean, tp_sd) -> bool:
    w = TWO * tp_sd
    return bool(tp_mean - w <= fp_mean and fp_mean <= tp_mean + w)


def begin(fp_stats: dict):
    """the candidates: {(locus, kmer): [mean32, mi, ma]}, and the loci that have one"""
    return {key: [v[2], 255, 0] for key, v in fp_stats.items()}, sorted({l for l, _ in fp_stats})


def apply(cands: dict, tp_stats: dict):
    """One TP profile: a candidate it holds dies inside mean +- 2 sd, else takes (where mi is 255) or widens by its (min, max)."""
    for key in list(cands):
        t = tp_stats.get(key)
        if t is None:
            continue
        c = cands[key]
        if inside(c[0], t[2], t[3]):
            del cands[key]
        elif c[1] == 255:
            c[1], c[2] = t[0], t[1]
        else:
            c[1], c[2] = min(c[1], t[0]), max(c[2], t[1])


def fps(fp_stats: dict, tp_stats_list):
    """({(locus, kmer): (mi, ma)} of the survivors, the loci that had a candidate)"""
    cands, loci = begin(fp_stats)
    for t in tp_stats_list:
        apply(cands, t)
    return {key: (c[1], c[2]) for key, c in cands.items()}, loci


def fps_text(kept: dict, loci) -> str:
    """the file `ktools fps` writes: a header for every locus that had a candidate, the lines of a locus ascending by k-mer"""
    per = {l: [] for l in loci}
    for (l, km) in sorted(kept):
        per[l].append("%d\t%d\t%d\n" % ((km,) + tuple(kept[(l, km)])))
    return "".join(">%d\n%s" % (l, "".join(per[l])) for l in sorted(per))


def fates(fp_stats: dict, kept: dict):
    """(dropped, kept as 255 0, widened)"""
    plain = sum(1 for v in kept.values() if tuple(v) == (255, 0))
    return len(fp_stats) - len(kept), plain, len(kept) - plain


def table_of_counts(entries):
    """[(cls, locus, kmer, [c, ...])] -> a kcp_model table: the moments of the per-read counts listed"""
    tab = {}
    for cls, l, km, cs in entries:
        tab[(cls, l, km)] = [len(cs), sum(cs), sum(c * c for c in cs), min(cs), max(cs)]
    return tab


profile_text = kcp_model.profile_text
