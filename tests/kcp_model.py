"""A plain Python model of the bait k-mer count profiles (include/dbtk_kcp.h): kam lines or reads in, a dict
{(class, locus, canonical k-mer): [n, sum, sumsq, min, max]} out, and the profile files' text.  tests/test_kcp_model.py pins it to
files the reference's baitBuilder wrote; the GPU tests compare the library with it."""
import math
from collections import Counter

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def canon_kmers(seq: str, k: int):
    """The canonical k-mer of every window of upper-case ACGT (any other byte resets the window), one entry per such window."""
    out, fw, rc, run = [], 0, 0, 0
    mask = (1 << (2 * k)) - 1
    for ch in seq:
        c = CODE.get(ch)
        if c is None:
            run = 0
            continue
        fw = ((fw << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << (2 * (k - 1)))
        run += 1
        if run >= k:
            out.append(min(fw, rc))
    return out


def add_read(tab: dict, seq: str, k: int, locus: int, cls: int):
    """One observation per distinct k-mer of the read: its count c in this read."""
    for km, c in Counter(canon_kmers(seq, k)).items():
        e = tab.get((cls, locus, km))
        if e is None:
            tab[(cls, locus, km)] = [1, c, c * c, c, c]
        else:
            e[0] += 1; e[1] += c; e[2] += c * c; e[3] = min(e[3], c); e[4] = max(e[4], c)


def add_pair(tab, reads, k, nloci, src, dst, tp_only=False):
    if dst >= nloci:
        return
    cls = 0 if src == dst else 1
    if cls and tp_only:
        return
    for r in reads:
        add_read(tab, r, k, dst, cls)


def from_kam(lines, k, nloci, tp_only=False):
    """kam lines of `danbing-tk -s`: src dst ... title seq qual seq qual (the fields baitBuilder v1.pf reads: 0, 1, 11 and 13)."""
    tab = {}
    for line in lines:
        f = line.split()
        if len(f) < 15:
            continue
        add_pair(tab, (f[11], f[13]), k, nloci, int(f[0]), int(f[1]), tp_only)
    return tab


def profile_lines(tab, cls):
    """{locus: [line, ...]} of one class, the lines of a locus ascending by k-mer, as dbtk_kcp_write prints them."""
    out = {}
    for (c, locus, km) in sorted(tab):
        if c != cls:
            continue
        n, s, q, mi, ma = tab[(c, locus, km)]
        sd = math.sqrt((n * q - s * s) / (n * n))
        out.setdefault(locus, []).append("%d\t%d\t%d\t%.4f\t%.4f" % (km, mi, ma, s / n, sd))
    return out


def profile_text(tab, cls):
    return "".join(">%d\n%s\n" % (l, "\n".join(v)) for l, v in sorted(profile_lines(tab, cls).items()))


def parse_profile(text):
    """A profile or fps file -> ({locus: [line, ...]}, loci in file order)."""
    out, order, cur = {}, [], None
    for line in text.split("\n"):
        if not line:
            continue
        if line[0] == ">":
            cur = int(line[1:])
            order.append(cur)
            out.setdefault(cur, [])
        else:
            out[cur].append(line)
    return out, order


def entries(tab, cls):
    """{(locus, kmer): (n, sum, sumsq, min, max)} of one class: what Kcp.read returns."""
    return {(l, km): tuple(v) for (c, l, km), v in tab.items() if c == cls}
