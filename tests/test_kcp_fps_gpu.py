"""The FP-specific filter on the GPU (include/dbtk_kcp.h: dbtk_kcp_fps_*, dbtk_kcp_text_stats; csrc/dbtk_kcp.hip) through the binding,
against the Python model that tests/test_fps_model.py pins to `ktools fps`: the text-exact floats of MEAN and SD from the device, and
the survivors of the filter with their (mi, ma), exactly."""
import math

import numpy as np
import pytest

import bind
import fps_model
import kcp_model

pkg, abi = bind.pkg, bind.abi
pytestmark = pytest.mark.gpu
K, NLOCI = 21, 16


@pytest.fixture(scope="module")
def lib():
    return pkg.Dbtk()


@pytest.fixture()
def small_tables(monkeypatch):
    """every handle starts with 64 slots: the tables grow, and a walk that starts near the end wraps"""
    monkeypatch.setenv("DBTK_KCP_SLOTS", "64")


# ---- dbtk_kcp_text_stats: the device's `/`, sqrt and the rounding to four places against the host's printf and parse
def mirror(n, s, q):
    mean, sd = np.empty(len(n), np.float32), np.empty(len(n), np.float32)
    for i, (a, b, c) in enumerate(zip(n, s, q)):
        mean[i], sd[i] = fps_model.text_floats(a, b, c)
    return mean, sd


def same_bits(lib, n, s, q):
    gm, gs = pkg.kcp_text_stats(lib, n, s, q)
    wm, ws = mirror(n, s, q)
    bad = np.flatnonzero((gm.view(np.uint32) != wm.view(np.uint32)) | (gs.view(np.uint32) != ws.view(np.uint32)))
    assert len(bad) == 0, [(n[i], s[i], q[i], float(gm[i]), float(wm[i]), float(gs[i]), float(ws[i])) for i in bad[:5]]
    return gm, gs


def test_text_stats_every_small_mean_with_its_ties_and_the_near_ties(lib):
    n, s = zip(*[(a, b) for a in range(1, 129) for b in range(a, 4 * a + 1)])
    q = [4 * b for b in s]  # (counts 1 .. 4: sumsq <= 4 sum, and n * 4 sum >= sum^2 as sum <= 4 n)
    ties = sum(1 for a, b in zip(n, s) if (2 * b * 10000) % a == 0 and (2 * b * 10000 // a) % 2 == 1 and (a // math.gcd(a, b)) & (a // math.gcd(a, b) - 1) == 0)
    assert ties >= 100
    gm, _ = same_bits(lib, n, s, q)
    at = {(a, b): i for i, (a, b) in enumerate(zip(n, s))}
    assert gm[at[(32, 33)]] == np.float32("1.0312") and gm[at[(32, 35)]] == np.float32("1.0938") and gm[at[(96, 99)]] == np.float32("1.0312")
    # i / 20000, i odd: the decimal number ends in ...5, the double lies just beside it
    s2 = list(range(1, 80000, 2))
    same_bits(lib, [20000] * len(s2), s2, [4 * b + 5 for b in s2])


def test_text_stats_random_means_and_standard_deviations(lib):
    rng = np.random.default_rng(20251019)
    n = [int(x) for x in rng.integers(1, 1 << 31, 100000)]
    s = [a + int(rng.integers(0, 235 * a + 1)) for a in n]  # counts per read 1 .. 236
    same_bits(lib, n, s, [236 * b for b in s])
    # the moments of real counts; all counts equal (n * sumsq == sum^2: sd 0)
    n, s, q = [], [], []
    for _ in range(20000):
        cs = rng.integers(1, int(rng.integers(1, 237)) + 1, int(rng.integers(1, 300)))
        n.append(len(cs)); s.append(int(cs.sum())); q.append(int((cs * cs).sum()))
    for a in range(1, 300):
        for c in (1, 2, 7, 236):
            n.append(a); s.append(a * c); q.append(a * c * c)
    _, gs = same_bits(lib, n, s, q)
    assert (gs[20000:] == 0).all()
    # numerators above 2^64: two count values over 2^30 .. 2^31 reads; and moments that no reads give, with both words of the difference in play
    n, s, q, big = [], [], [], 0
    for _ in range(20000):
        a = int(rng.integers(1 << 30, 1 << 31))
        x, c0 = int(rng.integers(0, a)), int(rng.integers(1, 101))
        c1 = c0 + int(rng.integers(1, 137))
        n.append(a); s.append(x * c0 + (a - x) * c1); q.append(x * c0 * c0 + (a - x) * c1 * c1)
    for _ in range(20000):
        a = int(rng.integers(1, 1 << 32))
        b = int(rng.integers(0, 1000 * a + 1))  # a mean of 1000 at the most, sd^2 < 2 * 10^6 + 1: the digits of both stay below 2^24
        n.append(a); s.append(b); q.append(-(-b * b // a) + int(rng.integers(0, a * 2000000)))
    big = sum(1 for a, b, c in zip(n, s, q) if (a * c - b * b) >> 64)
    assert big > 10000
    same_bits(lib, n, s, q)


# ---- the filter.  Per-read counts are chosen through reads of one k-mer: a homopolymer or the dinucleotides AT / CG of k + c - 1 bases
# hold one canonical k-mer c times.  (locus, key) names an entry; the lists are its per-read counts in the FP class of the first
# handle, the TP class of the first handle and the TP class of a second handle.
def one_kmer_read(key: str, c: int) -> bytes:
    return (key * 300)[:K + c - 1].encode()


SPECS = [
    (0, "A", [3], None, None),                                  # no TP table holds it: kept 255 0 (the k-mer is a TP entry of other loci)
    (1, "A", [4], [1, 3], None),                                # TP mean 2, sd 1: 4 == mean + 2 sd, dropped
    (2, "A", [1], [2, 4, 2, 4], None),                          # TP mean 3, sd 1: 1 == mean - 2 sd, dropped
    (3, "A", [2], [2, 2], None),                                # sd 0, equal means: dropped
    (4, "A", [3], [2, 2], None),                                # sd 0, other mean: widened to 2 2
    (5, "A", [1] * 31 + [2], None, [1] * 62 + [2] * 2),         # n = 32, sum = 33: 1.03125 prints 1.0312; inside 1.0312 +- 2 * 0.1740
    (6, "A", [1] * 15 + [2] * 17, [2] * 8 + [3] * 9, None),     # 1.53125 prints 1.5312 (1.5313 would be inside 2.5294 - 2 * 0.4991): widened to 2 3
    (7, "A", [1] * 9 + [2] * 23, [2] * 41 + [3], None),         # 1.71875 prints 1.7188 (1.7187 would be outside 2.0238 - 2 * 0.1525): dropped
    (8, "A", [5], [1, 2], [7, 9]),                              # outside both: 1 2, then 1 9 (or 7 9, then 1 9)
    (9, "A", [2], [2, 2], [7, 9]),                              # dropped by the first table; the second would widen it
    (10, "A", [2], [7, 9], [2, 2]),                             # dropped by the second; the first would widen it
    (11, "C", [3], None, [1]),                                  # the second table alone: 1 1
    (12, "AT", [4], [1, 1, 2], None),
    (13, "CG", [6, 6], [2], [3, 4]),
    (13, "A", [7], [7], [1]),                                   # dropped by the first
    (14, "C", [2, 3], [9], [8]),                                # 8 9
    (15, "AT", [236], None, None),
]


def pairs_of(specs, column):
    """column 0: the FP reads (titled with the next locus), 1 / 2: the TP reads of the first / second handle"""
    out = []
    for spec in specs:
        l, key, cs = spec[0], spec[1], spec[2 + column]
        for c in cs or []:
            out.append((one_kmer_read(key, c), b"", (l + 1) % NLOCI if column == 0 else l, l))
    return out


def pack(pairs):
    seqs = [m for p in pairs for m in p[:2]]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    seq = np.frombuffer(b"".join(seqs) + b"\0", np.uint8).copy()
    return seq, off, np.array([p[2] for p in pairs], np.uint32), np.array([p[3] for p in pairs], np.uint32)


def model_of(pairs, tp_only=False):
    tab = {}
    for a, b, src, dst in pairs:
        kcp_model.add_pair(tab, (a.decode(), b.decode()), K, NLOCI, src, dst, tp_only)
    return tab


def filled(lib, pairs, tp_only=False, k=K, nloci=NLOCI):
    h = pkg.Kcp(lib, k, nloci, tp_only=tp_only)
    if pairs:
        h.add(*pack(pairs))
    return h


def test_chosen_moments_two_tables_in_both_orders(lib, small_tables, tmp_path):
    first, second = pairs_of(SPECS, 0) + pairs_of(SPECS, 1), pairs_of(SPECS, 2)
    m0, m1 = model_of(first), model_of(second, tp_only=True)
    fp_stats, t0, t1 = fps_model.stats_of(m0, 1), fps_model.stats_of(m0, 0), fps_model.stats_of(m1, 0)
    assert len(fp_stats) == len(SPECS)
    # the model's verdicts on the cases, before the device is asked
    want, loci = fps_model.fps(fp_stats, [t0, t1])
    key = {(l, k): km for (l, km) in fp_stats for k in ("A", "C", "AT", "CG") if kcp_model.canon_kmers(one_kmer_read(k, 1).decode(), K) == [km]}
    verdict = {(l, k): want.get((l, km)) for (l, k), km in key.items()}
    assert verdict == {(0, "A"): (255, 0), (1, "A"): None, (2, "A"): None, (3, "A"): None, (4, "A"): (2, 2), (5, "A"): None, (6, "A"): (2, 3), (7, "A"): None, (8, "A"): (1, 9),
                       (9, "A"): None, (10, "A"): None, (11, "C"): (1, 1), (12, "AT"): (1, 2), (13, "CG"): (2, 4), (13, "A"): None, (14, "C"): (8, 9), (15, "AT"): (255, 0)}
    assert fp_stats[(5, key[(5, "A")])][2] == np.float32("1.0312") and fp_stats[(6, key[(6, "A")])][2] == np.float32("1.5312")
    assert fps_model.inside(np.float32("1.5313"), *t0[(6, key[(6, "A")])][2:]) and not fps_model.inside(np.float32("1.7187"), *t0[(7, key[(7, "A")])][2:]), \
        "the two ties decide: rounded the other way, locus 6 would be dropped and locus 7 kept"
    h0, h1 = filled(lib, first), filled(lib, second, tp_only=True)
    a = b = None
    try:
        assert h0.stats()[1] > 64, "the table has grown"
        a, b = pkg.KcpFps(h0), pkg.KcpFps(h0)
        assert a.count() == (len(SPECS), len(SPECS)) and a.read() == {k: (255, 0) for k in fp_stats}
        a.apply(h0)
        after0, _ = fps_model.fps(fp_stats, [t0])
        assert a.read() == after0 and a.count() == (len(SPECS), len(after0)) and a.times()[1] == len(SPECS)
        a.apply(h1)
        b.apply(h1)
        after1, _ = fps_model.fps(fp_stats, [t1])
        assert b.read() == after1
        b.apply(h0)
        assert a.read() == b.read() == want and a.count() == b.count() == (len(SPECS), len(want))
        assert a.times()[1] == len(SPECS) + len(after0) and b.times()[1] == len(SPECS) + len(after1) and a.times()[0] > 0
        assert (9, key[(9, "A")]) not in want and (10, key[(10, "A")]) not in want, "a dropped candidate stays dropped"
        a.apply(h1)
        a.apply(h0)
        assert a.read() == want, "applying a table again changes nothing"
        # the list lives on its own: the handles are reset and freed, the file is written afterwards
        h0.reset()
        h1.close()
        a.write(str(tmp_path / "fps.txt"))
        assert open(tmp_path / "fps.txt").read() == fps_model.fps_text(want, loci)
        assert ">1\n>2\n>3\n>4\n" in open(tmp_path / "fps.txt").read(), "the header of a locus whose candidates all died"
    finally:
        for x in (a, b):
            if x:
                x.close()
        h0.close()
        h1.close()


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65])
def test_candidate_counts_around_a_wave(lib, small_tables, m):
    """m candidates with count 1 from one random read; the first half dropped by a TP table that holds them with count 1, three
    widened by a second TP table that holds them with count 2 (the read's piece twice in one read, an N between), the rest in no table."""
    rng = np.random.default_rng(300 + m)
    r = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, K + 65)])
    fp = [(r[:K + m - 1], b"", 1, 0)] if m else []
    half = r[:K + m // 2 - 1] if m // 2 else b""
    piece = r[m // 2:m // 2 + K + 2] if m >= m // 2 + 3 else b""
    tp0, tp1 = [(half, half, 0, 0), (r[:K + 20], b"", 5, 5)], [(piece + b"N" + piece, b"", 0, 0)]
    mf, m0, m1 = model_of(fp + tp0[1:]), model_of(tp0), model_of(tp1)
    fp_stats = fps_model.stats_of(mf, 1)
    assert len(fp_stats) == m
    want, loci = fps_model.fps(fp_stats, [fps_model.stats_of(x, 0) for x in (mf, m0, m1)])
    assert len(want) == m - m // 2 and sum(1 for v in want.values() if v == (2, 2)) == (3 if piece else 0)
    hf, h0, h1 = filled(lib, fp + tp0[1:]), filled(lib, tp0, tp_only=True), filled(lib, tp1, tp_only=True)
    f = None
    try:
        f = pkg.KcpFps(hf)
        assert f.count() == (m, m)
        for h in (hf, h1, h0):
            f.apply(h)
        assert f.read() == want and f.count() == (m, len(want))
    finally:
        if f:
            f.close()
        for h in (hf, h0, h1):
            h.close()


def test_a_table_without_tp_entries_and_an_empty_table_change_nothing(lib, small_tables):
    fp = pairs_of(SPECS, 0)
    hf, empty = filled(lib, fp), filled(lib, [])
    f = None
    try:
        assert hf.count(0) == 0 and hf.count(1) == len(SPECS)
        f = pkg.KcpFps(hf)
        f.apply(hf)
        f.apply(empty)
        assert f.count() == (len(SPECS), len(SPECS)) and set(f.read().values()) == {(255, 0)}
        assert f.times()[1] == 2 * len(SPECS)
    finally:
        if f:
            f.close()
        hf.close()
        empty.close()


def test_more_candidates_than_one_pass_of_the_grid(lib):
    """2 300 random 256-base reads: 542 800 candidates.  The apply kernel is launched with at most 8 blocks of 256 lanes per compute
    unit — 524 288 lanes on the 256 compute units of an MI355X — so the grid-stride loop takes a second step for the last 18 512.
    Read i is dropped whole (i % 3 == 0: the TP table holds the read itself), widened to 2 2 over the k-mers of its first 127 bases
    (i % 3 == 1: the TP read is that piece twice, an N between) or in no table.  (Seed 9: no k-mer occurs twice at a locus, which
    the count of the expected survivors asserts.)"""
    rng = np.random.default_rng(9)
    reads = [bytes(x) for x in np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (2300, 256))]]
    fp = [(r, b"", (i + 1) % NLOCI, i % NLOCI) for i, r in enumerate(reads)]
    tp = [(r, b"", i % NLOCI, i % NLOCI) if i % 3 == 0 else (r[:127] + b"N" + r[:127], b"", i % NLOCI, i % NLOCI) for i, r in enumerate(reads) if i % 3 != 2]
    want = {}
    for i, r in enumerate(reads):
        if i % 3 == 0:
            continue
        twice = set(kcp_model.canon_kmers(r[:127].decode(), K)) if i % 3 == 1 else set()
        for km in kcp_model.canon_kmers(r.decode(), K):
            want[(i % NLOCI, km)] = (2, 2) if km in twice else (255, 0)
    ncand = 2300 * 236
    assert len(want) == ncand - 767 * 236 and ncand > 256 * 8 * 256
    hf, ht = filled(lib, fp), filled(lib, tp, tp_only=True)
    f = None
    try:
        f = pkg.KcpFps(hf)
        assert f.count() == (ncand, ncand)
        f.apply(ht)
        assert f.count() == (ncand, len(want)) and f.times()[1] == ncand
        assert f.read() == want
    finally:
        if f:
            f.close()
        hf.close()
        ht.close()


def test_refusals(lib):
    """A TP-only handle has no candidates to give; a table of another k or another number of loci is not the candidates'.  (A table
    on another device is refused by the same comparison; it is tried where the machine has a second device.)"""
    import torch
    fp = pairs_of(SPECS, 0)
    tp_only, hf, other_k, other_n = filled(lib, fp, tp_only=True), filled(lib, fp), filled(lib, [], k=25), filled(lib, [], nloci=NLOCI + 1)
    f = far = None
    try:
        with pytest.raises(pkg.DbtkError) as e:
            pkg.KcpFps(tp_only)
        assert e.value.status == abi.ERR_ARG and "DBTK_KCP_TP_ONLY" in str(e.value)
        f = pkg.KcpFps(hf)
        for h in (other_k, other_n):
            with pytest.raises(pkg.DbtkError) as e:
                f.apply(h)
            assert e.value.status == abi.ERR_ARG and "does not match" in str(e.value)
        if torch.cuda.device_count() > 1:
            far = pkg.Kcp(lib, K, NLOCI, device=1)
            with pytest.raises(pkg.DbtkError) as e:
                f.apply(far)
            assert e.value.status == abi.ERR_ARG and "does not match" in str(e.value)
        # the filter of a handle moves between batches: TP-only from here on, what it holds stays
        hf.set_tp_only(True)
        hf.add(*pack(fp + pairs_of(SPECS, 1)))
        assert hf.count(1) == len(SPECS) and hf.count(0) == sum(1 for s in SPECS if s[3])
        with pytest.raises(pkg.DbtkError):
            pkg.KcpFps(hf)
        hf.set_tp_only(False)
        f.apply(hf)
        assert f.read() == fps_model.fps(fps_model.stats_of(model_of(fp), 1), [fps_model.stats_of(model_of(pairs_of(SPECS, 1)), 0)])[0]
    finally:
        for x in (f, far, tp_only, hf, other_k, other_n):
            if x:
                x.close()
