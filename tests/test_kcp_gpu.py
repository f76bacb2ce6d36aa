"""The bait k-mer count profile table on the GPU (include/dbtk_kcp.h, csrc/dbtk_kcp.hip) through the binding, against the Python model
that tests/test_kcp_model.py pins to the reference's baitBuilder: every entry's n, sum, sum of squares, min and max, exactly."""
import numpy as np
import pytest

import bind
import kcp_model

pkg, abi = bind.pkg, bind.abi
pytestmark = pytest.mark.gpu
NLOCI = 16


def rc(s: bytes) -> bytes:
    return s[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))


def rand_read(rng, n) -> bytes:
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)])


def pack(pairs):
    """[(mate, mate, src, dst)] -> seq, off, src, dst as Kcp.add takes them"""
    seqs = [m for p in pairs for m in p[:2]]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    seq = np.frombuffer(b"".join(seqs) + b"\0", np.uint8).copy()
    return seq, off, np.array([p[2] for p in pairs], np.uint32), np.array([p[3] for p in pairs], np.uint32)


def model_of(pairs, k, nloci=NLOCI, tp_only=False, tab=None):
    tab = {} if tab is None else tab
    for a, b, src, dst in pairs:
        kcp_model.add_pair(tab, (a.decode("latin1"), b.decode("latin1")), k, nloci, src, dst, tp_only)
    return tab


def check(kcp, tab):
    for cls in (0, 1):
        want = kcp_model.entries(tab, cls)
        got = kcp.read(cls)
        assert kcp.count(cls) == len(want)
        assert got == want, (cls, len(got), len(want), sorted(set(got.items()) ^ set(want.items()))[:4])


@pytest.fixture(scope="module")
def lib():
    return pkg.Dbtk()


def shapes(k):
    rng = np.random.default_rng(100 + k)
    r150 = rand_read(rng, 150)

    def with_byte(s, at, ch):
        return s[:at] + ch + s[at + 1:]
    pairs = [
        (b"A" * 150, b"", 0, 0),                                      # a homopolymer: one key, c = L - k + 1
        (b"AC" * 75, b"CA" * 60, 1, 1),                               # a dinucleotide repeat: two keys (AC.. and its reverse complement GT.. are one)
        (r150, rc(r150), 2, 2),                                       # a read and its reverse complement: the same keys, two observations
        (with_byte(r150, 0, b"N"), with_byte(r150, k - 1, b"N"), 3, 3),
        (with_byte(r150, 75, b"N"), with_byte(r150, 149, b"N"), 4, 4),
        (with_byte(r150, 40, b"g"), r150, 5, 5),                      # one lower-case base resets the window like an N
        (b"", rand_read(rng, k - 1), 6, 6),                           # nothing to count
        (rand_read(rng, k), rand_read(rng, 256), 7, 7),
        (r150, r150, 9, 8),                                           # a false positive: the same read twice, two observations of count 1
        (b"ACGT" * 64, b"T" * 256, 8, 8),                             # 256 bases of period 4 and of period 1
        (r150, r150, 3, NLOCI), (r150, r150, 3, NLOCI + 7),           # not assigned: skipped
    ]
    return pairs


@pytest.mark.parametrize("k", [21, 25, 31])
def test_multiplicity_shapes(lib, k):
    pairs = shapes(k)
    kcp = pkg.Kcp(lib, k, NLOCI)
    try:
        kcp.add(*pack(pairs))
        tab = model_of(pairs, k)
        check(kcp, tab)
        tp = kcp.read(0)
        homo = [v for (l, _), v in tp.items() if l == 0]
        c = 150 - k + 1
        assert homo == [(1, c, c * c, c, c)]
        di = [v for (l, _), v in tp.items() if l == 1]
        assert len(di) == 2 and all(v[0] == 2 for v in di) and sum(v[1] for v in di) == (150 - k + 1) + (120 - k + 1)
        assert all(v[0] == 2 for (l, _), v in tp.items() if l == 2) and sum(1 for (l, _) in tp if l == 2) == c
        assert not any(l in (6,) for (l, _) in tp) and sum(1 for (l, _) in tp if l == 7) == 1 + 256 - k + 1
        assert all(l == 8 and v[:2] == (2, 2) for (l, _), v in kcp.read(1).items())
        assert kcp.times()[1] == sum(len(set(kcp_model.canon_kmers(m.decode("latin1"), k))) for p in pairs if p[3] < NLOCI for m in p[:2])
    finally:
        kcp.close()


def test_contention_8192_identical_pairs_in_one_batch(lib):
    k = 21
    r = rand_read(np.random.default_rng(5), 150)
    one = [(r, rc(r), 3, 3)]
    kcp = pkg.Kcp(lib, k, NLOCI)
    try:
        kcp.add(*pack(one * 8192))
        want = {key: (n * 8192, s * 8192, q * 8192, mi, ma) for key, (n, s, q, mi, ma) in kcp_model.entries(model_of(one, k), 0).items()}
        got = kcp.read(0)
        assert got == want and kcp.count(1) == 0
        assert all(v[0] == 16384 for v in got.values())
    finally:
        kcp.close()


def test_growth_from_64_slots_over_uneven_batches(lib, monkeypatch, tmp_path):
    k = 25
    monkeypatch.setenv("DBTK_KCP_SLOTS", "64")
    kcp = pkg.Kcp(lib, k, NLOCI)
    monkeypatch.delenv("DBTK_KCP_SLOTS")
    try:
        assert kcp.stats()[1:] == (64, 0)
        rng = np.random.default_rng(77)
        pool = [rand_read(rng, 150) for _ in range(40)]  # reads come back: keys that exist already, beside new ones
        tab = {}
        for n in (1, 7, 300, 0, 50, 120, 33):
            pairs = []
            for _ in range(n):
                a = pool[int(rng.integers(0, len(pool)))] if rng.random() < 0.3 else rand_read(rng, int(rng.integers(k - 2, 257)))
                b = rand_read(rng, int(rng.integers(0, 200)))
                dst = int(rng.integers(0, NLOCI + 2))
                pairs.append((a, b, dst if rng.random() < 0.6 else int(rng.integers(0, NLOCI)), dst))
            kcp.add(*pack(pairs))
            model_of(pairs, k, tab=tab)
            nbytes, slots, occ = kcp.stats()
            assert occ == len(tab) and 2 * occ <= slots and nbytes == 40 * slots
        assert slots > 64 and kcp_model.entries(tab, 0) and kcp_model.entries(tab, 1)
        check(kcp, tab)
        kcp.write(str(tmp_path / "g"))
        assert open(tmp_path / "g.TP_pf.txt").read() == kcp_model.profile_text(tab, 0)
        assert open(tmp_path / "g.FP_pf.txt").read() == kcp_model.profile_text(tab, 1)
    finally:
        kcp.close()


def test_tp_only_reset_and_two_tables_alive_at_once(lib, tmp_path):
    k = 21
    rng = np.random.default_rng(9)
    pairs = [(rand_read(rng, 150), rand_read(rng, 100), int(rng.integers(0, 4)), int(rng.integers(0, 5))) for _ in range(60)]
    assert any(p[3] == 4 for p in pairs) and any(p[2] != p[3] for p in pairs)
    both, tp = pkg.Kcp(lib, k, 4), pkg.Kcp(lib, k, 4, tp_only=True)
    try:
        both.add(*pack(pairs[:30]))
        tp.add(*pack(pairs))
        both.add(*pack(pairs[30:]))
        check(both, model_of(pairs, k, nloci=4))
        check(tp, model_of(pairs, k, nloci=4, tp_only=True))
        assert tp.count(1) == 0 and tp.read(0) == both.read(0)
        tp.write(str(tmp_path / "t"))
        assert not (tmp_path / "t.FP_pf.txt").exists() and open(tmp_path / "t.TP_pf.txt").read() == kcp_model.profile_text(model_of(pairs, k, nloci=4), 0)
        slots = both.stats()[1]
        both.reset()
        assert both.count(0) == 0 and both.count(1) == 0 and both.stats()[1:] == (slots, 0) and both.times() == (0.0, 0)
        both.add(*pack(pairs[:5]))
        check(both, model_of(pairs[:5], k, nloci=4))
        check(tp, model_of(pairs, k, nloci=4, tp_only=True))
    finally:
        both.close()
        tp.close()


def test_a_read_longer_than_256_bases_is_refused_and_nothing_is_counted(lib):
    kcp = pkg.Kcp(lib, 21, 4)
    try:
        with pytest.raises(pkg.DbtkError) as e:
            kcp.add(*pack([(b"A" * 100, b"C" * 100, 1, 1), (b"A" * 257, b"C" * 10, 1, 1)]))
        assert e.value.status == abi.ERR_READ_TOO_LONG
        assert kcp.count(0) == 0
        kcp.add(*pack([(b"A" * 257, b"C" * 10, 1, 4)]))  # not assigned: its length does not matter
        assert kcp.count(0) == 0
    finally:
        kcp.close()
