"""The simulated read source on the GPU (include/dbtk_sim.h, csrc/dbtk_sim.hip) at library level: what k_sim_tile writes — reads,
offsets, source loci — copied back and compared byte for byte with the model of tests/sim_model.py (which test_sim_host.py pins
to the compiled sim_reads), and the batches through the hot path against dbtk_align_batch over the model's reads."""
import ctypes as C
import random

import numpy as np
import pytest

import bind
import sim_cases
import sim_model
from test_sim_host import bed_text, fasta_text

pkg, abi = bind.pkg, bind.abi
pytestmark = pytest.mark.gpu
NLOCI = 7


@pytest.fixture(scope="module")
def lib():
    return pkg.Dbtk()


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return h


def d2h(hip, ptr, n, dtype):
    out = np.empty(n, dtype)
    if n:
        assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), ptr, out.nbytes, 2) == 0
    return out


def contigs_of(sizes, seed, marks=()):
    """random contigs; lower-case letters and N anywhere, at the first and last base of every contig, and at the positions `marks`
    (the first and last base of both mates of the fragment at 0), alternately"""
    rng = random.Random(seed)
    out = []
    for i, n in enumerate(sizes):
        s = [rng.choice("ACGT") for _ in range(n)]
        for j in range(n):
            x = rng.random()
            if x < 0.06:
                s[j] = s[j].lower()
            elif x < 0.09:
                s[j] = rng.choice("Nn")
        for j, m in enumerate(marks):
            if m < n:
                s[m] = "Nn"[(i + j) % 2] if (i + j) % 3 else s[m].lower()
        if n:
            s[0], s[-1] = ("n", "c") if i % 2 else ("g", "N")
        out.append((f">c{i} d" if i % 2 else f">c{i}", "".join(s)))
    return out


def bed_of(contigs, flen, seed):
    """a few intervals per contig: short, long, overlapping, at position 0 and at the end"""
    rng = random.Random(seed)
    bed = []
    for h, s in contigs:
        n = len(s)
        if n < 4:
            continue
        name = sim_model.name_of(h)
        for _ in range(rng.randrange(0, 4)):
            a = rng.randrange(0, n - 1)
            bed.append((name, a, min(n, a + 1 + rng.randrange(0, max(2, flen))), rng.randrange(0, NLOCI)))
        if rng.random() < 0.3:
            bed.append((name, 0, 1, rng.randrange(0, NLOCI)))
        if rng.random() < 0.3:
            bed.append((name, n - 1, n, rng.randrange(0, NLOCI)))
    return bed


def check_batches(lib, hip, tmp_path, contigs, bed, flen, rlen, cv, ml, batch_sizes, groups=None, monkeypatch=None):
    fa, bd = tmp_path / "a.fa", tmp_path / "a.bed"
    fa.write_text(fasta_text(contigs))
    bd.write_text(bed_text(bed))
    s = pkg.Sim(lib, str(fa), str(bd), NLOCI, flen, rlen, cv, ml)
    try:
        s.attach(0)
        nfr = int(s.info().nfrags)
        assert nfr == len(sim_model.fragments(contigs, flen, rlen, cv, ml)) and nfr > 0
        if groups is not None:
            assert s.info().ngroups == groups
        wseq, woff, wsrc = sim_model.batch(contigs, bed, NLOCI, 0, nfr, flen, rlen, cv, ml)
        for bs in batch_sizes:
            bs = nfr if bs is None else bs
            for first in range(0, nfr, bs):
                n = min(bs, nfr - first)
                d_seq, d_off, d_src = s.batch(first, n)
                s.wait()
                assert d_seq % 16 == 0
                nb = 2 * n * rlen
                pad = (nb + 15) // 16 * 16
                got = d2h(hip, d_seq, pad, np.uint8)
                where = (flen, rlen, cv, bs, first)
                assert got[:nb].tobytes() == wseq[2 * first * rlen:2 * (first + n) * rlen].tobytes(), where
                assert not got[nb:].any(), where  # the tail up to the multiple of 16 is zeroed
                assert (d2h(hip, d_off, 2 * n + 1, np.uint64) == woff[:2 * n + 1]).all(), where
                assert (d2h(hip, d_src, n, np.uint32) == wsrc[first:first + n]).all(), where
        ms, wrote, up = s.times()
        assert ms >= 0 and wrote == sum(2 * rlen * nfr for _ in batch_sizes) and up >= s.info().arena_bytes
    finally:
        s.close()


# (FLEN, RLEN, cv): SHFT = 20, 1, 42, 1, 32 — reads shorter and longer than a lane's 16 bytes, 2 * RLEN a multiple of 16 and not
SHAPES = [(500, 150, 15), (40, 17, 34), (300, 150, 7), (500, 250, 300), (300, 256, 16)]


@pytest.mark.parametrize("flen,rlen,cv", SHAPES)
def test_tiles_equal_the_model(lib, hip, tmp_path, flen, rlen, cv):
    """Contigs of FLEN (one fragment), FLEN + SHFT - 1 (still one) and FLEN + SHFT (two), one too short for a fragment, and a run of
    twenty 500-520-base contigs (FLEN-scaled); batches of 1, 7 and 64 pairs start and end inside contigs, one batch covers everything."""
    shft = 2 * rlen // cv
    sizes = [flen, flen + shft - 1, flen + shft, flen - 1] + [flen + (i * 7) % 21 for i in range(20)] + [flen + 9 * shft + 3]
    contigs = contigs_of(sizes, seed=flen + rlen, marks=(0, rlen - 1, flen - rlen, flen - 1))
    check_batches(lib, hip, tmp_path, contigs, bed_of(contigs, flen, seed=cv), flen, rlen, cv, 1, (1, 7, 64, None))


def test_three_contig_groups(lib, hip, tmp_path, monkeypatch):
    """DBTK_SIM_ARENA_BYTES small enough for three groups of contigs: batches that lie in one group, span two, and span all three"""
    flen, rlen, cv = 500, 150, 15
    sizes = [700, 640, 520, 900, 560, 600, 1000]  # arena 2000: [700 640 520] [900 560] [600 1000]... by whole contigs
    contigs = contigs_of(sizes, seed=5)
    monkeypatch.setenv("DBTK_SIM_ARENA_BYTES", "2000")
    check_batches(lib, hip, tmp_path, contigs, bed_of(contigs, flen, seed=6), flen, rlen, cv, 1, (5, 13, None, 1), groups=3)


def test_a_contig_larger_than_the_arena_is_nomem(lib, tmp_path, monkeypatch):
    contigs = contigs_of([700, 2100], seed=5)
    (tmp_path / "a.fa").write_text(fasta_text(contigs))
    (tmp_path / "a.bed").write_text("")
    monkeypatch.setenv("DBTK_SIM_ARENA_BYTES", "2000")
    s = pkg.Sim(lib, str(tmp_path / "a.fa"), str(tmp_path / "a.bed"), NLOCI, 500, 150, 15, 1)
    with pytest.raises(pkg.DbtkError) as e:
        s.attach(0)
    assert e.value.status == abi.ERR_NOMEM and "2100" in str(e.value) and "2000" in str(e.value)
    s.close()


# ---- through the hot path: the two-haplotype assembly of the command-line test
@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return sim_cases.AsmCase(str(tmp_path_factory.mktemp("simgpu")))


@pytest.fixture(scope="module")
def want(lib, asm):
    """dbtk_align_batch over the model's reads, once"""
    g = lib.load(asm.pref, sim_cases.K)
    seq, off, src, _ = asm.batch()
    out = {}
    for okam in (0, 1):
        ctx = lib.context(g, abi.default_params(ksize=sim_cases.K, cthreshold=sim_cases.CTH, okam=okam, simmode=2))
        recs, n = ctx.align(seq, off)
        r = ctx.counts()
        out[okam] = (r, [(x.pair, x.stage, x.dst, x.dst0) for x in recs[:n]] if okam else None)
        ctx.close()
    return g, out


@pytest.mark.parametrize("sync", [0, 1])
def test_counts_through_the_hot_path_equal_align_batch(lib, asm, want, sync):
    g, out = want
    r0, recs0 = out[sync]
    assert int(r0["counts"].sum()) > 0 and int(r0["nmapread"].sum()) > 0
    ctx = lib.context(g, abi.default_params(ksize=sim_cases.K, cthreshold=sim_cases.CTH, okam=sync, simmode=2))
    got, base = [], 0
    for h in range(2):
        s = pkg.Sim(lib, asm.fa[h], asm.bed[h], sim_cases.NLOCI, sim_cases.FLEN, sim_cases.RLEN, sim_cases.CV, 1)
        s.attach(0)
        nfr = int(s.info().nfrags)
        for first in range(0, nfr, 97):
            n = min(97, nfr - first)
            s.batch(first, n)
            recs, nrec = s.align(ctx, sync=bool(sync))
            if sync:
                got += [(base + first + x.pair, x.stage, x.dst, x.dst0) for x in recs[:nrec]]
        ctx.synchronize()
        s.close()
        base += nfr
    r = ctx.counts()
    assert (r["counts"] == r0["counts"]).all() and (r["kmc"] == r0["kmc"]).all() and (r["nmapread"] == r0["nmapread"]).all()
    assert (r["counters"] == r0["counters"]).all(), (r["counters"], r0["counters"])
    if sync:
        assert got == recs0 and len(got) > 50
    ctx.close()


def test_profile_fed_from_the_device_equals_the_host_feed(lib, hip, asm, want):
    """dbtk_kcp_add_device over a tiled batch == dbtk_kcp_add over the model's reads with the same src / dst"""
    seq, off, src, _ = asm.batch()
    rng = np.random.default_rng(3)
    nh = [len(sim_model.fragments(asm.contigs[h], sim_cases.FLEN, sim_cases.RLEN, sim_cases.CV, 1)) for h in range(2)]
    dst = rng.integers(0, sim_cases.NLOCI + 2, nh[0] + nh[1]).astype(np.uint32)  # some pairs skipped (>= nloci), true and false positives
    a, b = pkg.Kcp(lib, sim_cases.K, sim_cases.NLOCI), pkg.Kcp(lib, sim_cases.K, sim_cases.NLOCI)
    a.add(seq, off, src, dst)
    base = 0
    for h in range(2):
        s = pkg.Sim(lib, asm.fa[h], asm.bed[h], sim_cases.NLOCI, sim_cases.FLEN, sim_cases.RLEN, sim_cases.CV, 1)
        s.attach(0)
        for first in range(0, nh[h], 200):
            n = min(200, nh[h] - first)
            d_seq, d_off, d_src = s.batch(first, n)
            s.wait()
            b.add_device(d_seq, d_off, n, d_src, dst[base + first:base + first + n])
        s.close()
        base += nh[h]
    for cls in (0, 1):
        assert a.read(cls) == b.read(cls) and a.count(cls) > 100
    a.close()
    b.close()
