"""-bu counted in the device table (params.bubbles = abi.BUBBLES_TABLE, dbtk_bubtab.h) against the oracle's event list aggregated
to {(locus, edge): count}: one batch, uneven batches on two lanes, growth from 256 slots, one edge in two loci, reset, merge, the
device reader's asynchronous and merged paths, k = 25.  The event-log form (params.bubbles = 1) keeps its restrictions."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))

import bind
import synth

abi = bind.abi
ROOT = os.path.dirname(HERE)


# ------------------------------------------------------------------ CPU ----
def test_abi_version_is_11_in_binding_and_header():
    assert abi.ABI_VERSION == 11 and abi.BUBBLES_TABLE == 2
    hdr = open(os.path.join(ROOT, "include", "dbtk.h")).read()
    assert "#define DBTK_ABI_VERSION 11u" in hdr and "#define DBTK_BUBBLES_TABLE 2u" in hdr
    assert "dbtk_ctx_bubbles" in bind.pkg.EXPORTS


def test_bu_table_flag_is_refused_at_parse_time_without_bu(tmp_path):
    """--bu-table without -bu, with -e, and --cohort -bu --bu-table without PREF.tre.kdb: status 1 and the message, before any device is touched
    (HIP_VISIBLE_DEVICES hides every device: a run that got as far as a context would fail differently)."""
    exe = os.path.join(ROOT, "danbing-tk_amd", "bin", "danbing-tk")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    pref = str(tmp_path / "pan")  # (-qs opens PREF.tr.kmers while the options are read: a real, tiny RPGG)
    synth.write_rpgg_files(synth.build_rpgg_arrays(synth.make_loci(nloci=2, nhap=1, flank=100, seed=3), 21), pref)
    fa = tmp_path / "r.fa"
    fa.write_text(">a/1\nACGT\n>a/2\nACGT\n")
    base = [exe, "-k", "21", "-qs", str(tmp_path / "pan"), "-fa", str(fa), "-o", str(tmp_path / "o"), "-p", "1"]
    r = subprocess.run(base + ["--bu-table"], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 1 and "--bu-table needs -bu" in r.stderr, r.stderr
    r = subprocess.run(base + ["-bu", "--bu-table", "-e", "1"], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 1 and "--bu-table" in r.stderr and "-bu does nothing" in r.stderr, r.stderr
    os.unlink(pref + ".tre.kdb")
    man = tmp_path / "m.tsv"
    man.write_text(f"{fa}\t{tmp_path}/s1\n")
    r = subprocess.run([exe, "-k", "21", "-qs", str(tmp_path / "pan"), "-ka", "--cohort", str(man), "-bu", "--bu-table", "-p", "1"],
                       capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 1 and "tre.kdb" in r.stderr, r.stderr


# ------------------------------------------------------------------ GPU ----
def aggregate(ev):
    want = {}
    for l, e in zip(ev["locus"], ev["edge"]):
        want[(int(l), int(e))] = want.get((int(l), int(e)), 0) + 1
    return want


def table_of(ctx, th=0):
    loci, edges, counts = ctx.bubbles(th)
    key = list(zip(loci.tolist(), edges.tolist()))
    assert key == sorted(key) and len(set(key)) == len(key), "sorted by (locus, edge), every key once"
    return dict(zip(key, counts.tolist()))


def parse_bub(fn, nloci):
    """OUT.bub.kmdb -> ({(locus, edge): count}, every locus ascending by edge?)"""
    a = np.fromfile(fn, np.uint64)
    nl = int(a[0]); nk = int(a[1 + nl])
    assert nl == nloci and a[2 + nl] == 8 and len(a) == 3 + nl + 2 * nk
    got, i, asc = {}, 0, True
    for l in range(nl):
        ks = [int(x) for x in a[3 + nl + i:3 + nl + i + int(a[1 + l])]]
        asc = asc and ks == sorted(ks)
        for j, e in enumerate(ks):
            got[(l, e)] = int(a[3 + nl + nk + i + j])
        i += len(ks)
    return got, asc


def build_prefix(loci, d, k):
    os.makedirs(d, exist_ok=True)
    if synth.have_ref():
        return synth.build_rpgg_with_reference(loci, d, k=k)
    pref = os.path.join(d, "pan")
    synth.write_rpgg_files(synth.build_rpgg_arrays(loci, k), pref)
    return pref


def fasta_of(reads):
    out = []
    for p in range(reads.npairs):
        t = reads.titles[p].encode()
        for which, tag in ((2 * p + 1, b"/2"), (2 * p, b"/1")):  # (the reader makes the LATER record of a title seqs[2p])
            out.append(b">" + t + tag + b"\n" + reads.seqs[which] + b"\n")
    return b"".join(out)


def oracle_params(p):
    q = abi.Params.from_buffer_copy(p)
    q.bubbles = 1 if p.bubbles else 0
    return q


class Base:
    """The synthetic RPGG of the event-log test, its reads, and the oracle's results: computed once, read by every test."""

    def __init__(self, d, k=21):
        self.k = k
        self.loci = synth.make_loci(nloci=10, nhap=3, flank=500, seed=61, shared_frac=0.3)
        self.pref = build_prefix(self.loci, os.path.join(d, f"k{k}"), k)
        self.reads = synth.sim_reads(self.loci, npairs=1500, seed=62, sub=0.01, indel=0.002)
        self.seq, self.off = self.reads.packed()
        self.dbtk = bind.pkg.Dbtk()
        self.oracle = bind.Oracle()
        self.g = self.dbtk.load(self.pref, k)
        self.go = self.oracle.load(self.pref, k)
        self.order = self.g.output_order()
        self.p = abi.default_params(ksize=k, cthreshold=30, okam=0, bubbles=abi.BUBBLES_TABLE)
        self.o = self.oracle.align_ex(self.go, oracle_params(self.p), self.seq, self.off, trace=False)
        self.want = aggregate(self.o["events"])

    def check_counts(self, ctx, o=None, times=1):
        o = o or self.o
        r = ctx.counts()
        co = np.zeros(self.g.ntrkmers, np.uint64)
        np.add.at(co, self.order.astype(np.int64), o["counts_file"])
        assert (times * co == r["counts"]).all() and (times * o["kmc"] == r["kmc"]).all()
        assert (times * o["nmapread"].astype(np.uint64) == r["nmapread"]).all() and (times * o["counters"] == r["counters"]).all()


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    return Base(str(tmp_path_factory.mktemp("bubtab")))


@pytest.mark.gpu
def test_one_batch_equals_the_oracles_aggregate_and_the_file_is_its_ge5_subset(base, tmp_path):
    assert len(base.want) > 2000 and any(v >= 5 for v in base.want.values())
    ctx = base.dbtk.context(base.g, base.p)
    ctx.align(base.seq, base.off)
    assert table_of(ctx, 0) == base.want
    ge5 = {k: v for k, v in base.want.items() if v >= 5}
    assert table_of(ctx, 5) == ge5
    base.check_counts(ctx)
    assert ctx.table_bytes()["bubble_table"] == 16 << 24
    ctx.write_bubbles(str(tmp_path / "t"))
    got, asc = parse_bub(str(tmp_path / "t.bub.kmdb"), base.g.nloci)
    assert got == ge5 and asc
    ctx.close()


@pytest.mark.gpu
def test_event_log_context_and_the_reference_hold_the_same_set_per_locus(base, tmp_path):
    p1 = abi.default_params(ksize=base.k, cthreshold=30, okam=0, bubbles=1)
    c1 = base.dbtk.context(base.g, p1)
    c1.align(base.seq, base.off)
    c1.write_bubbles(str(tmp_path / "log"))
    with pytest.raises(bind.pkg.DbtkError) as e:
        c1.bubbles(0)
    assert e.value.status == abi.ERR_ARG
    c1.close()
    c2 = base.dbtk.context(base.g, base.p)
    c2.align(base.seq, base.off)
    c2.write_bubbles(str(tmp_path / "tab"))
    c2.close()
    log, _ = parse_bub(str(tmp_path / "log.bub.kmdb"), base.g.nloci)
    tab, asc = parse_bub(str(tmp_path / "tab.bub.kmdb"), base.g.nloci)
    assert asc and log == tab == {k: v for k, v in base.want.items() if v >= 5}
    if synth.have_ref():  # the reference binary's own file at -p 1
        fa = str(tmp_path / "reads.fa")
        synth.write_fasta(base.reads, fa)
        r = subprocess.run([synth.ref_tool("danbing-tk"), "-bu", "-k", str(base.k), "-qs", base.pref, "-fa", fa, "-o", str(tmp_path / "ref"),
                            "-p", "1", "-cth", "30"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        ref, _ = parse_bub(str(tmp_path / "ref.bub.kmdb"), base.g.nloci)
        assert ref == tab


def device_copy(seq, off):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    d_seq, d_off = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_seq), len(seq) + 64) == 0 and hip.hipMalloc(C.byref(d_off), off.nbytes) == 0
    assert hip.hipMemcpy(d_seq, seq.ctypes.data_as(C.c_void_p), len(seq), 1) == 0
    assert hip.hipMemcpy(d_off, off.ctypes.data_as(C.c_void_p), off.nbytes, 1) == 0
    return hip, d_seq, d_off


@pytest.mark.gpu
def test_seven_uneven_device_batches_on_two_lanes_without_a_synchronize(base, monkeypatch):
    monkeypatch.setenv("DBTK_LANES", "2")
    ctx = base.dbtk.context(base.g, base.p)
    hip, d_seq, d_off = device_copy(base.seq, base.off)
    n = base.reads.npairs
    cuts = [0, 1, 8, n // 5, n // 3, n // 3 + 311, n - 2, n]
    maxlen = int(np.diff(base.off.astype(np.int64)).max())
    for a, b in zip(cuts[:-1], cuts[1:]):  # (offsets stay absolute: every batch is a window of the same arrays)
        ctx.align_device(d_seq.value, d_off.value + 16 * a, b - a, maxlen)
    assert table_of(ctx, 0) == base.want
    base.check_counts(ctx)
    ctx.close()
    hip.hipFree(d_seq); hip.hipFree(d_off)


GROWTH_CUTS = 5


def growth_child(d):
    """Run in a fresh process with DBTK_BUB_SLOTS=256 (read when the context is created)."""
    b = Base(d)
    assert len(b.want) > 2000
    ctx = b.dbtk.context(b.g, b.p)
    before = ctx.table_bytes()["bubble_table"]
    n = b.reads.npairs
    for i in range(GROWTH_CUTS):
        lo, hi = n * i // GROWTH_CUTS, n * (i + 1) // GROWTH_CUTS
        ctx.align(b.seq, b.off[2 * lo:2 * hi + 1])
    got = table_of(ctx, 0)
    after = ctx.table_bytes()["bubble_table"]
    b.check_counts(ctx)
    ctx.close()
    print("GROWTH " + json.dumps(dict(equal=got == b.want, distinct=len(b.want), before=before, after=after)))


@pytest.mark.gpu
def test_table_grows_from_256_slots_over_five_batches(tmp_path):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "growth", str(tmp_path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, DBTK_BUB_SLOTS="256"))
    line = [l for l in r.stdout.splitlines() if l.startswith("GROWTH ")]
    assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(line[0][7:])
    assert res["equal"] and res["distinct"] > 2000
    # (it grew, and a table holds at least as many slots as entries)
    assert res["before"] == 256 * 16 and res["after"] > res["before"] and res["after"] >= res["distinct"] * 16


@pytest.mark.gpu
def test_one_edge_in_two_loci_is_two_entries_with_exact_counts(base):
    """Two loci whose TR regions share 100 bp; pairs of each locus carry the same substitution inside the shared stretch, so the very same
    novel (k+1)-mers are counted at both loci — with different counts."""
    k = 21
    rng = np.random.default_rng(7)
    rnd = lambda n: synth.BASES[rng.integers(0, 4, n)]
    shared = rnd(100)
    trs = [np.concatenate([rnd(150), shared, rnd(150)]) for _ in range(2)]
    loci = synth.Loci(flank=500, haps=[[np.concatenate([rnd(500), tr, rnd(500)]) for tr in trs]], nloci=2, nhap=1)
    arr = synth.build_rpgg_arrays(loci, k)
    g = base.dbtk.from_arrays(k, arr["keys"], arr["vals"], arr["vv"], arr["fl_cnt"], arr["fl_ks"], arr["tr_cnt"], arr["tr_ks"], arr["tre_cnt"], arr["tre_ks"])
    go = base.oracle.from_arrays(g.view())
    reads = synth.Reads()
    for l, copies in ((0, 8), (1, 6)):
        tr = trs[l].copy()
        tr[200] = synth.BASES[(int(np.nonzero(synth.BASES == tr[200])[0][0]) + 1) % 4]  # the same base of the shared stretch, the same change
        for c in range(copies):
            reads.seqs += [tr[100:250].tobytes(), synth.revcomp(trs[l][250:400]).tobytes()]
            reads.titles.append(f"l{l}c{c}")
    seq, off = reads.packed()
    p = abi.default_params(ksize=k, cthreshold=30, okam=0, bubbles=abi.BUBBLES_TABLE)
    o = base.oracle.align_ex(go, oracle_params(p), seq, off, trace=False)
    want = aggregate(o["events"])
    both = [e for (l, e) in want if l == 0 and (1, e) in want]
    assert both and all(want[(0, e)] == 8 and want[(1, e)] == 6 for e in both), "the oracle itself counts one edge at both loci"
    ctx = base.dbtk.context(g, p)
    ctx.align(seq, off)
    assert table_of(ctx, 0) == want
    ctx.close()
    base.oracle.free(go)
    g.close()


@pytest.mark.gpu
def test_reset_empties_the_table(base):
    n = base.reads.npairs
    ctx = base.dbtk.context(base.g, base.p)
    ctx.align(base.seq, base.off[:2 * (n // 2) + 1])
    assert table_of(ctx, 0)
    ctx.reset()
    assert table_of(ctx, 0) == {}
    tail = base.off[2 * (n // 2):]
    ctx.align(base.seq, tail)
    o2 = base.oracle.align_ex(base.go, oracle_params(base.p), base.seq, tail, trace=False)
    assert table_of(ctx, 0) == aggregate(o2["events"])
    base.check_counts(ctx, o2)
    ctx.close()


@pytest.mark.gpu
def test_merge_of_two_table_contexts_and_refusal_of_a_mixed_pair(base):
    n = base.reads.npairs
    a, b = base.dbtk.context(base.g, base.p), base.dbtk.context(base.g, base.p)
    a.align(base.seq, base.off[:2 * (n // 2) + 1])
    b.align(base.seq, base.off[2 * (n // 2):])
    a.merge_bubbles(b)
    assert table_of(a, 0) == base.want
    c1 = base.dbtk.context(base.g, abi.default_params(ksize=base.k, cthreshold=30, okam=0, bubbles=1))
    for dst, src in ((a, c1), (c1, a)):
        with pytest.raises(bind.pkg.DbtkError) as e:
            dst.merge_bubbles(src)
        assert e.value.status == abi.ERR_ARG
    for c in (a, b, c1):
        c.close()


@pytest.mark.gpu
def test_device_reader_asynchronous_and_merged_paths_take_a_table_context(base):
    data = fasta_of(base.reads)
    chunk = 65536
    nblocks = (len(data) + chunk - 1) // chunk
    for merged in (False, True):
        ctx = base.dbtk.context(base.g, base.p)
        ing = bind.pkg.Ingest(ctx, False, 0, chunk, nslots=4, with_spans=False)
        slots = []
        for j in range(nblocks):
            slots.append(ing.submit(data[j * chunk:(j + 1) * chunk], j == nblocks - 1))
            if len(slots) == 3 or j == nblocks - 1:
                for s in (slots if j == nblocks - 1 else slots[:1]):
                    info = ing.wait(s)
                    assert info.flags == 0
                    if merged:
                        ing.align_merged(s, 400)
                    else:
                        ing.align(s, info, sync=False)
                slots = [] if j == nblocks - 1 else slots[1:]
        if merged:
            ing.align_merged(None, 0, flush=True)
        assert table_of(ctx, 0) == base.want, merged
        base.check_counts(ctx)
        ing.close()
        ctx.close()
    # the event-log form: both still refused, with the messages they have always had
    c1 = base.dbtk.context(base.g, abi.default_params(ksize=base.k, cthreshold=30, okam=0, bubbles=1))
    ing = bind.pkg.Ingest(c1, False, 0, chunk, nslots=2, with_spans=False)
    s = ing.submit(data[:chunk], nblocks == 1)
    info = ing.wait(s)
    with pytest.raises(bind.pkg.DbtkError) as e:
        ing.align(s, info, sync=False)
    assert e.value.status == abi.ERR_ARG and "dbtk_ingest_align: -bu is replayed batch by batch on the host: sync = 1" in str(e.value)
    with pytest.raises(bind.pkg.DbtkError) as e:
        ing.align_merged(s, 1)
    assert e.value.status == abi.ERR_ARG and "dbtk_ingest_align_merged: records, -bu and -b with qualities go block by block (dbtk_ingest_align)" in str(e.value)
    ing.close()
    c1.close()


@pytest.mark.gpu
def test_k25_edges_of_52_bits_keep_their_locus(tmp_path):
    b = Base(str(tmp_path), k=25)
    assert len(b.want) > 2000 and max(e for _, e in b.want) >= 1 << 48
    ctx = b.dbtk.context(b.g, b.p)
    ctx.align(b.seq, b.off)
    assert table_of(ctx, 0) == b.want
    assert table_of(ctx, 5) == {k: v for k, v in b.want.items() if v >= 5}
    b.check_counts(ctx)
    ctx.close()


if __name__ == "__main__":
    if sys.argv[1] == "growth":
        growth_child(sys.argv[2])
