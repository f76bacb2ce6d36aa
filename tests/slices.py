#!/usr/bin/env python3
"""Device batches that dbtk_align_batch_device cuts into slices (danbing-tk_amd/csrc/dbtk_slices.h, dbtk_hip.hip), each small and
built for one edge, checked against the oracle: counts, kmc, nmapread and every counter bit-exact.  tests/test_slices.py uses the
pieces in its own process; with DBTK_TRACE_LAUNCHES=1 (read once per process) it runs
    python tests/slices.py launches
as a child, once per DBTK_SLICE_PAIRS: every scenario between two marks on stderr, so that the parent can count the encode kernel's
launches of each, and a RESULT line per scenario on stdout."""
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import bind  # noqa: E402
import synth  # noqa: E402
from probe_unsorted import LMAX, join, with_n_in_each_mate  # noqa: E402

abi = bind.abi
K = 21
SIZES = (1, 15, 16, 17, 47, 48, 49, 200)
WHOLE = {"walk": dict(threading=abi.THREADING_V13, thread_cth=85, correction=1, maxncorrection=3), "bu": dict(bubbles=abi.BUBBLES_TABLE), "trace": dict(trace=1)}
KEYS = ("counts", "kmc", "nmapread", "counters")

_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipFree.argtypes = [C.c_void_p]
    return _hip


class DevReads:
    """A batch in device memory, as dbtk_align_batch_device wants it: readable to the end of the last read rounded up to 16."""

    def __init__(self, reads):
        self.seq, self.off = reads.packed()
        self.npairs = reads.npairs
        self.maxlen = int(np.diff(self.off.astype(np.int64)).max())
        self.d_seq, self.d_off = C.c_void_p(), C.c_void_p()
        assert hip().hipMalloc(C.byref(self.d_seq), len(self.seq) + 64) == 0 and hip().hipMalloc(C.byref(self.d_off), self.off.nbytes) == 0
        assert hip().hipMemcpy(self.d_seq, self.seq.ctypes.data_as(C.c_void_p), len(self.seq), 1) == 0
        assert hip().hipMemcpy(self.d_off, self.off.ctypes.data_as(C.c_void_p), self.off.nbytes, 1) == 0

    def align(self, ctx, maxlen=None):
        ctx.align_device(self.d_seq.value, self.d_off.value, self.npairs, maxlen or self.maxlen)

    def free(self):
        hip().hipFree(self.d_seq); hip().hipFree(self.d_off)


class World:
    """One small RPGG (with its graph, for the walking context) on the device and in the oracle."""

    def __init__(self, tmp):
        self.loci = synth.make_loci(nloci=12, nhap=3, flank=500, seed=5)
        d = os.path.join(tmp, "slices")
        os.makedirs(d, exist_ok=True)
        self.prefix = os.path.join(d, "pan")
        synth.write_rpgg_files(synth.build_rpgg_arrays(self.loci, K), self.prefix)
        synth.write_graph_file(synth.build_graph_arrays(self.loci, K), self.prefix)
        self.dbtk, self.oracle = bind.pkg.Dbtk(), bind.Oracle()
        self.g = self.dbtk.load(self.prefix, K, flags=abi.LOAD_GRAPH)
        self.go = self.oracle.load(self.prefix, K)
        self.oracle.load_graph(self.go, self.prefix + ".graph.kmers")
        self.order = self.g.output_order().astype(np.int64)

    def want(self, p, batches):
        """The oracle's totals over the batches, counts in the library's order."""
        tot = None
        for reads in batches:
            seq, off = reads.packed()
            q = abi.Params.from_buffer_copy(p)
            q.bubbles = 1 if p.bubbles else 0
            if p.threading == abi.THREADING_V13:
                o = self.oracle.align_walk(self.go, q, seq, off)
            elif p.bubbles:
                o = self.oracle.align_ex(self.go, q, seq, off, trace=False)
            else:
                o = self.oracle.align(self.go, q, seq, off, trace=False)
            co = np.zeros(self.g.ntrkmers, np.uint64)
            np.add.at(co, self.order, o["counts_file"])
            one = dict(counts=co, kmc=o["kmc"].astype(np.uint64), nmapread=o["nmapread"].astype(np.uint64), counters=o["counters"].astype(np.uint64))
            tot = one if tot is None else {k_: tot[k_] + one[k_] for k_ in KEYS}
        return tot

    def diff(self, want, got):
        """"" when the context's totals are the oracle's, else what differs"""
        bad = [k_ for k_ in KEYS if not (want[k_] == got[k_].astype(np.uint64)).all()]
        return ", ".join(f"{k_}: {int((want[k_] != got[k_].astype(np.uint64)).sum())} differ" for k_ in bad)

    def close(self):
        self.oracle.free(self.go)
        self.g.close()


def bg(n, seed, loci, rlen=150):
    return synth.sim_reads(loci, npairs=n, seed=1000 + seed, background=1.0, rlen=rlen)


def half_and_half(loci, n, seed):
    """n pairs, half from the loci, half background, interleaved by the generator's own draw"""
    return synth.sim_reads(loci, npairs=n, seed=seed, sub=0.004, background=0.5)


def shapes(loci, s):
    """2 s + 1 pairs for slices of s: a slice of background alone (no survivor), a slice from the loci in reads of 21, 22, 150 and
    174 bases (so the boundaries fall at offsets that are no multiple of 16), a last slice of one pair; an N in each mate of the
    pairs on both sides of both boundaries."""
    q = s // 4
    mixed = join(*[synth.sim_reads(loci, npairs=(q if i else s - 3 * q), rlen=L, seed=10 + L, sub=0.004, frag=(max(300, L), 520)) for i, L in enumerate((150, 21, LMAX, 22))])
    r = join(bg(s - 1, 1, loci), bg(1, 2, loci, rlen=145), mixed, synth.sim_reads(loci, npairs=1, seed=77))
    assert sum(len(x) for x in r.seqs[:2 * s]) % 16 and sum(len(x) for x in r.seqs[:4 * s]) % 16
    assert r.npairs == 2 * s + 1
    for p in (s - 1, s, 2 * s - 1, 2 * s):
        nn = with_n_in_each_mate(synth.Reads(seqs=r.seqs[2 * p:2 * p + 2], titles=r.titles[p:p + 1]))
        r.seqs[2 * p:2 * p + 2] = nn.seqs
    return r


def too_long_in_the_middle(loci, s):
    """4 s pairs of 100 bases and, in the second slice, one pair of 150 from a locus: longer than the 100 the caller will promise"""
    r = synth.sim_reads(loci, npairs=4 * s, rlen=100, seed=31, frag=(300, 500))
    one = synth.sim_reads(loci, npairs=1, rlen=150, seed=32)
    p = s + s // 2
    r.seqs[2 * p:2 * p + 2] = one.seqs
    return r


def hints_main():
    """The child under DBTK_TRACE_LAUNCHES=1, DBTK_LANES=1 and no DBTK_SLICE_PAIRS: the default rule on a batch of 2^20 pairs, one in
    ten thousand from a locus (the generator of bench.py, 300 loci: ~100 survivors against the sort's 600).  Three calls between marks:
    the first runs whole (no hint yet), the others in halves; then an all-hit batch of the same size, twice: whole.  The totals are
    those of a context that never slices (DBTK_SLICE_PAIRS=0 set for its creation)."""
    dbtk = bind.pkg.Dbtk()
    syn = bind.pkg.Synth(nloci=300)
    arrs = syn.arrays()
    h = C.c_void_p()
    dbtk._chk(dbtk.L.dbtk_rpgg_from_arrays(C.byref(arrs), C.byref(h)))
    g = bind.pkg.Rpgg(dbtk, h)
    p = abi.default_params(ksize=K, cthreshold=45, okam=0)
    n = 1 << 20
    batches = {"wgs": syn.reads(n, hit_frac=1e-4, seed=5), "allhit": syn.reads(n, hit_frac=1.0, seed=6)}
    dev = {}
    for name, (seq, off) in batches.items():
        d_seq, d_off = C.c_void_p(), C.c_void_p()
        assert hip().hipMalloc(C.byref(d_seq), len(seq) + 64) == 0 and hip().hipMalloc(C.byref(d_off), off.nbytes) == 0
        assert hip().hipMemcpy(d_seq, seq.ctypes.data_as(C.c_void_p), len(seq), 1) == 0
        assert hip().hipMemcpy(d_off, off.ctypes.data_as(C.c_void_p), off.nbytes, 1) == 0
        dev[name] = (d_seq, d_off)
    calls = [("wgs", 1), ("wgs", 2), ("wgs", 3), ("allhit", 1), ("allhit", 2)]

    def run(mark):
        ctx = dbtk.context(g, p)
        ctx.timers_enable(False)
        for name, i in calls:
            if mark:
                print(f"[mark] {name}{i} begin", file=sys.stderr, flush=True)
            ctx.align_device(dev[name][0].value, dev[name][1].value, n, 150)
            ctx.synchronize()
            if mark:
                print(f"[mark] {name}{i} end", file=sys.stderr, flush=True)
        r = ctx.counts()
        ctx.close()
        return r
    got = run(True)
    os.environ["DBTK_SLICE_PAIRS"] = "0"
    want = run(False)
    bad = [k_ for k_ in KEYS if not (want[k_] == got[k_]).all()]
    print("RESULT " + json.dumps(dict(name="hints", diff=", ".join(bad), survivors=int(got["counters"][abi.C_SURVIVORS]))), flush=True)
    g.close()
    print("slices child ok")


def main():
    """The child under DBTK_TRACE_LAUNCHES=1: batches of every size on a counting context, then one batch on each context that must
    stay whole."""
    if sys.argv[1:] == ["hints"]:
        return hints_main()
    assert sys.argv[1:] == ["launches"]
    with tempfile.TemporaryDirectory() as tmp:
        w = World(tmp)

        def scenario(name, p, reads):
            dev = DevReads(reads)
            ctx = w.dbtk.context(w.g, p)
            ctx.timers_enable(False)
            sys.stderr.flush()
            print(f"[mark] {name} begin", file=sys.stderr, flush=True)
            dev.align(ctx)
            ctx.synchronize()
            print(f"[mark] {name} end", file=sys.stderr, flush=True)
            d = w.diff(w.want(p, [reads]), ctx.counts())
            print("RESULT " + json.dumps(dict(name=name, npairs=reads.npairs, diff=d)), flush=True)
            ctx.close()
            dev.free()
        for n in SIZES:
            scenario(f"n{n}", abi.default_params(ksize=K, cthreshold=45, okam=0), half_and_half(w.loci, n, 100 + n))
        for name, kw in WHOLE.items():
            scenario(name, abi.default_params(ksize=K, cthreshold=45, okam=0, **kw), half_and_half(w.loci, 200, 300))
        w.close()
    print("slices child ok")


if __name__ == "__main__":
    main()
