#!/usr/bin/env python3
"""Batches for the lean probe kernel (dbtk_probe2.h) on a survivor list that was NOT sorted — the form a WGS-like batch takes: few
survivors per locus, no locus-resident kernel, every pair of a wave's range another locus — each small and built to hit one edge,
checked against the oracle: counts, kmc, nmapread and every counter bit-exact.  tests/test_probe_unsorted.py runs them one by one;
    python tests/probe_unsorted.py
runs them all in one process (the launcher reads its switches, DBTK_P2_CACHE among them, once per process: a child process per
setting) and prints "N/N batches bit-exact".

Which form a batch takes is decided by what the batch BEFORE it left in the context's hint words, so every context here first
aligns a primer — one background pair, no survivor — and is reset: the batches after it are not sorted and skip the locus path
(checked: the sort's timer slot records no launch for them — the launcher picks the probe kernel's form by that very decision —,
and by the path statistics no pair went through the locus-resident kernel or onto its rest list)."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import bind  # noqa: E402
import cases  # noqa: E402
import synth  # noqa: E402

abi = bind.abi
K = 21
LMAX = 32 * 5 + 15 - 1  # bases the lanes of a half-wave cover at k = 21 (minimizers of 15 bases): 174


def loci_plain():
    return synth.make_loci(nloci=12, nhap=3, flank=500, seed=5)


def loci_repeats():
    """Tandem repeats of short motifs with many variants: many k-mers around few minimizers, so that full buckets turn keys away
    (the emulator part of the tests checks that they do: Emu.probe_stats()[2] > 0)."""
    return synth.make_loci(nloci=6, nhap=3, flank=300, seed=77, tr_min=600, tr_max=1500, motif_min=5, motif_max=9, variation=0.6)


def primer():
    r = synth.Reads()
    rng = np.random.default_rng(99)
    r.seqs = [synth.BASES[rng.integers(0, 4, 150)].tobytes() for _ in range(2)]
    r.titles = ["primer"]
    return r


def join(*parts):
    out = synth.Reads()
    for r in parts:
        out.seqs += r.seqs
        out.titles += r.titles
    return out


def from_locus(loci, l, npairs, seed, rlen=150, **kw):
    """npairs pairs of locus l alone"""
    one = synth.Loci(flank=loci.flank, haps=[[h[l]] for h in loci.haps], nloci=1, nhap=loci.nhap)
    return synth.sim_reads(one, npairs=npairs, rlen=rlen, seed=seed, **kw)


def with_n_in_each_mate(reads):
    out = synth.Reads(titles=list(reads.titles))
    for i, s in enumerate(reads.seqs):
        b = bytearray(s)
        b[(17 + 31 * i) % len(b)] = ord("N")
        out.seqs.append(bytes(b))
    return out


# name -> (loci, [batches], parameter sets, environment).  Each batch is aligned on the same context, results compared after each.
def scenarios():
    P, R = loci_plain(), loci_repeats()
    usual = [dict(cthreshold=45, okam=0), dict(cthreshold=45, okam=1)]
    bg = lambda n, seed: synth.sim_reads(P, npairs=n, seed=1000 + seed, background=1.0)  # (seeds away from the loci's: the same seed draws the same bases)
    sc = {}
    # far fewer pairs than the launched waves (a launch is at least the resident waves, 4 096): most waves have no work, every working
    # wave's range is one pair, and the count is no multiple of anything
    sc["ranges"] = (P, [join(bg(5, 1), synth.sim_reads(P, npairs=37, seed=2, sub=0.005), bg(3, 3))], usual, {})
    sc["none"] = (P, [bg(9, 4)], usual, {})
    sc["one"] = (P, [join(bg(4, 5), from_locus(P, 3, 1, 6), bg(4, 7))], usual, {})
    # one position, two, the usual read, the longest the lanes cover (more runs than staged rows)
    sc["lengths"] = (P, [join(*[synth.sim_reads(P, npairs=24, rlen=L, seed=10 + L, sub=0.004, frag=(max(300, L), 520)) for L in (21, 22, 150, LMAX)])],
                     [dict(cthreshold=45, okam=0), dict(cthreshold=1, okam=0), dict(cthreshold=1, okam=1)], {})
    # a non-ACGT byte in each mate: the exact path, in the middle of a wave's range
    sc["n_bases"] = (P, [join(synth.sim_reads(P, npairs=11, seed=20), with_n_in_each_mate(synth.sim_reads(P, npairs=3, seed=21)),
                              synth.sim_reads(P, npairs=11, seed=22))], usual, {})
    # overflow look-ups: pairs of one tandem-repeat locus next to each other, and apart
    sc["overflow"] = (R, [join(from_locus(R, 2, 2, 30), synth.sim_reads(R, npairs=40, seed=31, sub=0.004), from_locus(R, 2, 1, 32),
                               from_locus(R, 4, 3, 33))], usual, {})
    S = synth.make_loci(nloci=30, nhap=2, flank=500, seed=7, shared_frac=0.8)
    sc["shared"] = (S, [synth.sim_reads(S, npairs=300, seed=13, sub=0.005, chimeric=0.5)], [dict(cthreshold=45, okam=0), dict(cthreshold=20, okam=0)], {})
    X = synth.make_loci(nloci=10, nhap=3, flank=500, seed=51)
    sc["spliced"] = (X, [synth.sim_reads(X, npairs=300, seed=52, sub=0.003, splice=0.4)], [dict(cthreshold=45, okam=0), dict(cthreshold=30, okam=0)], {})
    # two batches in a row on one context, the second with fewer survivors: what is zeroed per batch, and the hint of the batch before
    sc["two_batches"] = (P, [join(synth.sim_reads(P, npairs=20, seed=40), bg(6, 41)), join(bg(6, 42), synth.sim_reads(P, npairs=7, seed=43))], usual, {})
    # the hit buffers hold 37 pairs: the probe kernel runs several times per batch
    sc["chunks"] = (P, [synth.sim_reads(P, npairs=120, seed=50, sub=0.005, background=0.1)], usual, {"DBTK_SURV_CAP": "37"})
    return sc


def run_scenario(name, dbtk, oracle, tmp, sc=None):
    """Aligns the scenario's batches after the primer, each against the oracle.  Returns (pairs the lean kernel resolved itself, by the
    path statistics; the survivors of every batch aligned)."""
    loci, batches, param_sets, env = (sc or scenarios())[name]
    pref = cases._np_rpgg(tmp, name, loci, K)
    go, g = oracle.load(pref, K), dbtk.load(pref, K)
    order = g.output_order().astype(np.int64)
    old = {k_: os.environ.get(k_) for k_ in env}
    os.environ.update(env)
    lean, surv = 0, []
    try:
        for kw in param_sets:
            p = abi.default_params(ksize=K, **kw)
            ctx = dbtk.context(g, p)
            ctx.align(*primer().packed())
            assert int(ctx.counts()["counters"][abi.C_SURVIVORS]) == 0
            for reads in batches:
                ctx.reset()
                ctx.timers_reset()
                seq, off = reads.packed()
                ctx.align(seq, off)
                r = ctx.counts()
                o = oracle.align(go, p, seq, off, trace=False)
                co = np.zeros(g.ntrkmers, np.uint64)
                np.add.at(co, order, o["counts_file"])
                assert (co == r["counts"]).all(), (name, kw, f"{int((co != r['counts']).sum())} k-mer counts differ")
                assert (o["kmc"] == r["kmc"]).all() and (o["nmapread"] == r["nmapread"]).all(), (name, kw)
                assert (o["counters"] == r["counters"]).all(), (name, kw, o["counters"], r["counters"])
                kt = ctx.kernel_times()
                assert kt["k_probe"][1] > 0 and kt.get("k_surv_sort", (0.0, 0))[1] == 0, (name, kt)  # the sort was not launched: the list is not sorted
                ps = ctx.path_stats()
                assert sum(ps["probe_pairs"]) == 0 and ps["probe_rest"] == 0, (name, ps)  # no locus path: the list was not sorted
                lean += ps["lean_done"]
                surv.append(int(r["counters"][abi.C_SURVIVORS]))
            ctx.close()
    finally:
        for k_, v in old.items():
            if v is None:
                os.environ.pop(k_, None)
            else:
                os.environ[k_] = v
        oracle.free(go)
        g.close()
    return lean, surv


def main():
    dbtk, orc = bind.pkg.Dbtk(), bind.Oracle()
    sc = scenarios()
    with tempfile.TemporaryDirectory() as tmp:
        for name in sc:
            lean, surv = run_scenario(name, dbtk, orc, tmp, sc)
            print(f"{name}: ok (survivors {surv}, {lean} pairs resolved by the lean kernel)", flush=True)
    print(f"{len(sc)}/{len(sc)} batches bit-exact")


if __name__ == "__main__":
    main()
