"""An optional table joining a share of device tables that is already live: the graph table, its minimizer-grouped copy and
the graph images are built by the first WALKING context of a (handle, device), into the share a plain context made before it — and
belong to the share from then on, whichever context goes first."""
from __future__ import annotations

import ctypes as C

import pytest

import bind
from test_walk import WalkCase, check_pair_mode

abi = bind.abi
pytestmark = pytest.mark.gpu


def test_graph_joins_a_live_share_and_survives_the_plain_context(tmp_path):
    """A plain context first, then a walking one on the same handle (it adds graph table, minimizer copy and graph images to the
    plain one's share), the plain one closed, the batch aligned by the walking one: the oracle's pair-mode results."""
    k = 21
    O = bind.Oracle()
    D = bind.pkg.Dbtk()
    case = WalkCase(str(tmp_path), "ts", k, 3)
    oh = O.load(case.prefix, k); O.load_graph(oh, case.prefix + ".graph.kmers")
    g = D.load(case.prefix, k, flags=abi.LOAD_GRAPH)
    order = g.output_order()

    def run(p, seq, off):
        plain_p = type(p).from_buffer_copy(p)
        plain_p.threading = 0
        plain = D.context(g, plain_p, device=0)
        assert plain.table_bytes()["graph"] == 0
        ctx = D.context(g, p, device=0)
        tb = ctx.table_bytes()
        assert tb == plain.table_bytes()                         # one share: the plain context reports what the walking one added
        assert tb["graph"] > 0 and tb["graph_by_minimizer"] > 0 and tb["graph_images"] > 0
        assert tb["total"] == sum(v for n, v in tb.items() if n not in ("total", "index_images:from_cache"))
        plain.close()                                            # the share's first context goes; what the second added stays
        ctx.align(seq, off)
        r = ctx.counts()
        res, _, nres = ctx.walk_results(len(off))
        out = dict(counts=r["counts"], counters=r["counters"], res=res, nres=nres, aln=ctx.aln_records(), order=order, txt=ctx.aln_text(len(off) // 2))
        ctx.close()
        return out
    check_pair_mode(run, O, oh, case, k, case.loci.nloci)
    g.close()


def test_graph_is_built_once_and_freed_with_the_share():
    """HBM by hipMemGetInfo: the first walking context pays for the graph tables, the second only for its own buffers; with the builder
    of the share and the builder of the graph both closed before the last context, everything goes back."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]

    def free_bytes():
        f, t = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value
    dbtk = bind.pkg.Dbtk()
    syn = bind.pkg.Synth(nloci=4000)
    syn.graph()
    arrs = syn.arrays()
    h = C.c_void_p()
    dbtk._chk(dbtk.L.dbtk_rpgg_from_arrays(C.byref(arrs), C.byref(h)))
    g = bind.pkg.Rpgg(dbtk, h)
    p = abi.default_params(ksize=21, cthreshold=45, okam=0)
    pw = abi.default_params(ksize=21, cthreshold=45, okam=0, threading=abi.THREADING_V13, thread_cth=85, correction=1, maxncorrection=3)
    seq, off = syn.reads(20000, hit_frac=0.5, seed=4)
    # (twice through everything first, with the contexts of the measured cycle alive: what the HIP runtime keeps for itself at a kernel's
    # first launches is not the library's to give back: see test_contexts_share_device_tables)
    for _ in range(2):
        warm = [dbtk.context(g, p), dbtk.context(g, pw), dbtk.context(g, pw)]
        for c0 in warm:
            c0.align(seq, off)
        for c0 in warm:
            c0.close()
    m0 = free_bytes()
    plain = dbtk.context(g, p)
    m1 = free_bytes()
    walk1 = dbtk.context(g, pw)
    m2 = free_bytes()
    walk2 = dbtk.context(g, pw)
    m3 = free_bytes()
    tb = walk2.table_bytes()
    print(f"free HBM: {m0} -> {m1} (plain) -> {m2} (first walking) -> {m3} (second walking); graph tables "
          f"{tb['graph'] + tb['graph_by_minimizer'] + tb['graph_images']} of {tb['total']} bytes")
    assert m1 - m2 > 0 and m2 - m3 < 0.25 * (m0 - m2), (m0, m1, m2, m3)   # the graph once: a further walking context costs its own buffers
    plain.close(); walk1.close()                                          # the share's builder, then the graph's
    assert walk2.table_bytes() == tb
    walk2.close()
    assert free_bytes() >= m0 - 64e6, (m0, free_bytes())                  # ... and all of it goes with the last context
    g.close()
    syn.close()
