"""The genotype score on the GPU (include/dbtk_eval.h, csrc/dbtk_eval.hip) at library level: what k_eval_truth counts from attached
assemblies against the model of tests/eval_model.py (which test_eval_model.py pins to the compiled fa2kmers), what k_eval_sums adds up
over hand-made vectors against Python integers, and a context's accumulators scored where they lie.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import bind
import eval_cases
import eval_model
import sim_cases
import sim_model

pkg, abi = bind.pkg, bind.abi
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pkg.Dbtk()


class Hip:
    def __init__(self):
        h = self.h = C.CDLL("libamdhip64.so")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipFree.argtypes = [C.c_void_p]

    def put(self, arr):
        d = C.c_void_p()
        assert self.h.hipMalloc(C.byref(d), max(arr.nbytes, 8)) == 0
        assert self.h.hipMemcpy(d, arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1) == 0
        return d

    def free(self, d):
        self.h.hipFree(d)


def rpgg_of(lib, case):
    a = case.arrays
    return lib.from_arrays(case.k, a["keys"], a["vals"], a["vv"], a["fl_cnt"], a["fl_ks"], a["tr_cnt"], a["tr_ks"], a["tre_cnt"], a["tre_ks"])


@pytest.mark.parametrize("k,small_arena", [(21, False), (21, True), (20, False)])
def test_truth_equals_the_model(lib, tmp_path, monkeypatch, k, small_arena):
    """Every edge of eval_cases.TruthCase, two assemblies added one after the other; with the default arena (one contig group each) and
    with DBTK_SIM_ARENA_BYTES so small that the first assembly goes through in three groups: the same truth, the same windows.
    k = 20: windows whose k-mer is its own reverse complement (there is none at odd k)."""
    case = eval_cases.TruthCase(k)
    files = case.write(str(tmp_path))
    g = rpgg_of(lib, case)
    slots, flank, beg = eval_cases.order_of(g)
    want_x, want_w = eval_model.truth(case.window_counts(), slots, g.ntrkmers)
    assert sum(want_x) > 3000 and sum(want_w) > sum(want_x) and want_w[1] == 0 and want_w[2] == 1
    assert any(want_x[i] > 64 for i in range(beg[11], beg[12]))   # the tandem repeat: a whole wave adds to one counter
    # TR k-mers that are flank k-mers of their locus as well (flank to the class table): the truth counts them
    assert sum(want_x[s] for l in range(g.nloci) for km, s in slots[l].items() if km in flank[l]) > 0
    if small_arena:
        monkeypatch.setenv("DBTK_SIM_ARENA_BYTES", str(case.arena))
    ev = pkg.Eval(lib, g)   # (no context exists: the evaluator builds the class table itself)
    try:
        for a, (fa, bd) in enumerate(files):
            s = pkg.Sim(lib, fa, bd, eval_cases.NLOCI, eval_cases.FLEN, eval_cases.RLEN, eval_cases.CV, 1)
            s.attach(0)
            assert s.info().ngroups == (3 if small_arena and a == 0 else 1)
            ev.truth_sim(s)
            if a == 0:   # the first assembly alone
                x, w = ev.truth()
                x0, w0 = eval_model.truth(case.window_counts((0,)), slots, g.ntrkmers)
                assert x.tolist() == x0 and w.tolist() == w0
            s.close()
        x, w = ev.truth()
        assert x.tolist() == want_x and w.tolist() == want_w
        t_ms, _, looked = ev.times()
        assert t_ms > 0 and looked == sum(want_w)
        ev.truth_reset()
        x, w = ev.truth()
        assert not x.any() and not w.any()
    finally:
        ev.close()
        g.close()


def test_truth_sim_checks_its_arguments(lib, tmp_path):
    case = eval_cases.TruthCase(21)
    (fa, bd), _ = case.write(str(tmp_path))
    g = rpgg_of(lib, case)
    ev = pkg.Eval(lib, g)
    s = pkg.Sim(lib, fa, bd, eval_cases.NLOCI, ml=1)
    with pytest.raises(pkg.DbtkError) as e:
        ev.truth_sim(s)   # not attached
    assert e.value.status == abi.ERR_ARG and "attach" in str(e.value)
    s.close()
    s = pkg.Sim(lib, fa, bd, eval_cases.NLOCI + 1, ml=1)
    s.attach(0)
    with pytest.raises(pkg.DbtkError) as e:
        ev.truth_sim(s)   # opened for another number of loci
    assert e.value.status == abi.ERR_ARG and "loci" in str(e.value)
    s.close()
    x, w = ev.truth()
    assert not x.any() and not w.any()
    ev.close()
    g.close()


def test_sums_equal_python_integers_and_overflow_is_detected(lib):
    """Loci of 0, 1, 63, 64, 65, 5000, 511, 512, 513, 7, 0 and 1300 k-mers (a wave's up to 512, a workgroup's above); x up to 2^20 and y
    up to 2^31; an all-zero truth; then one term x = 2^31, y = 2^33 in the 5000-k-mer locus: DBTK_ERR_OVERFLOW naming it, no sums."""
    g = eval_cases.sized_rpgg(lib)
    _, _, beg = eval_cases.order_of(g)
    assert [beg[l + 1] - beg[l] for l in range(g.nloci)] == eval_cases.SIZES
    nk = g.ntrkmers
    rng = np.random.default_rng(5)
    x = rng.choice(np.array([0, 0, 1, 2, 3, 1000, 1 << 20], np.uint64), nk)
    big = rng.integers(0, 1 << 20, nk, dtype=np.uint64)
    m = rng.random(nk) < 0.3
    x[m] = big[m]
    y = rng.integers(0, 1 << 24, nk, dtype=np.uint64)
    y[rng.random(nk) < 0.2] = 0
    for l in range(g.nloci):   # two counts of 2^31 a locus (three more and Syy would leave 64 bits)
        for i, v in zip(range(beg[l], beg[l + 1]), ((1 << 31) - 1, 1 << 31)):
            x[i], y[i] = 1 << 20, v
    x[beg[6]:beg[7]] = 0       # a locus whose truth is all zero
    hip = Hip()
    ev = pkg.Eval(lib, g)
    d_y = hip.put(y)
    try:
        ev.truth_set(x)
        got = ev.score_device(d_y.value)
        want = eval_model.sums(x.tolist(), y.tolist(), beg)
        assert all(eval_model.fits64(s) for s in want) and max(s["Sxy"] for s in want) > 1 << 51 and max(s["Syy"] for s in want) > 1 << 62
        assert got == want
        assert want[0]["nk"] == 0 and want[6]["Sxy"] == 0 and want[6]["Sy"] > 0 and want[5]["n1"] > 1000
        tx, tw = ev.truth()
        assert (tx == x).all() and tw.tolist() == [s["Sx"] for s in want]   # without windows: windows = Sx
        assert ev.score_host(y) == want
        win = np.arange(g.nloci, dtype=np.uint64) * np.uint64(3)
        ev.truth_set(x, win)
        assert ev.score_device(d_y.value) == eval_model.sums(x.tolist(), y.tolist(), beg, windows=win.tolist())
        assert ev.times()[1] > 0
        # all-zero truth
        ev.truth_set(np.zeros(nk, np.uint64))
        z = ev.score_device(d_y.value)
        assert z == eval_model.sums([0] * nk, y.tolist(), beg) and all(s["Sxy"] == 0 and s["n1"] == 0 for s in z)
        # the overflow: in a workgroup's locus and in a wave's
        for l in (5, 2):
            x2, y2 = x.copy(), y.copy()
            x2[beg[l] + 17], y2[beg[l] + 17] = 1 << 31, 1 << 33
            assert not eval_model.fits64(eval_model.sums(x2.tolist(), y2.tolist(), beg)[l])
            ev.truth_set(x2)
            with pytest.raises(pkg.DbtkError) as e:
                ev.score_host(y2)
            assert e.value.status == abi.ERR_OVERFLOW and f"locus {l} " in str(e.value)
            with pytest.raises(pkg.DbtkError) as e:
                ev.sums()   # no wrapped number is handed out
            assert e.value.status == abi.ERR_ARG
        with pytest.raises(pkg.DbtkError) as e:
            ev.score_device(y.ctypes.data)   # host memory
        assert e.value.status == abi.ERR_ARG
    finally:
        hip.free(d_y)
        ev.close()
        g.close()


def test_a_context_scored_where_its_counts_lie(lib, tmp_path):
    """A two-haplotype --sim run through a context (asynchronous batches, the truth pass of each assembly before its first batch), then
    dbtk_eval_score_ctx: the sums of the model over dbtk_ctx_counts and the model's truth.  A context with unflushed merged pairs and
    an evaluator of another RPGG are refused."""
    asm = sim_cases.AsmCase(str(tmp_path))
    K, NL = sim_cases.K, sim_cases.NLOCI
    g = lib.load(asm.pref, K)
    slots, flank, beg = eval_cases.order_of(g)
    ctx = lib.context(g, abi.default_params(ksize=K, cthreshold=sim_cases.CTH, okam=0, simmode=2))
    ev = pkg.Eval(lib, g)
    wc = [dict() for _ in range(NL)]
    for h in range(2):
        s = pkg.Sim(lib, asm.fa[h], asm.bed[h], NL, sim_cases.FLEN, sim_cases.RLEN, sim_cases.CV, 1)
        s.attach(0)
        ev.truth_sim(s)
        nfr = int(s.info().nfrags)
        for first in range(0, nfr, 97):
            s.batch(first, min(97, nfr - first))
            s.align(ctx, sync=False)
        ctx.synchronize()
        s.close()
        wc = eval_model.add_counts(wc, eval_model.window_counts(asm.contigs[h], asm.beds[h], K, NL))
    want_x, want_w = eval_model.truth(wc, slots, g.ntrkmers)
    got = ev.score_ctx(ctx)
    y = ctx.counts()["counts"]
    assert y.any() and sum(want_x) > 0
    want = eval_model.sums(want_x, y.tolist(), beg, windows=want_w)
    assert got == want and sum(s["Sxy"] for s in want) > 0
    x, w = ev.truth()
    assert x.tolist() == want_x and w.tolist() == want_w
    ev.write(str(tmp_path / "lib"))
    assert open(tmp_path / "lib.eval.tsv").read() == eval_model.tsv_text(want) and open(tmp_path / "lib.pred").read() == eval_model.pred_text(want)
    # an evaluator of another RPGG build
    g2 = eval_cases.sized_rpgg(lib)
    ev2 = pkg.Eval(lib, g2)
    with pytest.raises(pkg.DbtkError) as e:
        ev2.score_ctx(ctx)
    assert e.value.status == abi.ERR_ARG and "RPGG" in str(e.value)
    ev2.close()
    g2.close()
    # pairs appended by dbtk_ingest_align_merged and not flushed
    fa = str(tmp_path / "il.fa")
    with open(fa, "w") as f:
        f.write(sim_model.annotated_fasta(asm.contigs[0], asm.beds[0], sim_cases.FLEN, sim_cases.RLEN, sim_cases.CV, 1))
    data = open(fa, "rb").read()
    ing = pkg.Ingest(ctx, False, 0, len(data) + 64, nslots=3, with_spans=False)
    s0 = ing.submit(data, True)
    assert ing.wait(s0).nkept > 0
    ing.align_merged(s0, 10 ** 9)
    with pytest.raises(pkg.DbtkError) as e:
        ev.score_ctx(ctx)
    assert e.value.status == abi.ERR_ARG and "dbtk_ingest_align_merged" in str(e.value)
    ing.align_merged(None, 0, flush=True)
    again = ev.score_ctx(ctx)
    assert sum(s["Sy"] for s in again) > sum(s["Sy"] for s in want)
    ing.close()
    ev.close()
    ctx.close()
    g.close()
