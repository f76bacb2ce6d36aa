"""dbtk_pred_load_ctx / dbtk_pred_load_device (include/dbtk_pred.h, ABI v9): a sample's counts go from the aligner's accumulators
(or any device buffer) into the genotype matrix without leaving HBM.

What is asserted, and why these bounds: the arithmetic is one uint64 -> float32 conversion and one float32 division, both correctly
rounded, exactly as dbtk_pred_load_samples does them — so the matrix must be equal BIT FOR BIT (compared as uint32 views) to the one
loaded from the host with the same counts, and to oracle/pred_oracle.py: raw_matrix.  No tolerance anywhere in this file."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import bind
import synth
from cases import make_case

sys.path.insert(0, os.path.join(bind.ROOT, "oracle"))
import pred_oracle as PO  # noqa: E402

abi = bind.abi
pkg = bind.pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dbtk():
    return pkg.Dbtk()


def _meta(nk, seed):
    """Any ikmer.meta over nk k-mers will do for the raw matrix: a handful of loci, a few invariant k-mers."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, nk), 6, replace=False))
    nk_cum = np.append(cuts, nk).astype(np.uint32)
    iki, nik_cum = [], []
    for t in range(len(nk_cum)):
        si = int(nk_cum[t - 1]) if t else 0
        iki += list(np.sort(rng.choice(np.arange(si, int(nk_cum[t])), min(3, int(nk_cum[t]) - si), replace=False)))
        nik_cum.append(len(iki))
    return dict(nk=nk, nk_cum=nk_cum, nik_cum=np.array(nik_cum, np.uint32), iki=np.array(iki, np.uint32),
                ikmc=rng.integers(1, 4, len(iki)).astype(np.uint8))


def _pred(dbtk, ns, m):
    return pkg.Pred(dbtk, ns, m["nk_cum"], m["nik_cum"], m["iki"], m["ikmc"], nk=m["nk"])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class _Hip:
    def __init__(self):
        h = self.h = C.CDLL("libamdhip64.so")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipFree.argtypes = [C.c_void_p]

    def put(self, arr, pad=0):
        d = C.c_void_p()
        assert self.h.hipMalloc(C.byref(d), arr.nbytes + pad) == 0
        assert self.h.hipMemcpy(d, arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1) == 0
        return d

    def free(self, d):
        self.h.hipFree(d)


@pytest.mark.parametrize("ns", [1, 37, 300])
def test_load_ctx_equals_host_load_bit_for_bit(dbtk, tmp_path, ns):
    """ns = 1, 37, 300 (one column; a ragged tile; several tiles of the host form) over nk = 1092 k-mers (not a multiple of 64).
    Every sample is a different batch aligned on one context that is reset in between; the columns are loaded in REVERSE order,
    and column ns // 2 is loaded twice (first with another sample's counts and another depth: the later load must win)."""
    c = make_case("mixed", str(tmp_path))
    g = dbtk.load(c.prefix, c.k, c.qc_file)
    nk = g.ntrkmers
    assert nk % 64 != 0
    seq, off = c.reads.packed()
    p = abi.default_params(ksize=c.k, **dict(c.param_sets[0], okam=0))
    ctx = dbtk.context(g, p)
    m = _meta(nk, 11 + ns)
    rng = np.random.default_rng(ns)
    depths = rng.uniform(0.5, 60.0, ns).astype(np.float32)
    npairs = c.reads.npairs
    counts = np.zeros((ns, nk), np.uint64)
    P_ctx, P_host = _pred(dbtk, ns, m), _pred(dbtk, ns, m)

    def align_sample(s):
        n = 1 + (s * 97 + 400) % npairs                          # a different prefix of the reads per sample
        ctx.reset()
        ctx.align(seq, off[:2 * n + 1])

    twice = ns // 2
    for s in reversed(range(ns)):
        if s == twice:                                           # a first load of this column that must be overwritten
            align_sample(s + 1)
            P_ctx.load_ctx(s, ctx, float(depths[s]) * 3 + 1)
        align_sample(s)
        counts[s] = ctx.counts()["counts"]
        P_ctx.load_ctx(s, ctx, float(depths[s]))
        ctx.reset()                                              # safe right after load_ctx: the accumulators are no longer read
    assert counts.any() and (ns < 3 or len({counts[s].tobytes() for s in range(ns)}) > 2)
    P_host.load(0, counts, depths)
    a, b = P_ctx.matrix(), P_host.matrix()
    assert a.shape == (nk, ns)
    assert (_bits(a) == _bits(b)).all()
    assert (_bits(a) == _bits(PO.raw_matrix(counts, depths))).all()
    # ... and what follows reads the same matrix
    P_ctx.correct(); P_host.correct()
    assert (_bits(P_ctx.matrix()) == _bits(P_host.matrix())).all() and (_bits(P_ctx.bias()) == _bits(P_host.bias())).all()
    P_ctx.close(); P_host.close(); ctx.close(); g.close()


@pytest.mark.parametrize("ns,n", [(1, 1), (37, 1), (37, 5), (300, 70)])
def test_load_device_counts_above_2_24(dbtk, ns, n):
    """Counts planted in a device buffer, among them values a float32 cannot hold exactly (2^24 + 1, 2^40 + 12345, 2^63 + 2^39 + 1,
    2^64 - 1): n = 1 takes the column kernel, n > 1 the tiles; first_sample > 0; nk = 1037 (not a multiple of 64)."""
    nk = 1037
    m = _meta(nk, 5)
    rng = np.random.default_rng(ns * 1000 + n)
    counts = rng.integers(0, 5000, (n, nk)).astype(np.uint64)
    big = np.array([2 ** 24 + 1, 2 ** 24 + 3, 2 ** 40 + 12345, 2 ** 63 + 2 ** 39 + 1, 2 ** 64 - 1, 2 ** 53 + 1], np.uint64)
    for i in range(n):
        counts[i, rng.choice(nk - 1, len(big), replace=False)] = big
    counts[0, nk - 1] = big[0]                                   # the last k-mer: the edge of the last tile / block
    depths = rng.uniform(0.5, 60.0, n).astype(np.float32)
    first = ns - n
    hip = _Hip()
    d = hip.put(counts)
    P_dev, P_host = _pred(dbtk, ns, m), _pred(dbtk, ns, m)
    P_dev.load_device(first, n, d.value, depths)
    P_host.load(first, counts, depths)
    a = P_dev.matrix()
    assert (_bits(a) == _bits(P_host.matrix())).all()
    want = np.zeros((nk, ns), np.float32)
    want[:, first:] = PO.raw_matrix(counts, depths)
    assert (_bits(a) == _bits(want)).all()
    with pytest.raises(pkg.DbtkError) as e:                      # past the cohort
        P_dev.load_device(first + 1, n, d.value, depths)
    assert e.value.status == abi.ERR_ARG
    hip.free(d)
    host = np.zeros(nk, np.uint64)
    with pytest.raises(pkg.DbtkError) as e:                      # host memory is dbtk_pred_load_samples' business
        P_dev.load_device(0, 1, host.ctypes.data, depths[:1])
    assert e.value.status == abi.ERR_ARG
    P_dev.close(); P_host.close()


def test_load_ctx_error_paths(dbtk, tmp_path):
    c = make_case("mixed", str(tmp_path))
    g = dbtk.load(c.prefix, c.k, c.qc_file)
    nk = g.ntrkmers
    seq, off = c.reads.packed()
    p = abi.default_params(ksize=c.k, **dict(c.param_sets[0], okam=0))
    ctx = dbtk.context(g, p)
    ctx.align(seq, off)
    want = ctx.counts()["counts"]
    # another RPGG build: nk differs
    P1 = _pred(dbtk, 4, _meta(nk + 1, 3))
    with pytest.raises(pkg.DbtkError) as e:
        P1.load_ctx(0, ctx, 1.0)
    assert e.value.status == abi.ERR_ARG and "RPGG" in str(e.value)
    P1.close()
    P = _pred(dbtk, 4, _meta(nk, 3))
    for s in (4, 5, 2 ** 40):
        with pytest.raises(pkg.DbtkError) as e:
            P.load_ctx(s, ctx, 1.0)
        assert e.value.status == abi.ERR_ARG
    assert not P.matrix().any()                                  # nothing was written by the refused calls
    # a pending sticky error word: a read longer than the promised max_read_len (as tests/test_gpu_parity.py raises it)
    hip = _Hip()
    d_seq, d_off = hip.put(seq, 64), hip.put(off)
    ctx.reset()
    ctx.align_device(d_seq.value, d_off.value, c.reads.npairs, 100)   # the reads are 150 bases
    with pytest.raises(pkg.DbtkError) as e:
        P.load_ctx(1, ctx, 2.0)
    assert e.value.status == abi.ERR_READ_TOO_LONG
    assert not P.matrix().any()                                  # the tainted counts were not loaded
    ctx.reset()
    hip.free(d_seq); hip.free(d_off)
    # pairs appended by dbtk_ingest_align_merged and not flushed: refused (include/dbtk_pred.h), never silently missed
    fa = str(tmp_path / "reads_il.fa")
    synth.write_fasta(c.reads, fa)
    data = open(fa, "rb").read()
    ing = pkg.Ingest(ctx, False, 0, len(data) + 64, nslots=3, with_spans=False)
    s0 = ing.submit(data, True)
    info = ing.wait(s0)
    assert info.flags == 0 and info.nkept > 0
    ing.align_merged(s0, 10 ** 9)                                # appended, not aligned
    with pytest.raises(pkg.DbtkError) as e:
        P.load_ctx(2, ctx, 2.0)
    assert e.value.status == abi.ERR_ARG and "dbtk_ingest_align_merged" in str(e.value)
    assert not P.matrix().any()
    ing.align_merged(None, 0, flush=True)
    P.load_ctx(2, ctx, 2.0)
    got = ctx.counts()["counts"]
    ing.close()
    assert got.any() and (got == want).all()                     # (the device reader handed on the same pairs)
    col = P.matrix()[:, 2]
    assert (_bits(col) == _bits(got.astype(np.float32) / np.float32(2.0))).all()
    P.close(); ctx.close(); g.close()
