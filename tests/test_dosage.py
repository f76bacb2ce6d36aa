"""The dosage tables (include/dbtk_pred.h, ABI v10) through ctypes: per sample and locus the exact k-mer sum, the bias and the
bias-corrected dosage, made from one pass over a sample's counts without the cohort matrix.

Bounds, and where they come from:
  kms      exact: uint64 sums against numpy's uint64 segment sums, and against the file the reference's `ktools sum -f` writes from
           the same counts as text.
  bias     BIT-IDENTICAL to dbtk_pred_bias after dbtk_pred_correct on the same counts and depths: the kernel takes the matrix path's
           operations in its order (conversion, / depth, / ikmc, adds sequential in j, / n) and the same normalisation kernel runs.
           Against oracle/pred_oracle.py: test_pred.py's RTOL = 2e-6 (the project's bound for its tree mean against another order).
  values   against the formula in float64 from the ORACLE's bias (never the device's): float64(kms) / float64(depth) / bias_o, relative
           2e-6 + 3 * 2^-24 — the bias bound plus one conversion and two divisions, each correctly rounded to float32 (2^-24 each).
           Loci without invariant k-mers (uncorrected) and loci without k-mers (0) exactly: float32(kms) / float32(depth), and 0.
Shapes: the four cohorts of tests/test_pred.py (loci without k-mers, loci without invariant k-mers, counts of 2^40), ns = 1, 37, 300,
and cohorts with loci of several thousand k-mers (more than one work item per locus: the partial sums and their fold)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bind
import synth
from cases import make_case
from test_pred import RTOL, close, make_cohort
from test_pred_device import _Hip, _bits, _meta

sys.path.insert(0, os.path.join(bind.ROOT, "oracle"))
import pred_oracle as PO  # noqa: E402

abi = bind.abi
pkg = bind.pkg
VTOL = RTOL + 3 * 2.0 ** -24

# (seed, ns, ntr, max_k): test_pred.py's four, then ns = 1 / 37 / 300 with large loci
SHAPES = [(3, 37, 50, 160), (4, 300, 20, 160), (5, 1, 8, 160), (6, 64, 400, 160), (13, 1, 9, 7000), (14, 37, 12, 9000), (15, 300, 6, 5000)]


def test_library_exports_the_dosage_abi():
    """(CPU) every dbtk_dosage_* the header declares is exported, and the ABI version says so."""
    import re
    hdr = open(os.path.join(bind.ROOT, "include", "dbtk_pred.h")).read()
    declared = set(re.findall(r"\b(dbtk_dosage_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(pkg.EXPORTS_DOSAGE), declared ^ set(pkg.EXPORTS_DOSAGE)
    lib = pkg.Dbtk()
    for s in declared:
        assert hasattr(lib.L, s), s
    assert abi.ABI_VERSION >= 10 and lib.L.dbtk_abi_version() == abi.ABI_VERSION


def segment_sums(counts, nk_cum):
    """uint64 [ntr][ns]: numpy's own segment sums (uint64 throughout, exact modulo 2^64)."""
    ns = counts.shape[0]
    c = np.concatenate([np.zeros((ns, 1), np.uint64), np.cumsum(counts, axis=1, dtype=np.uint64)], axis=1)
    e = np.asarray(nk_cum, np.int64)
    b = np.concatenate([np.zeros(1, np.int64), e[:-1]])
    return np.ascontiguousarray((c[:, e] - c[:, b]).T)


def skipped(meta):
    nk = np.diff(np.concatenate([[0], meta["nk_cum"].astype(np.int64)]))
    nik = np.diff(np.concatenate([[0], meta["nik_cum"].astype(np.int64)]))
    return nk == 0, (nk == 0) | (nik == 0)


def dosage(lib, ns, m):
    return pkg.Dosage(lib, ns, m["nk_cum"], m["nik_cum"], m["iki"], m["ikmc"], nk=m["nk"])


@pytest.fixture(scope="module")
def dbtk():
    return pkg.Dbtk()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,ns,ntr,max_k", SHAPES)
def test_tables_against_numpy_the_matrix_path_and_the_oracle(dbtk, seed, ns, ntr, max_k):
    meta, counts, depths = make_cohort(seed, ns=ns, ntr=ntr, max_k=max_k)
    empty, skip = skipped(meta)
    if max_k > 2048:
        assert (np.diff(np.concatenate([[0], meta["nk_cum"].astype(np.int64)])) > 2048).any()      # a locus of several work items
    D = dosage(dbtk, ns, meta)
    # 20 bytes per sample and locus, metadata and a work list of a few bytes per locus: nothing of size nk * ns
    assert D.nk == meta["nk"] and D.ntr == ntr and 20 * ntr * ns <= D.nbytes() < 20 * ntr * ns + 4 * ns + 128 * (ntr + meta["nik"]) + meta["nk"] // 16 + 4096
    for s0 in range(0, ns, 23):                                   # ragged transfers, 16 samples staged at a time inside
        D.load(s0, counts[s0:s0 + 23], depths[s0:s0 + 23])
    with pytest.raises(pkg.DbtkError) as e:                       # not finished yet
        D.bias()
    assert e.value.status == abi.ERR_ARG
    kms = D.kms()
    want = segment_sums(counts, meta["nk_cum"])
    assert kms.dtype == np.uint64 and kms.shape == (ntr, ns) and (kms == want).all()
    assert (kms >= np.uint64(1) << np.uint64(40)).any() and (kms[empty] == 0).all()
    # bias: the bits of the matrix path
    D.finish()
    P = pkg.Pred(dbtk, ns, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"], nk=meta["nk"])
    P.load(0, counts, depths)
    P.correct()
    bias = D.bias()
    assert (_bits(bias) == _bits(P.bias())).all()
    P.close()
    raw_o = PO.raw_matrix(counts, depths)
    _, bias_o = PO.bias_correction(raw_o, meta)
    assert close(bias, bias_o) and (bias[skip] == 0).all() and (bias_o[skip] == 0).all()
    # values
    val = D.values()
    v32 = kms.astype(np.float32) / depths[None, :]                # one conversion, one division
    assert (_bits(val[skip & ~empty]) == _bits(v32[skip & ~empty])).all() and (val[empty] == 0).all()
    on = ~skip
    assert on.any() and skip.any()
    with np.errstate(divide="ignore", invalid="ignore"):
        want64 = kms[on].astype(np.float64) / depths[None, :].astype(np.float64) / bias_o[on].astype(np.float64)
    assert close(val[on], want64, VTOL)
    D.finish()                                                    # again: the raw bias is kept, so nothing changes
    assert (_bits(D.bias()) == _bits(bias)).all() and (_bits(D.values()) == _bits(val)).all()
    t = D.times()
    assert t[0] > 0 and t[1] > 0
    D.close()


@pytest.mark.gpu
@pytest.mark.skipif(not synth.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("seed,ns,ntr,max_k", [(3, 37, 50, 160), (14, 5, 12, 9000)])
def test_kms_is_the_reference_sum_file(dbtk, tmp_path, seed, ns, ntr, max_k):
    """The same counts as text through the reference's `ktools sum -f`.  Leading empty loci are left out of the reference's index (it
    never emits a row for such a file: kmertools.cpp:100); their kms must be 0."""
    meta, counts, depths = make_cohort(seed, ns=ns, ntr=ntr, max_k=max_k)
    counts = counts[:, :] & np.uint64((1 << 41) - 1)
    D = dosage(dbtk, ns, meta)
    D.load(0, counts, depths)
    kms = D.kms()
    D.close()
    lead = int(np.argmax(meta["nk_cum"] > 0))
    assert (kms[:lead] == 0).all() and ntr - lead >= 2
    d = str(tmp_path)
    open(os.path.join(d, "x.ksi"), "w").write("".join("%d\n" % c for c in meta["nk_cum"][lead:]))
    with open(os.path.join(d, "files.txt"), "w") as f:
        for s in range(ns):
            fn = os.path.join(d, "s%d.txt" % s)
            open(fn, "w").write("".join("%d\n" % int(c) for c in counts[s]))
            f.write(fn + "\n")
    r = subprocess.run([synth.ref_tool("ktools"), "sum", "-f", os.path.join(d, "x.ksi"), os.path.join(d, "files.txt"), os.path.join(d, "ref.kms")], capture_output=True)
    assert r.returncode == 0, r.stderr
    mine = "".join("\t".join(str(int(kms[t, s])) for t in range(lead, ntr)) + "\n" for s in range(ns))
    assert mine == open(os.path.join(d, "ref.kms")).read()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,ns,ntr,max_k", [(5, 1, 8, 160), (3, 37, 50, 160), (15, 300, 6, 5000)])
def test_host_and_device_loads_agree_bit_for_bit(dbtk, seed, ns, ntr, max_k):
    """dbtk_dosage_load_device in reverse order, in pieces of 1 and of 5 samples, one column loaded twice (first with other counts
    and another depth: the later load wins) against dbtk_dosage_load_samples in one call."""
    meta, counts, depths = make_cohort(seed, ns=ns, ntr=ntr, max_k=max_k)
    hip = _Hip()
    d_counts = hip.put(counts)
    nk = meta["nk"]
    A, B = dosage(dbtk, ns, meta), dosage(dbtk, ns, meta)
    A.load(0, counts, depths)
    twice = ns // 2
    other = (twice + 1) % ns
    B.load_device(twice, 1, d_counts.value + other * nk * 8, depths[other:other + 1] * 3 + 1)
    if ns > 1:
        assert (B.kms()[:, twice] != A.kms()[:, twice]).any()
    s = ns
    while s > 0:                                                  # from the last sample down
        n = 1 if s % 2 else min(5, s)
        s -= n
        B.load_device(s, n, d_counts.value + s * nk * 8, depths[s:s + n])
    assert (A.kms() == B.kms()).all()
    A.finish(); B.finish()
    assert (_bits(A.bias()) == _bits(B.bias())).all() and (_bits(A.values()) == _bits(B.values())).all()
    # refusals of the device form: past the cohort, host memory
    before = B.kms()
    with pytest.raises(pkg.DbtkError) as e:
        B.load_device(ns, 1, d_counts.value, depths[:1])
    assert e.value.status == abi.ERR_ARG
    host = np.ones(nk, np.uint64)
    with pytest.raises(pkg.DbtkError) as e:
        B.load_device(0, 1, host.ctypes.data, depths[:1])
    assert e.value.status == abi.ERR_ARG
    with pytest.raises(pkg.DbtkError) as e:
        B.load(ns - 1, np.ones((2, nk), np.uint64), np.ones(2, np.float32))
    assert e.value.status == abi.ERR_ARG
    assert (B.kms() == before).all()
    B.finish()
    assert (_bits(A.bias()) == _bits(B.bias())).all()             # the refused calls touched neither the raw bias nor the depths
    assert (_bits(A.values()) == _bits(B.values())).all()
    hip.free(d_counts)
    A.close(); B.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [1, 37])
def test_load_ctx_equals_host_load_bit_for_bit(dbtk, tmp_path, ns):
    """As tests/test_pred_device.py does for the matrix: every sample a different batch on one context, columns loaded in REVERSE
    order from the context's accumulators, column ns // 2 loaded twice; against the host form fed dbtk_ctx_counts' vector, and
    against a handle made from the RPGG itself (the --kms form: same sums, no bias)."""
    c = make_case("mixed", str(tmp_path))
    g = dbtk.load(c.prefix, c.k, c.qc_file)
    nk = g.ntrkmers
    seq, off = c.reads.packed()
    p = abi.default_params(ksize=c.k, **dict(c.param_sets[0], okam=0))
    ctx = dbtk.context(g, p)
    m = _meta(nk, 11 + ns)
    depths = np.random.default_rng(ns).uniform(0.5, 60.0, ns).astype(np.float32)
    npairs = c.reads.npairs
    counts = np.zeros((ns, nk), np.uint64)
    D_ctx, D_host, D_g = dosage(dbtk, ns, m), dosage(dbtk, ns, m), pkg.Dosage(dbtk, ns, rpgg=g)
    assert D_g.nk == nk and D_g.ntr == g.nloci

    def align_sample(s):
        ctx.reset()
        ctx.align(seq, off[:2 * (1 + (s * 97 + 400) % npairs) + 1])

    for s in reversed(range(ns)):
        if s == ns // 2:
            align_sample(s + 1)
            D_ctx.load_ctx(s, ctx, float(depths[s]) * 3 + 1)
        align_sample(s)
        counts[s] = ctx.counts()["counts"]
        D_ctx.load_ctx(s, ctx, float(depths[s]))
        D_g.load_ctx(s, ctx, 1.0)
        ctx.reset()                                               # safe right after load_ctx
    assert counts.any()
    D_host.load(0, counts, depths)
    assert (D_ctx.kms() == D_host.kms()).all() and (D_ctx.kms() == segment_sums(counts, m["nk_cum"])).all()
    D_ctx.finish(); D_host.finish(); D_g.finish()
    assert (_bits(D_ctx.bias()) == _bits(D_host.bias())).all() and (_bits(D_ctx.values()) == _bits(D_host.values())).all()
    # the RPGG form: the loci of the RPGG's own output order, every locus uncorrected
    kg = D_g.kms()
    assert kg.shape == (g.nloci, ns) and (kg.sum(axis=0) == counts.sum(axis=1)).all()
    assert not D_g.bias().any() and (_bits(D_g.values()) == _bits(kg.astype(np.float32))).all()
    for D in (D_ctx, D_host, D_g):
        D.close()
    ctx.close(); g.close()


@pytest.mark.gpu
def test_load_ctx_refusals_leave_the_tables_untouched(dbtk, tmp_path):
    """The refusals of dbtk_pred_load_ctx, one by one (tests/test_pred_device.py: test_load_ctx_error_paths), on a handle that
    already holds a sample: kms, bias and values keep their bits."""
    c = make_case("mixed", str(tmp_path))
    g = dbtk.load(c.prefix, c.k, c.qc_file)
    nk = g.ntrkmers
    seq, off = c.reads.packed()
    p = abi.default_params(ksize=c.k, **dict(c.param_sets[0], okam=0))
    ctx = dbtk.context(g, p)
    ctx.align(seq, off)
    want = ctx.counts()["counts"]
    m = _meta(nk, 3)
    D = dosage(dbtk, 4, m)
    D.load_ctx(0, ctx, 7.5)
    D.finish()
    k0, b0, v0 = D.kms(), D.bias(), D.values()
    assert k0[:, 0].any() and not k0[:, 1:].any()

    def untouched():
        assert (D.kms() == k0).all()
        D.finish()
        assert (_bits(D.bias()) == _bits(b0)).all() and (_bits(D.values()) == _bits(v0)).all()

    # another RPGG build: nk differs
    D1 = dosage(dbtk, 4, _meta(nk + 1, 3))
    with pytest.raises(pkg.DbtkError) as e:
        D1.load_ctx(0, ctx, 1.0)
    assert e.value.status == abi.ERR_ARG and "RPGG" in str(e.value)
    assert not D1.kms().any()
    D1.close()
    for s in (4, 5, 2 ** 40):                                    # sample >= ns
        with pytest.raises(pkg.DbtkError) as e:
            D.load_ctx(s, ctx, 1.0)
        assert e.value.status == abi.ERR_ARG
    untouched()
    hipdll = C.CDLL("libamdhip64.so")
    ndev = C.c_int(0)
    hipdll.hipGetDeviceCount(C.byref(ndev))
    if ndev.value > 1:                                           # a handle on another device (needs two GPUs to be asked at all)
        D2 = pkg.Dosage(dbtk, 4, m["nk_cum"], m["nik_cum"], m["iki"], m["ikmc"], nk=nk, device=1)
        with pytest.raises(pkg.DbtkError) as e:
            D2.load_ctx(0, ctx, 1.0)
        assert e.value.status == abi.ERR_ARG and "device" in str(e.value)
        assert not D2.kms().any()
        D2.close()
    # a pending sticky error word, returned once instead of loading
    hip = _Hip()
    d_seq, d_off = hip.put(seq, 64), hip.put(off)
    ctx.reset()
    ctx.align_device(d_seq.value, d_off.value, c.reads.npairs, 100)   # the reads are 150 bases
    with pytest.raises(pkg.DbtkError) as e:
        D.load_ctx(1, ctx, 2.0)
    assert e.value.status == abi.ERR_READ_TOO_LONG
    untouched()
    ctx.reset()
    hip.free(d_seq); hip.free(d_off)
    # pairs appended by dbtk_ingest_align_merged and not flushed
    fa = str(tmp_path / "reads_il.fa")
    synth.write_fasta(c.reads, fa)
    data = open(fa, "rb").read()
    ing = pkg.Ingest(ctx, False, 0, len(data) + 64, nslots=3, with_spans=False)
    s0 = ing.submit(data, True)
    info = ing.wait(s0)
    assert info.flags == 0 and info.nkept > 0
    ing.align_merged(s0, 10 ** 9)
    with pytest.raises(pkg.DbtkError) as e:
        D.load_ctx(2, ctx, 2.0)
    assert e.value.status == abi.ERR_ARG and "dbtk_ingest_align_merged" in str(e.value)
    untouched()
    ing.align_merged(None, 0, flush=True)
    D.load_ctx(2, ctx, 2.0)
    got = ctx.counts()["counts"]
    ing.close()
    assert (got == want).all()
    k = D.kms()
    assert (k[:, 2] == segment_sums(got[None, :], m["nk_cum"])[:, 0]).all() and (k[:, 0] == k0[:, 0]).all() and not k[:, 1].any()
    D.close(); ctx.close(); g.close()
