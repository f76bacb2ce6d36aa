"""Windowed dbtk_pred_t (include/dbtk_pred.h, "Windows"): whole loci of at most max_rows k-mers at a time must give the BYTES of the
whole-matrix handle — raw matrix, corrected matrix and Bias, NaN payloads included — through the fused pass (dbtk_pred_window_outputs)
and through the separate calls (load, matrix, correct, matrix) alike.

Against oracle/pred_oracle.py the tolerances are those of tests/test_pred.py: the raw matrix bit-exact, Bias and the corrected matrix
relative 2e-6 (the mean over the samples is a pairwise tree here and numpy's pairwise sum there)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import bind
from cases import make_case

sys.path.insert(0, os.path.join(bind.ROOT, "oracle"))
import pred_oracle as PO  # noqa: E402

pkg, abi = bind.pkg, bind.abi
RTOL = 2e-6

# locus sizes: empty loci at the start, two adjacent in the middle, at the end; 1, 2, the tile size of the load kernels and its
# neighbours, one locus of several tiles
SIZES = [0, 1, 2, 63, 64, 65, 7, 300, 12, 0, 0, 33, 5, 90, 64, 1, 18, 0, 128, 3, 40, 77, 2, 9, 0, 51, 66, 10, 4, 25, 31, 8, 70, 6, 14, 2, 19, 11, 0, 0]
NOINV = {4, 12, 21, 30}     # loci with k-mers and without invariant k-mers
ZERO_LOCUS = 13             # every invariant k-mer of this locus is uncounted in sample 0: Bias 0, corrected inf / NaN
LARGEST = max(SIZES)


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    same_kind = (np.isnan(a) == np.isnan(b)).all() and (np.isposinf(a) == np.isposinf(b)).all() and (np.isneginf(a) == np.isneginf(b)).all()
    return bool(same_kind and (np.abs(a[fin] - b[fin]) <= rtol * np.maximum(np.abs(a[fin]), np.abs(b[fin]))).all())


@functools.lru_cache(maxsize=None)
def cohort(ns):
    rng = np.random.default_rng(100 + ns)
    nks = np.asarray(SIZES)
    ntr = len(nks)
    nk_cum = np.cumsum(nks).astype(np.uint32)
    nk = int(nk_cum[-1])
    iki, ikmc, nik_cum = [], [], []
    for t in range(ntr):
        si, n = int(nk_cum[t]) - int(nks[t]), int(nks[t])
        m = 0 if (n == 0 or t in NOINV) else int(rng.integers(1, max(2, n // 2 + 1)))
        if t == 7:
            m = 150                                              # more invariant k-mers than one turn of the bias kernel holds
        sel = np.sort(rng.choice(n, m, replace=False)) + si if m else np.zeros(0, np.int64)
        iki += list(sel)
        ikmc += list(rng.integers(1, 5, m))
        nik_cum.append(len(iki))
    depths = (rng.uniform(8, 60, ns) + 0.37).astype(np.float32)  # no powers of two
    lam = rng.uniform(0.5, 3.0, nk)
    counts = rng.poisson(lam[None, :] * depths[:, None].astype(np.float64)).astype(np.uint64)
    counts[:, rng.integers(0, nk, 5)] += np.uint64(1) << np.uint64(40)          # counts beyond float32's integers
    meta = dict(nk=nk, nik=len(iki), ntr=ntr, nk_cum=nk_cum, nik_cum=np.asarray(nik_cum, np.uint32), iki=np.asarray(iki, np.uint32), ikmc=np.asarray(ikmc, np.uint8))
    a, b = (int(meta["nik_cum"][ZERO_LOCUS - 1]), int(meta["nik_cum"][ZERO_LOCUS]))
    assert b > a
    counts[0, meta["iki"][a:b]] = 0
    z0 = int(nk_cum[ZERO_LOCUS - 1])
    counts[0, z0 + [k for k in range(SIZES[ZERO_LOCUS]) if z0 + k not in set(meta["iki"][a:b])][0]] = 0   # a 0 / 0 among the x / 0
    counts.setflags(write=False)
    return meta, counts, depths


@functools.lru_cache(maxsize=None)
def whole(ns):
    """(raw, corrected, Bias) of the whole-matrix handle and of the oracle, made once per ns."""
    meta, counts, depths = cohort(ns)
    P = pkg.Pred(pkg.Dbtk(), ns, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"], nk=meta["nk"])
    P.load(0, counts, depths)
    raw = P.matrix()
    P.correct()
    cor, bias = P.matrix(), P.bias()
    P.close()
    raw_o = PO.raw_matrix(counts, depths)
    cor_o, bias_o = PO.bias_correction(raw_o, meta)
    for a in (raw, cor, bias, raw_o, cor_o, bias_o):
        a.setflags(write=False)
    return raw, cor, bias, raw_o, cor_o, bias_o


def windowed(ns, max_rows):
    meta, _, _ = cohort(ns)
    return pkg.PredWindowed(pkg.Dbtk(), ns, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"], max_rows, nk=meta["nk"])


def max_rows_cases():
    nk_cum = np.cumsum(SIZES)
    nk = int(nk_cum[-1])
    boundary = int(nk_cum[8])        # loci 0 .. 8 fill the first window exactly (>= LARGEST)
    return [LARGEST, boundary, boundary - 1, nk]


def test_the_cases_are_what_they_claim():
    nk_cum = np.cumsum(SIZES)
    assert len(SIZES) == 40 and SIZES[0] == 0 and SIZES[-1] == 0 and SIZES[9] == SIZES[10] == 0
    assert {0, 1, 2, 63, 64, 65, 300} <= set(SIZES)
    m = max_rows_cases()
    assert m[1] >= LARGEST and m[1] in nk_cum and m[2] not in nk_cum and m[3] == nk_cum[-1]


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [1, 3, 64, 70])
def test_windows_give_the_bytes_of_the_whole_matrix(ns):
    meta, counts, depths = cohort(ns)
    raw, cor, bias, raw_o, cor_o, bias_o = whole(ns)
    assert not np.isfinite(cor).all() and (bias[ZERO_LOCUS, 0] == 0 or ns == 1)     # the inf / NaN case is there
    assert raw.tobytes() == raw_o.tobytes() and close(cor, cor_o) and close(bias, bias_o)
    for max_rows in max_rows_cases():
        W = windowed(ns, max_rows)
        fused_raw, fused_cor, sep_raw, sep_cor, nwin, first = [], [], [], [], 0, 0
        one_locus_window = False
        while first < meta["ntr"]:
            end, row0, rows = W.window(first)
            assert end > first and rows <= W.max_rows and row0 == (int(meta["nk_cum"][first - 1]) if first else 0)
            assert row0 + rows == (meta["nk"] if end == meta["ntr"] else int(meta["nk_cum"][end - 1]))
            one_locus_window |= sum(1 for t in range(first, end) if SIZES[t]) == 1
            for s0 in range(0, ns, 23):                           # ragged transfers
                W.load(s0, counts[s0:s0 + 23, row0:row0 + rows], depths[s0:s0 + 23])
            r, c = W.outputs()                                    # the fused pass
            fused_raw.append(r); fused_cor.append(c)
            sep_raw.append(W.matrix())                            # the separate calls, on the same window
            W.correct()
            sep_cor.append(W.matrix())
            first, nwin = end, nwin + 1
        wbias = W.bias()
        W.close()
        assert nwin == (1 if max_rows == meta["nk"] else nwin) and (max_rows != LARGEST or one_locus_window)
        f_raw, f_cor, s_raw, s_cor = (np.concatenate(x) for x in (fused_raw, fused_cor, sep_raw, sep_cor))
        assert f_raw.tobytes() == raw.tobytes(), max_rows
        assert f_cor.tobytes() == cor.tobytes(), max_rows
        assert wbias.tobytes() == bias.tobytes(), max_rows
        assert s_raw.tobytes() == f_raw.tobytes() and s_cor.tobytes() == f_cor.tobytes(), max_rows
        assert f_raw.tobytes() == raw_o.tobytes() and close(f_cor, cor_o) and close(wbias, bias_o)


@pytest.mark.gpu
def test_submitted_window_runs_beside_the_next_ones_loads():
    """submit, open and load the next window, then take the outputs: the pipelined order of the command line."""
    ns = 3
    meta, counts, depths = cohort(ns)
    raw, cor, bias = whole(ns)[:3]
    W = windowed(ns, LARGEST)
    outs, first, pending = [], 0, False
    while first < meta["ntr"]:
        end, row0, rows = W.window(first)
        W.load(0, counts[:, row0:row0 + rows], depths)
        if pending:
            outs.append(W.outputs())
        W.submit()
        with pytest.raises(pkg.DbtkError) as e:                   # one submitted window at a time
            W._lib._chk(W._lib.L.dbtk_pred_window_submit(W.h))
        assert e.value.status == abi.ERR_ARG
        first, pending = end, True
    outs.append(W.outputs())
    assert np.concatenate([o[0] for o in outs]).tobytes() == raw.tobytes()
    assert np.concatenate([o[1] for o in outs]).tobytes() == cor.tobytes()
    assert W.bias().tobytes() == bias.tobytes()
    W.close()


@pytest.mark.gpu
def test_unvisited_loci_have_zero_bias_and_earlier_windows_keep_theirs():
    ns = 3
    meta, counts, depths = cohort(ns)
    bias = whole(ns)[2]
    W = windowed(ns, LARGEST)
    end, row0, rows = W.window(0)
    W.load(0, counts[:, row0:row0 + rows], depths)
    W.correct()
    b = W.bias()
    assert b[:end].tobytes() == bias[:end].tobytes() and (b[end:] == 0).all()
    end2, row0, rows = W.window(end)
    W.load(0, counts[:, row0:row0 + rows], depths)
    W.outputs()
    b = W.bias()
    assert b[:end2].tobytes() == bias[:end2].tobytes() and (b[end2:] == 0).all()
    W.close()


@pytest.mark.gpu
def test_load_order_and_reload():
    ns = 3
    meta, counts, depths = cohort(ns)
    raw, cor = whole(ns)[:2]
    W = windowed(ns, meta["nk"])
    _, row0, rows = W.window(0)
    assert (row0, rows) == (0, meta["nk"])
    W.load(1, counts[0:1], depths[2:3])                           # the wrong sample's counts and depth first: the later load wins
    assert W.matrix()[:, 1].tobytes() == (counts[0].astype(np.float32) / depths[2]).tobytes()
    for s in (2, 1, 0):                                           # reverse order
        W.load(s, counts[s:s + 1], depths[s:s + 1])
    assert W.matrix().tobytes() == raw.tobytes()
    r, c = W.outputs()
    assert r.tobytes() == raw.tobytes() and c.tobytes() == cor.tobytes()
    W.close()


@pytest.mark.gpu
def test_load_device_into_a_window():
    import torch
    ns = 3
    meta, counts, depths = cohort(ns)
    raw, cor = whole(ns)[:2]
    W = windowed(ns, LARGEST)
    first, outs = 0, []
    while first < meta["ntr"]:
        end, row0, rows = W.window(first)
        d = torch.from_numpy(np.ascontiguousarray(counts[:, row0:row0 + rows]).view(np.int64)).cuda()
        torch.cuda.synchronize()
        W.load_device(1, 2, d[1:], depths[1:])
        W.load_device(0, 1, d[:1], depths[:1])
        outs.append(W.outputs())
        first = end
    assert np.concatenate([o[0] for o in outs]).tobytes() == raw.tobytes()
    assert np.concatenate([o[1] for o in outs]).tobytes() == cor.tobytes()
    W.close()


@pytest.mark.gpu
def test_refusals(tmp_path):
    ns = 3
    meta, counts, depths = cohort(ns)
    with pytest.raises(pkg.DbtkError) as e:                       # a locus of max_rows + 1 k-mers
        windowed(ns, LARGEST - 1)
    assert e.value.status == abi.ERR_ARG and "locus 7 " in str(e.value) and "300" in str(e.value)
    with pytest.raises(pkg.DbtkError) as e:
        windowed(ns, 0)
    assert e.value.status == abi.ERR_ARG
    W = windowed(ns, LARGEST)
    for first in (meta["ntr"], meta["ntr"] + 5, 2 ** 40):
        with pytest.raises(pkg.DbtkError) as e:
            W.window(first)
        assert e.value.status == abi.ERR_ARG
    end, row0, rows = W.window(0)
    W.load(0, counts[:, row0:row0 + rows], depths)
    before = W.matrix()
    for s0, n in ((2, 2), (3, 1), (2 ** 40, 1)):                  # a load of the wrong sample range leaves the window alone
        with pytest.raises(pkg.DbtkError) as e:
            W.load(s0, np.full((n, rows), 7, np.uint64), np.ones(n, np.float32))
        assert e.value.status == abi.ERR_ARG
    assert W.matrix().tobytes() == before.tobytes()
    r, _ = W.outputs()
    assert r.tobytes() == before.tobytes()
    # a context holds one sample's whole vector: refused on a windowed handle
    dbtk = pkg.Dbtk()
    c = make_case("mixed", str(tmp_path))
    g = dbtk.load(c.prefix, c.k, c.qc_file)
    ctx = dbtk.context(g, abi.default_params(ksize=c.k, **dict(c.param_sets[0], okam=0)))
    with pytest.raises(pkg.DbtkError) as e:
        W.load_ctx(0, ctx, 1.0)
    assert e.value.status == abi.ERR_ARG and "windowed" in str(e.value)
    assert W.matrix().tobytes() == before.tobytes()
    ctx.close()
    W.close()
    # the window calls on a handle of dbtk_pred_create
    P = pkg.Pred(dbtk, ns, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"], nk=meta["nk"])
    L = dbtk.L
    L.dbtk_pred_window.argtypes = [C.c_void_p, C.c_uint64, bind.abi.u64p, bind.abi.u64p, bind.abi.u64p]
    assert L.dbtk_pred_window(P.h, 0, None, None, None) == abi.ERR_ARG
    assert L.dbtk_pred_window_submit(P.h) == abi.ERR_ARG
    P.close()
