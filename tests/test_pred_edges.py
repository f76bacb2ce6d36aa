"""danbing-tk-pred, its windowed form and the dosage tables PAST the sizes at which their kernels change what they do
(danbing-tk_amd/csrc/dbtk_pred.hip; the table of DESIGN 7).  The other pred tests stay below every one of these thresholds:

  (a) pred_tile / launch_tile    gy = min(ceil(n / PT_S), 64): more than 2048 samples in one launch and a block's i0 loop takes a second,
                                 possibly ragged, step (k_pred_load with n = ns; k_pred_wfused always runs with n = ns)
  (b) k_pred_load_col            nb = min(ceil(nk / 256), 65536): past 2^24 k-mers the grid-stride loop takes a second step
  (c) k_dosage_sample            more than DS_T loci in a work item (a second pass of the kms loop, a second `lg` group with its own
                                 J0 / J1); more than DS_TB invariant k-mers in a whole-loci item (a second turn of terms[], a locus cut
                                 by lo / hi); k_dosage_fold with more than 64 folded loci (a second block)
  (d) IEEE inputs                depth 0, ikmc 0, a locus whose mean bias is 0, a sample whose bias is 0: through all three paths
                                 (test_pred.py: make_cohort draws every depth from 8 .. 60 and every ikmc from 1 .. 4, whatever its
                                 docstring says of a zero-depth column: no other pred test feeds a zero)
  (e) columns of no locus        nk > nk_cum[ntr - 1]: they travel with the last window and are copied uncorrected
  (f) the command line           (a) at ns = 2081 through bin/danbing-tk-pred, with and without --window-rows

test_the_cases_are_what_they_claim (CPU) reads the constants from the source text and restates the packing rule of
dbtk_pred_plan::dosage_items, so that a changed constant fails here instead of silently ending the coverage.

References and bounds.  None of them comes from running the code under test.
  raw matrix   bit for bit against oracle/pred_oracle.py: raw_matrix (one conversion and one division, both correctly rounded).
  two device paths that take the same operations in the same order (whole matrix, windowed fused pass, windowed separate calls; the
               dosage tables' Bias and the matrix path's Bias): equal as uint32 views, NaN payloads included.
  kms          exact uint64, against numpy's segment sums.
  Bias, corrected matrix, dosage values: against the formulas of pred.h:212-233 evaluated in float64 on the float32 raw matrix (what
               test_pred.py: test_oracle_against_the_formulas_in_float64 does for the oracle), within a bound that is derived, not tuned.
               Let u = 2^-24 (float32's unit roundoff), n_i the locus' invariant k-mers, T = ceil(ns / 256).  Every summand is
               non-negative, so relative errors do not amplify through the sums, and to first order:
                 raw bias of a sample   (n_i + 1) u      one division per term (raw / ikmc), n_i - 1 effective adds, one division by n_i
                 mean over the samples  (n_i + 1) u of its inputs, + (T + 8) u of its own: T - 1 sequential adds per thread of
                                        k_pred_bias_norm, 8 levels of its tree over 256 partial sums, one division by ns
                 Bias = raw / mean      + u
               so |Bias - Bias64| <= (2 n_i + T + 11) u |Bias64|.  The corrected matrix (raw / Bias) takes one more u; a dosage value
               ((float)kms / depth / Bias) three more.  The bound is computed per locus.  (The float32 oracle's own Bias lies at
               0.10 - 0.14 of it at ns = 2049, 2081, 4131: the inputs leave room.)  NaN, +inf and -inf must stand where the float64
               reference has them: the "same kind" rule of test_pred.py: close.
  RTOL = 2e-6 against the float32 oracle is asserted where it is today, at ns <= 300 (here: case d), and NOT at ns > 2048: nobody
               has measured the kernel's tree mean against numpy's pairwise sum there.

PARITY UNPINNED against the reference itself: pred.cpp needs Eigen, which is not available to this project's builds."""
import filecmp
import functools
import math
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import bind
from test_dosage import segment_sums
from test_pred import RTOL, close
from test_pred_device import _Hip, _bits

sys.path.insert(0, os.path.join(bind.ROOT, "oracle"))
import pred_oracle as PO  # noqa: E402

pkg = bind.pkg
U = 2.0 ** -24
CSRC = os.path.join(bind.ROOT, "danbing-tk_amd", "csrc")
EXE = os.path.join(bind.ROOT, "danbing-tk_amd", "bin", "danbing-tk-pred")

A_SIZES = [0, 5, 64, 0, 65, 31, 1, 0]      # locus sizes of (a) and (d): the tile's 64 k-mers and its neighbour, 1, empty loci at both ends
A_NOINV = 5                                # ... its locus with k-mers and without invariant k-mers
A_TAIL = 3                                 # ... and its columns of no locus
A_NS = [2048, 2049, 2081, 4131]            # one full pass of the 64 x PT_S grid, one over, a ragged second step, a third step
B_NK = (1 << 24) + 257
B_SIZES = [40, (1 << 24) - 60, 50, 150, 60]   # loci 0, 2 and 4 are corrected: at the start, across row 2^24, at the end (+ 17 columns of no locus)
C_SIZES = [0] * 300 + [1] * 40 + [0, 2, 0, 0, 3] * 60 + [60] * 34 + [2048, 2049, 0, 4096, 4097] + [2049] * 66 + [5, 0, 0]
C_TAIL = 37
C_MAX_ROWS = 4097
D_NS = 70
D_VARIANTS = ["depth0", "ikmc0", "zero_locus", "zero_sample", "all"]
E_SIZES = [0, 5, 64, 0, 130, 31, 1, 0, 20]    # the last window: loci 6 .. 8 and the 100 columns of no locus
E_TAIL = 100


# ---------------------------------------------------------------- the cases ---
def spans(meta):
    """(t, si, ei, isi, iei) of every locus."""
    nkc, nikc = meta["nk_cum"].astype(np.int64), meta["nik_cum"].astype(np.int64)
    for t in range(len(nkc)):
        yield t, (int(nkc[t - 1]) if t else 0), int(nkc[t]), (int(nikc[t - 1]) if t else 0), int(nikc[t])


def make_meta(sizes, tail, n_inv, rng):
    """ikmer.meta over the given locus sizes and `tail` columns of no locus; n_inv(t, n, rng) = locus t's invariant k-mers."""
    nks = np.asarray(sizes, np.int64)
    nk_cum = np.cumsum(nks)
    iki, nik_cum = [], []
    for t, n in enumerate(nks):
        m = int(n_inv(t, int(n), rng))
        assert 0 <= m <= n
        iki.append(np.sort(rng.choice(int(n), m, replace=False)) + int(nk_cum[t] - n) if m else np.zeros(0, np.int64))
        nik_cum.append((nik_cum[-1] if nik_cum else 0) + m)
    iki = np.concatenate(iki).astype(np.uint32)
    return dict(nk=int(nk_cum[-1]) + tail, nik=len(iki), ntr=len(nks), nk_cum=nk_cum.astype(np.uint32), nik_cum=np.asarray(nik_cum, np.uint32), iki=iki,
                ikmc=rng.integers(1, 5, len(iki)).astype(np.uint8))


def make_counts(meta, ns, rng):
    depths = (rng.uniform(8, 60, ns) + 0.37).astype(np.float32)   # no powers of two
    lam = rng.uniform(0.5, 3.0, meta["nk"])
    counts = rng.poisson(lam[None, :] * depths[:, None].astype(np.float64)).astype(np.uint64)
    counts[:, rng.integers(0, meta["nk"], 5)] += np.uint64(1) << np.uint64(40)   # counts beyond float32's integers
    return counts, depths


def a_inv(t, n, rng):
    return 0 if n == 0 or t == A_NOINV else int(rng.integers(1, n + 1))


@functools.lru_cache(maxsize=None)
def cohort_a(ns):
    rng = np.random.default_rng(7000 + ns)
    meta = make_meta(A_SIZES, A_TAIL, a_inv, rng)
    counts, depths = make_counts(meta, ns, rng)
    counts.setflags(write=False)
    return meta, counts, depths


@functools.lru_cache(maxsize=None)
def cohort_b():
    rng = np.random.default_rng(24)
    meta = make_meta(B_SIZES, B_NK - sum(B_SIZES), lambda t, n, r: 0 if t % 2 else int(r.integers(3, 9)), rng)
    counts = rng.integers(1, 1000, size=(2, B_NK), dtype=np.uint64)   # (no zeros: a row the kernel never wrote stays 0 and shows)
    big = [(1 << 24) + 1, (1 << 40) + 12345, (1 << 64) - 1]     # rounds to even; beyond float32's integers; the largest count
    for rows in ([5, (1 << 24) + 3, B_NK - 1], [(1 << 24) + 7, 1 << 23, 0], [B_NK - 70, 17, (1 << 24) - 1]):
        for r, v in zip(rows, big):
            counts[:, r] = np.uint64(v)
    depths = np.asarray([23.37, 41.61], np.float32)
    counts.setflags(write=False)
    return meta, counts, depths


def c_inv(t, n, rng):
    if n == 0 or t % 7 == 3:
        return 0
    if n == 60:
        return n
    if n >= 2048:
        return (1, 1500, n)[t % 3]
    return int(rng.integers(1, n + 1))


@functools.lru_cache(maxsize=None)
def cohort_c(ns):
    rng = np.random.default_rng(300 + ns)
    meta = make_meta(C_SIZES, C_TAIL, c_inv, rng)
    counts, depths = make_counts(meta, ns, rng)
    counts.setflags(write=False)
    return meta, counts, depths


@functools.lru_cache(maxsize=None)
def cohort_d(variant):
    """(a)'s metadata at ns = 70 with the IEEE inputs of the issue, each alone and all together."""
    rng = np.random.default_rng(70)
    meta = make_meta(A_SIZES, A_TAIL, a_inv, rng)
    counts, depths = make_counts(meta, D_NS, rng)
    inv = {t: meta["iki"][isi:iei] for t, _, _, isi, iei in spans(meta)}
    on = lambda v: variant in (v, "all")  # noqa: E731
    if on("depth0"):
        depths[11] = 0.0                                          # x / 0, and 0 / 0 below
        counts[11, int(meta["nk_cum"][1]) + 3] = 0
    if on("ikmc0"):
        meta["ikmc"][int(meta["nik_cum"][3])] = 0                 # the first invariant k-mer of locus 4
    if on("zero_locus"):
        counts[:, inv[1]] = 0                                     # mean bias 0: the whole locus is NaN
    if on("zero_sample"):
        counts[29, inv[2]] = 0                                    # bias 0 for one sample: its column is inf, or NaN where the count is 0
        free = [k for k in range(int(meta["nk_cum"][1]), int(meta["nk_cum"][2])) if k not in set(inv[2].tolist())]
        assert len(free) > 1 and counts[29, free[1]] > 0
        counts[29, free[0]] = 0
    counts.setflags(write=False)
    return meta, counts, depths


@functools.lru_cache(maxsize=None)
def cohort_e():
    rng = np.random.default_rng(5)
    meta = make_meta(E_SIZES, E_TAIL, a_inv, rng)
    counts, depths = make_counts(meta, 37, rng)
    counts.setflags(write=False)
    return meta, counts, depths


def largest_locus(meta):
    """As the window planning sees it: the columns of no locus travel with the last locus."""
    n = np.diff(np.concatenate([[0], meta["nk_cum"].astype(np.int64)]))
    return int(max(n.max(), n[-1] + meta["nk"] - int(meta["nk_cum"][-1])))


# ------------------------------------------------------- references, bounds ---
def bias_bound(n_i, ns):
    return (2 * n_i + math.ceil(ns / 256) + 11) * U


def bias64(meta, raw):
    """Bias[ntr][ns] by pred.h:217-229 in float64 on the float32 raw matrix (skipped loci: 0), and the per-locus bound."""
    ns = raw.shape[1]
    out, bound = np.zeros((meta["ntr"], ns)), np.zeros(meta["ntr"])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for t, si, ei, isi, iei in spans(meta):
            if si == ei or isi == iei:
                continue
            B = raw[meta["iki"][isi:iei].astype(np.int64)].astype(np.float64) / meta["ikmc"][isi:iei, None].astype(np.float64)
            b = B.sum(axis=0) / (iei - isi)
            out[t] = b / (b.sum() / ns)
            bound[t] = bias_bound(iei - isi, ns)
    return out, bound


def within(got, want, bound, what):
    """|got - want| <= bound * |want| where want is finite; NaN, +inf and -inf where want has them.  Prints the largest error as a
    fraction of the bound before it judges."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    kinds = all((f(got) == f(want)).all() for f in (np.isnan, np.isposinf, np.isneginf))
    fin = np.isfinite(want) & np.isfinite(got)
    err, lim = np.abs(got[fin] - want[fin]), bound[fin] * np.abs(want[fin])
    nz = lim > 0
    worst = float((err[nz] / lim[nz]).max()) if nz.any() else 0.0
    print(f"{what}: largest error {worst:.3f} of the bound, same kinds: {kinds}")
    return bool(kinds and (err <= lim).all())


def corrected_within(meta, raw, cor, b64, bound, what, row0=0, rows=None):
    """cor[r - row0] against raw / Bias64 within the locus' bound + u on the rows of corrected loci, the bits of raw on all others."""
    rows = raw.shape[0] - row0 if rows is None else rows
    copied = np.ones(rows, bool)
    ok = True
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for t, si, ei, isi, iei in spans(meta):
            if si == ei or isi == iei or ei <= row0 or si >= row0 + rows:
                continue
            copied[si - row0:ei - row0] = False
            ok &= within(cor[si - row0:ei - row0], raw[si:ei].astype(np.float64) / b64[t][None, :], bound[t] + U, f"{what}, locus {t}")
    ok &= bool((_bits(cor)[copied] == _bits(raw[row0:row0 + rows])[copied]).all())
    return ok


def skipped(meta):
    e = np.asarray([si == ei for _, si, ei, _, _ in spans(meta)])
    s = np.asarray([si == ei or isi == iei for _, si, ei, isi, iei in spans(meta)])
    return e, s


# ----------------------------------------------------------- the device paths ---
def pred(ns, m):
    return pkg.Pred(pkg.Dbtk(), ns, m["nk_cum"], m["nik_cum"], m["iki"], m["ikmc"], nk=m["nk"])


def whole_matrix(meta, counts, depths, device=False):
    """(raw, corrected, Bias) of a whole-matrix handle, loaded in ONE call: n = ns in one launch."""
    ns = len(depths)
    P = pred(ns, meta)
    if device:
        hip = _Hip()
        d = hip.put(counts)
        P.load_device(0, ns, d.value, depths)
        hip.free(d)
    else:
        P.load(0, counts, depths)
    raw = P.matrix()
    P.correct()
    out = raw, P.matrix(), P.bias()
    P.close()
    return out


def windows(meta, counts, depths, max_rows):
    """All windows of a windowed handle: the fused pass' (raw, corrected), the separate calls' (raw, corrected), Bias, and the windows
    as (first locus, end, row0, rows)."""
    ns = len(depths)
    W = pkg.PredWindowed(pkg.Dbtk(), ns, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"], max_rows, nk=meta["nk"])
    parts, wins, first = [[], [], [], []], [], 0
    while first < meta["ntr"]:
        end, row0, rows = W.window(first)
        W.load(0, counts[:, row0:row0 + rows], depths)
        r, c = W.outputs()                                        # k_pred_wfused, n = ns
        sr = W.matrix()                                           # pred_window_materialize: k_pred_load, n = ns
        W.correct()
        for p, x in zip(parts, (r, c, sr, W.matrix())):
            p.append(x)
        wins.append((first, end, row0, rows))
        first = end
    bias = W.bias()
    W.close()
    return [np.concatenate(p) for p in parts] + [bias, wins]


def dosage_tables(meta, counts, depths, order=None):
    ns = len(depths)
    D = pkg.Dosage(pkg.Dbtk(), ns, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"], nk=meta["nk"])
    if order is None:
        D.load(0, counts, depths)
    else:
        for s, c, d in order:
            D.load(s, counts[c:c + 1], depths[d:d + 1])
    kms = D.kms()
    D.finish()
    out = kms, D.bias(), D.values()
    D.close()
    return out


def check_dosage(meta, counts, depths, kms, bias, val, b64, bound, what):
    empty, skip = skipped(meta)
    assert (kms == segment_sums(counts, meta["nk_cum"])).all()
    assert within(bias, b64, bound[:, None], f"{what}: dosage Bias") and (bias[skip] == 0).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        v32 = kms.astype(np.float32) / depths[None, :]
        want = kms.astype(np.float64) / depths[None, :].astype(np.float64) / b64
    assert (_bits(val[skip & ~empty]) == _bits(v32[skip & ~empty])).all() and (val[empty] == 0).all()
    assert (skip & ~empty).any() and empty.any() and (~skip).any()
    assert within(val[~skip], want[~skip], (bound[:, None] + 3 * U)[~skip], f"{what}: dosage values")


# ------------------------------------------------------------------- CPU ---
def pack(sizes, ch):
    """dbtk_pred_plan::dosage_items restated: whole loci packed greedily into items of at most ch k-mers, a larger locus cut into
    ch-sized parts.  -> [(k0, nkm, l0, nl)] with nl = 0 for a part, and the folded loci."""
    items, fold, cur, k = [], [], None, 0
    for t, n in enumerate(sizes):
        if n > ch:
            if cur:
                items.append(tuple(cur))
            cur = None
            items += [(k + o, min(ch, n - o), t, 0) for o in range(0, n, ch)]
            fold.append(t)
        else:
            if cur and cur[1] + n > ch:
                items.append(tuple(cur))
                cur = None
            cur = cur or [k, 0, t, 0]
            cur[1] += n
            cur[3] += 1
        k += n
    if cur:
        items.append(tuple(cur))
    return items, fold


def source_constants():
    hip = open(os.path.join(CSRC, "dbtk_pred.hip")).read()
    plan = open(os.path.join(CSRC, "dbtk_pred_plan.h")).read()
    one = lambda pat, text: int(re.search(pat, text).group(1))  # noqa: E731
    c = dict(PT_K=one(r"constexpr int PT_K = (\d+),", hip), PT_S=one(r"\bPT_S = (\d+);", hip), DS_TB=one(r"constexpr int DS_TB = (\d+);", hip),
             DS_T=one(r"constexpr int DS_T = (\d+),", plan), DS_E=one(r"\bDS_E = (\d+),", plan),
             gy_cap=one(r"gy = \(uint32_t\)std::min<uint64_t>\(\(n \+ PT_S - 1\) / PT_S, (\d+)\);", hip),
             col_cap=1 << one(r"nb = \(uint32_t\)std::min<uint64_t>\(\(p->nk \+ 255\) / 256, 1u << (\d+)\);", hip))
    assert re.search(r"DS_CH = DS_T \* DS_E;", plan) and "__launch_bounds__(256) k_pred_load_col" in hip
    assert "q = blockIdx.x * 64 + threadIdx.x" in hip and "dim3((d->nfold + 63) / 64), dim3(64)" in hip        # k_dosage_fold: 64 loci per block
    return c


def test_the_cases_are_what_they_claim():
    c = source_constants()
    assert c == dict(PT_K=64, PT_S=32, DS_TB=1024, DS_T=256, DS_E=8, gy_cap=64, col_cap=65536), c
    # (a) a block of the sample axis takes 1, 2, 2 (the second ragged) and 3 steps
    full = c["gy_cap"] * c["PT_S"]
    assert A_NS[0] == full and A_NS[1] == full + 1 and all(math.ceil(n / c["PT_S"]) > c["gy_cap"] for n in A_NS[1:])
    assert full + c["PT_S"] < A_NS[2] < 2 * full and A_NS[2] % c["PT_S"]      # two blocks take a second step, the second of them a ragged one
    assert A_NS[3] > 2 * full and A_NS[3] % c["PT_S"]
    ma = cohort_a(A_NS[0])[0]
    assert ma["nk"] == sum(A_SIZES) + A_TAIL and largest_locus(ma) == 65 and {0, 1, c["PT_K"], c["PT_K"] + 1} <= set(A_SIZES)
    e, s = skipped(ma)
    assert e.sum() == 3 and (s & ~e).sum() == 1
    # (b) the column kernel's grid is capped and strides; corrected loci at both ends and across row 2^24
    mb = cohort_b()[0]
    assert mb["nk"] == B_NK and math.ceil(B_NK / 256) > c["col_cap"] and B_NK % 256
    sp = list(spans(mb))
    assert sp[2][1] < c["col_cap"] * 256 < sp[2][2] and sp[4][2] < B_NK and sp[0][1] == 0
    assert [t for t, si, ei, isi, iei in sp if iei > isi] == [0, 2, 4]
    assert any(i >= c["col_cap"] * 256 for i in mb["iki"][sp[2][3]:sp[2][4]]) and any(i < c["col_cap"] * 256 for i in mb["iki"][sp[2][3]:sp[2][4]])
    # (c) the work list
    ch = c["DS_T"] * c["DS_E"]
    mc = cohort_c(1)[0]
    assert mc["ntr"] == len(C_SIZES) == 748 and mc["nk"] == sum(C_SIZES) + C_TAIL
    items, fold = pack(C_SIZES, ch)
    nikc = np.concatenate([[0], mc["nik_cum"].astype(np.int64)])
    assert len(items) == 144 and max(it[3] for it in items) == 668 > 2 * c["DS_T"]      # three `lg` groups, three passes of the kms loop
    assert len(fold) == 69 > 64                                                          # a second block of k_dosage_fold
    assert any(nl and not nkm for _, nkm, _, nl in items)                                # an item of empty loci only
    assert all(nkm <= ch for _, nkm, _, _ in items) and sum(it[1] for it in items) == sum(C_SIZES)
    straddled = 0
    for k0, nkm, l0, nl in items:
        for g0 in range(l0, l0 + nl, c["DS_T"]):                                         # a group of DS_T loci has turns of its own
            g1 = min(g0 + c["DS_T"], l0 + nl)
            if nikc[g1] - nikc[g0] > c["DS_TB"]:
                cut = nikc[g0] + c["DS_TB"]                                              # where the second turn of terms[] begins
                straddled += any(nikc[l] < cut < nikc[l + 1] for l in range(g0, g1))
    assert straddled >= 2                                                                # (the third group of the first item, and the locus of 2048 alone)
    first = items[0]
    assert first[3] == 668 and nikc[first[2] + 512] > nikc[first[2] + 256] >= nikc[first[2]]                # the third group's J0 is not the item's
    assert nikc[first[2] + 512] - nikc[first[2] + 256] > 0 and nikc[first[2] + 668] - nikc[first[2] + 512] > c["DS_TB"]   # ... and it takes two turns
    big = [t for t in fold if nikc[t + 1] - nikc[t] > c["DS_TB"]]
    assert big and any(nikc[t + 1] == nikc[t] for t in fold) and any(nikc[t + 1] - nikc[t] == 1 for t in fold)
    # (c) windows of one locus beside windows of hundreds
    nkc = np.concatenate([[0], mc["nk_cum"].astype(np.int64)])
    assert largest_locus(mc) == C_MAX_ROWS and nkc[641] <= C_MAX_ROWS
    # (e) the last window holds loci with k-mers and the columns of no locus
    me = cohort_e()[0]
    assert me["nk"] == int(me["nk_cum"][-1]) + E_TAIL and largest_locus(me) == 130 and sum(E_SIZES[6:]) + E_TAIL <= 130 < sum(E_SIZES[5:]) + E_TAIL


def test_dosage_work_list_under_sanitizers(tmp_path):
    """dosage_items is host code in a header without HIP: tests/dosage_plan_check.cpp runs it under AddressSanitizer and
    UndefinedBehaviorSanitizer in a stand-alone program, on the list of case (c) and on 4 000 random lists."""
    src = os.path.join(bind.ROOT, "tests", "dosage_plan_check.cpp")
    exe = str(tmp_path / "dosage_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "dosage work list ok\n", r.stdout + r.stderr


@pytest.mark.parametrize("ns", [D_NS, 2049])
def test_the_oracle_is_within_the_bound_of_the_float64_formulas(ns):
    """The reference and the bound of this file on the project's float32 oracle, which needs no device: its sums take the kernels'
    order but for the mean over the samples (numpy's pairwise sum)."""
    meta, counts, depths = cohort_a(ns)
    raw = PO.raw_matrix(counts, depths)
    cor, bias = PO.bias_correction(raw, meta)
    b64, bound = bias64(meta, raw)
    assert within(bias, b64, bound[:, None], "oracle Bias") and corrected_within(meta, raw, cor, b64, bound, "oracle corrected")
    assert (bias[skipped(meta)[1]] == 0).all() and (bound[~skipped(meta)[1]] > 0).all()


@pytest.mark.parametrize("variant", D_VARIANTS)
def test_the_ieee_cases_are_there(variant):
    meta, counts, depths = cohort_d(variant)
    raw = PO.raw_matrix(counts, depths)
    cor, bias = PO.bias_correction(raw, meta)
    b64, bound = bias64(meta, raw)
    assert within(bias, b64, bound[:, None], "oracle Bias") and corrected_within(meta, raw, cor, b64, bound, "oracle corrected")
    sp = list(spans(meta))
    if variant == "depth0":
        assert np.isposinf(raw[:, 11]).any() and np.isnan(raw[:, 11]).any() and np.isfinite(np.delete(raw, 11, axis=1)).all()
    if variant == "ikmc0":
        assert np.isnan(bias[4]).all() and np.isfinite(np.delete(bias, 4, axis=0)).all()
    if variant == "zero_locus":
        assert np.isnan(bias[1]).all() and np.isnan(cor[sp[1][1]:sp[1][2]]).all() and np.isfinite(np.delete(bias, 1, axis=0)).all()
    if variant == "zero_sample":
        col = cor[sp[2][1]:sp[2][2], 29]
        assert bias[2, 29] == 0 and np.isposinf(col).any() and np.isnan(col).any() and np.isfinite(np.delete(cor, 29, axis=1)).all()
    if variant == "all":
        assert np.isnan(bias).any() and not np.isfinite(cor).all()


# ------------------------------------------------------------------- GPU ---
@functools.lru_cache(maxsize=None)
def run_a(ns):
    """The whole-matrix handle's (raw, corrected, Bias) at n = ns in one launch, the oracle's raw matrix and the float64 Bias."""
    meta, counts, depths = cohort_a(ns)
    raw, cor, bias = whole_matrix(meta, counts, depths)
    raw_o = PO.raw_matrix(counts, depths)
    b64, bound = bias64(meta, raw_o)
    return raw, cor, bias, raw_o, b64, bound


@pytest.mark.gpu
@pytest.mark.parametrize("ns", A_NS)
def test_samples_past_one_pass_of_the_tile_grid_whole_matrix(ns):
    meta, counts, depths = cohort_a(ns)
    raw, cor, bias, raw_o, b64, bound = run_a(ns)
    assert (_bits(raw) == _bits(raw_o)).all()
    assert raw[:, ns - 1].any() and raw[:, 2048 - 1].any()
    assert within(bias, b64, bound[:, None], "Bias") and (bias[skipped(meta)[1]] == 0).all()
    assert corrected_within(meta, raw_o, cor, b64, bound, "corrected")
    d_raw, d_cor, d_bias = whole_matrix(meta, counts, depths, device=True)           # dbtk_pred_load_device(0, ns, ...)
    assert (_bits(d_raw) == _bits(raw_o)).all() and (_bits(d_cor) == _bits(cor)).all() and (_bits(d_bias) == _bits(bias)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("ns", A_NS)
def test_samples_past_one_pass_of_the_tile_grid_windowed(ns):
    meta, counts, depths = cohort_a(ns)
    raw, cor, bias, raw_o, b64, bound = run_a(ns)
    for max_rows in (largest_locus(meta), meta["nk"]):
        f_raw, f_cor, s_raw, s_cor, wbias, wins = windows(meta, counts, depths, max_rows)
        assert len(wins) == 1 if max_rows == meta["nk"] else len(wins) > 2
        assert wins[-1][2] + wins[-1][3] == meta["nk"]                              # the last window carries the columns of no locus
        assert (_bits(f_raw) == _bits(raw_o)).all(), max_rows
        assert (_bits(s_raw) == _bits(f_raw)).all() and (_bits(s_cor) == _bits(f_cor)).all(), max_rows
        assert (_bits(f_cor) == _bits(cor)).all() and (_bits(wbias) == _bits(bias)).all(), max_rows
        assert within(wbias, b64, bound[:, None], "windowed Bias") and corrected_within(meta, raw_o, f_cor, b64, bound, "windowed corrected")


@pytest.mark.gpu
@pytest.mark.parametrize("ns", A_NS)
def test_samples_past_one_pass_of_the_tile_grid_dosage(ns):
    meta, counts, depths = cohort_a(ns)
    bias, b64, bound = run_a(ns)[2], *run_a(ns)[4:]
    kms, dbias, val = dosage_tables(meta, counts, depths)
    assert (_bits(dbias) == _bits(bias)).all()
    check_dosage(meta, counts, depths, kms, dbias, val, b64, bound, "a")


@pytest.mark.gpu
def test_the_column_kernel_past_65536_blocks():
    meta, counts, depths = cohort_b()
    hip = _Hip()
    d = hip.put(counts)
    P = pred(2, meta)
    P.load_device(1, 1, d.value + B_NK * 8, depths[1:])          # k_pred_load_col: 65 536 blocks, the last 257 k-mers in a second step
    P.load_device(0, 1, d.value, depths[:1])
    raw = P.matrix()
    raw_o = PO.raw_matrix(counts, depths)
    assert (_bits(raw) == _bits(raw_o)).all()
    top = 1 << 24
    assert raw[top:].shape == (257, 2) and (raw[top:] != 0).all() and (_bits(raw[top:]) == _bits(raw_o[top:])).all()   # the second step's rows
    assert raw[B_NK - 1, 1] == np.float32(2.0 ** 64) / depths[1] and raw[top + 3, 0] == np.float32((1 << 40) + 12345) / depths[0]
    P.correct()
    cor, bias = P.matrix(), P.bias()
    P.close()
    hip.free(d)
    b64, bound = bias64(meta, raw_o)
    assert within(bias, b64, bound[:, None], "Bias") and (bias[[1, 3]] == 0).all() and np.isfinite(bias).all() and (bias[[0, 2, 4]] > 0).all()
    assert corrected_within(meta, raw_o, cor, b64, bound, "corrected")


@functools.lru_cache(maxsize=None)
def run_c(ns):
    meta, counts, depths = cohort_c(ns)
    raw, cor, bias = whole_matrix(meta, counts, depths)
    raw_o = PO.raw_matrix(counts, depths)
    b64, bound = bias64(meta, raw_o)
    return raw, cor, bias, raw_o, b64, bound


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [1, 3])
def test_dosage_work_list_past_its_thresholds(ns):
    meta, counts, depths = cohort_c(ns)
    raw, cor, bias, raw_o, b64, bound = run_c(ns)
    assert (_bits(raw) == _bits(raw_o)).all()
    assert within(bias, b64, bound[:, None], "matrix Bias") and corrected_within(meta, raw_o, cor, b64, bound, "corrected")
    kms, dbias, val = dosage_tables(meta, counts, depths)
    assert (_bits(dbias) == _bits(bias)).all()
    check_dosage(meta, counts, depths, kms, dbias, val, b64, bound, "c")
    # a column loaded twice (first another sample's counts and depth: the later load wins), the samples in reverse order
    order = [(ns // 2, (ns // 2 + 1) % ns, ns - 1)] + [(s, s, s) for s in reversed(range(ns))]
    if ns == 1:
        order[0] = (0, 0, 0)
        counts2 = np.ascontiguousarray(counts[:, ::-1])          # (one sample: its own counts in another order first)
        D = pkg.Dosage(pkg.Dbtk(), 1, meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"], nk=meta["nk"])
        D.load(0, counts2, depths * 3 + 1)
        assert (D.kms() != kms).any()
        D.load(0, counts, depths)
        k2 = D.kms()
        D.finish()
        b2, v2 = D.bias(), D.values()
        D.close()
    else:
        k2, b2, v2 = dosage_tables(meta, counts, depths, order)
    assert (k2 == kms).all() and (_bits(b2) == _bits(dbias)).all() and (_bits(v2) == _bits(val)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [1, 3])
def test_dosage_meta_through_windows_of_one_and_of_hundreds_of_loci(ns):
    meta, counts, depths = cohort_c(ns)
    raw, cor, bias, raw_o, b64, bound = run_c(ns)
    f_raw, f_cor, s_raw, s_cor, wbias, wins = windows(meta, counts, depths, C_MAX_ROWS)
    per = [end - first for first, end, _, _ in wins]
    assert 1 in per and max(per) > 600 and wins[-1][2] + wins[-1][3] == meta["nk"]
    assert (_bits(f_raw) == _bits(raw_o)).all() and (_bits(f_cor) == _bits(cor)).all() and (_bits(wbias) == _bits(bias)).all()
    assert (_bits(s_raw) == _bits(f_raw)).all() and (_bits(s_cor) == _bits(f_cor)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", D_VARIANTS)
def test_ieee_inputs_through_the_three_paths(variant):
    meta, counts, depths = cohort_d(variant)
    raw, cor, bias = whole_matrix(meta, counts, depths)
    raw_o = PO.raw_matrix(counts, depths)
    cor_o, bias_o = PO.bias_correction(raw_o, meta)
    b64, bound = bias64(meta, raw_o)
    assert (_bits(raw) == _bits(raw_o)).all()
    assert within(bias, b64, bound[:, None], "Bias") and corrected_within(meta, raw_o, cor, b64, bound, "corrected")
    assert close(bias, bias_o, RTOL) and close(cor, cor_o, RTOL)                      # the project's bound, at ns <= 300
    for max_rows in (largest_locus(meta), meta["nk"]):
        f_raw, f_cor, s_raw, s_cor, wbias, _ = windows(meta, counts, depths, max_rows)
        assert (_bits(f_raw) == _bits(raw)).all() and (_bits(f_cor) == _bits(cor)).all() and (_bits(wbias) == _bits(bias)).all()
        assert (_bits(s_raw) == _bits(raw)).all() and (_bits(s_cor) == _bits(cor)).all()
    kms, dbias, val = dosage_tables(meta, counts, depths)
    assert (_bits(dbias) == _bits(bias)).all()
    check_dosage(meta, counts, depths, kms, dbias, val, b64, bound, variant)


@pytest.mark.gpu
def test_trailing_columns_travel_with_the_last_window_uncorrected():
    meta, counts, depths = cohort_e()
    raw, cor, bias = whole_matrix(meta, counts, depths)
    raw_o = PO.raw_matrix(counts, depths)
    b64, bound = bias64(meta, raw_o)
    tail = int(meta["nk_cum"][-1])
    assert meta["nk"] - tail == E_TAIL and (_bits(raw) == _bits(raw_o)).all() and raw[tail:].all(axis=1).any()
    assert (_bits(cor[tail:]) == _bits(raw[tail:])).all() and (_bits(cor[:tail]) != _bits(raw[:tail])).any()
    assert within(bias, b64, bound[:, None], "Bias") and corrected_within(meta, raw_o, cor, b64, bound, "corrected")
    f_raw, f_cor, s_raw, s_cor, wbias, wins = windows(meta, counts, depths, largest_locus(meta))
    first, end, row0, rows = wins[-1]
    assert len(wins) > 2 and end == meta["ntr"] and row0 < tail and row0 + rows == meta["nk"] and any(E_SIZES[first:end])
    for r, c in ((f_raw, f_cor), (s_raw, s_cor)):
        assert (_bits(r) == _bits(raw)).all() and (_bits(c) == _bits(cor)).all() and (_bits(c[tail:]) == _bits(r[tail:])).all()
    assert (_bits(wbias) == _bits(bias)).all()
    kms, dbias, val = dosage_tables(meta, counts, depths)                              # (the dosage tables never read the tail)
    assert (_bits(dbias) == _bits(bias)).all()
    check_dosage(meta, counts, depths, kms, dbias, val, b64, bound, "e")


# ---- (f) the command line on (a) at ns = 2081
CLI_NS = 2081


@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("pred_edges_cli"))
    meta, counts, depths = cohort_a(CLI_NS)
    PO.write_ikmer_meta(os.path.join(d, "ikmer.meta"), meta["nk"], meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"])
    with open(os.path.join(d, "gt.meta"), "w") as f:
        for s in range(CLI_NS):
            fn = os.path.join(d, f"s{s}.trkmc.ar")
            with open(fn, "wb") as g:
                g.write(struct.pack("<Q", meta["nk"]) + counts[s].tobytes())
            f.write(f"{fn}\t{float(depths[s])!r}\n")
    return d


@pytest.mark.gpu
def test_command_line_files_do_not_notice_the_windows(cli_inputs):
    """The plain run stages 16 samples per load and never strides; the windowed runs' fused pass takes all 2081 samples at once."""
    d = cli_inputs
    meta, counts, depths = cohort_a(CLI_NS)

    def run(tag, flags):
        out = [os.path.join(d, f"{tag}.{x}") for x in ("raw.gt", "cor.gt", "bias.tsv")]
        r = subprocess.run([EXE] + flags + [os.path.join(d, "gt.meta"), os.path.join(d, "ikmer.meta")] + out, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return out
    plain = run("plain", [])
    assert open(plain[0], "rb").read() == PO.matrix_bytes(PO.raw_matrix(counts, depths))
    for i, rows in enumerate((largest_locus(meta), meta["nk"])):
        for a, b in zip(plain, run(f"w{i}", ["--window-rows", str(rows)])):
            assert filecmp.cmp(a, b, shallow=False), (rows, b)


@pytest.mark.gpu
def test_command_line_dosage_tables_do_not_notice_the_flag(cli_inputs):
    d = cli_inputs
    meta, counts, depths = cohort_a(CLI_NS)

    def run(tag, flags):
        out = [os.path.join(d, f"{tag}.{x}") for x in ("dosage.tsv", "kms", "bias.tsv")]
        r = subprocess.run([EXE] + flags + ["--dosage", out[0], "--kms", out[1], os.path.join(d, "gt.meta"), os.path.join(d, "ikmer.meta"), out[2]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return out
    plain = run("dplain", [])
    for a, b in zip(plain, run("dwin", ["--window-rows", str(largest_locus(meta))])):
        assert filecmp.cmp(a, b, shallow=False), b
    kms = segment_sums(counts, meta["nk_cum"])
    rows = open(plain[1]).read().split("\n")
    assert [int(x) for x in rows[CLI_NS - 1].split("\t")] == [int(v) for v in kms[:, CLI_NS - 1]]
