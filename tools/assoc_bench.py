#!/usr/bin/env python3
"""Throughput of the association scan on one MI355X (include/dbtk_assoc.h): a synthetic cohort of ns samples over ntr loci x kpl k-mers,
counts made on the device and loaded with dbtk_pred_load_device, the matrix corrected, then scanned with ppl phenotypes per locus.
Prints, per (ns, ppl): k_assoc_scan's HIP-event time (median of 5 after 2 warm-ups), the rate at which it reads G (4 * nk * ns bytes)
against the 8 TB/s roofline, the FP64 multiply-add rate reached ((ppl + 2) * nk * n multiply-adds, the algorithm's count), and beside
them k_pred_correct's time on the same matrix from the same run (dbtk_pred_times), the yardstick of a one-pass stream (it reads AND
writes G: 8 bytes per entry).
    python tools/assoc_bench.py [--ns 256,879] [--ppl 5,20] [--ntr 20000] [--kpl 184] [--covar 0,10,60]
--covar Q: the same scans with Q covariates regressed out on the device (include/dbtk_assoc_covar.h; 0: none); the multiply-add count
then has Q more dot products per row, (ppl + 2 + Q) * nk * n, and Q more per (row, phenotype) pair.
    python tools/assoc_bench.py --perm 1000 [--ns 256,879] [--ppl 5] [--covar 0,60] [--reps 7]
--perm B: behind each scan, the permutation pass (include/dbtk_assoc_perm.h) with B seeded permutations: k_assoc_perm's HIP-event time
(median of the runs after 2 warm-ups) and its FP64 multiply-add rate, ppl * (B + 1) * nk * n multiply-adds.
    python tools/assoc_bench.py --perm-yardstick [--yardstick-lib PATH] [--perm 100] [--ns 256,879] [--ntr 1000] [--ppl 5]
--perm-yardstick: k_assoc_perm against k_assoc_scan fed the SAME permuted vectors as explicit phenotypes through a pair list, on one
random matrix in device memory, at equal (row, column) work; PATH is the library whose scan is the yardstick (a build of the commit
before the permutation pass; default: this library's own scan).  Also k_assoc_perm with B identity permutations: the same multiply-adds
with a gather that is a plain read, which tells what the scattered gather costs.
    python tools/assoc_bench.py --workflow [--ns 256] [--ntr 2000]
--workflow: what the scan replaces.  The corrected matrix is copied to the host and written to /dev/shm in danbing-tk-pred's layout, read
back, and a 16-thread numpy loop (one locus per task, the formulas of tests/assoc_model.py without the p-values) makes the same r; beside
it the scan of the resident matrix, the host fold included."""
import argparse
import importlib
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("danbing-tk_amd")


def cohort(lib, ns, ntr, kpl, seed=1):
    import torch

    rng = np.random.default_rng(seed)
    nk = ntr * kpl
    nk_cum = (np.arange(1, ntr + 1, dtype=np.uint64) * kpl).astype(np.uint32)
    nikl = max(1, kpl // 10)
    iki = (np.arange(ntr, dtype=np.uint64)[:, None] * kpl + np.sort(rng.integers(0, kpl, (ntr, nikl)), axis=1)).astype(np.uint32).ravel()
    nik_cum = (np.arange(1, ntr + 1, dtype=np.uint64) * nikl).astype(np.uint32)
    ikmc = rng.integers(1, 4, len(iki)).astype(np.uint8)
    depths = rng.uniform(10, 50, ns).astype(np.float32)
    P = pkg.Pred(lib, ns, nk_cum, nik_cum, iki, ikmc, nk=nk)
    g = torch.Generator(device="cuda").manual_seed(seed)
    for s0 in range(0, ns, 16):
        n = min(16, ns - s0)
        c = torch.randint(1, 200, (n, nk), dtype=torch.int64, device="cuda", generator=g)
        torch.cuda.synchronize()
        P.load_device(s0, n, c, depths[s0:s0 + n])
    P.correct()
    P.correct()
    return P, nk_cum, nk


def tables(ns, ntr, ppl, seed=2):
    rng = np.random.default_rng(seed)
    npheno = max(ppl, min(ntr, 2000))
    pheno = rng.normal(0, 1, (npheno, ns))
    idx = np.concatenate([np.sort(rng.choice(npheno, ppl, replace=False)) for _ in range(ntr)]).astype(np.uint32)
    off = np.arange(ntr + 1, dtype=np.uint64) * ppl
    return pheno, off, idx


def rates(lib, nss, ppls, ntr, kpl, covars=(0,), perm=0, reps=7):
    for ns in nss:
        P, nk_cum, nk = cohort(lib, ns, ntr, kpl)
        cor_ms = P.times()[2]
        gbytes = 4.0 * nk * ns
        print(f"cohort {ns} samples x {nk} k-mers ({gbytes / 1e9:.2f} GB matrix), {ntr} loci x {kpl}; k_pred_correct {cor_ms:.3f} ms = "
              f"{2 * gbytes / cor_ms / 1e9:.2f} TB/s read + written", flush=True)
        for ppl in ppls:
            pheno, off, idx = tables(ns, ntr, ppl)
            A = pkg.Assoc(lib, ns, np.arange(ns), pheno)
            A.set_pairs(off, idx)
            for q in covars:
                A.set_covariates(np.random.default_rng(3).normal(0, 1, (q, ns)) if q else None)
                ms, fold = [], []
                for _ in range(7):
                    A.scan_pred(P, p_threshold=1e-6)
                    t = A.times()
                    ms.append(t[0]); fold.append(t[1])
                k = float(np.median(ms[2:]))
                fma = (ppl + 2.0 + q) * nk * ns + float(q) * ppl * nk
                print(f"  {ppl:3d} phenotypes per locus, {q:3d} covariates: k_assoc_scan {k:.3f} ms (min {min(ms[2:]):.3f}, max {max(ms[2:]):.3f}) = {gbytes / k / 1e9:.2f} TB/s of G "
                      f"({gbytes / k / 1e9 / 8:.1%} of 8 TB/s), {fma / k / 1e9:.2f} T FP64 multiply-adds/s; {k / cor_ms:.2f} x k_pred_correct; host fold {np.median(fold[2:]):.1f} ms; "
                      f"{len(A.hits())} hits", flush=True)
                if perm:
                    A.set_permutations(perm, seed=1)
                    pms = []
                    for _ in range(reps):
                        A.perm_scan_pred(P)
                        pms.append(A.perm_times())
                    kp = float(np.median([t[0] for t in pms[2:]]))
                    pfma = float(ppl) * (perm + 1) * nk * ns
                    print(f"      {perm} permutations: k_assoc_perm {kp:.1f} ms (min {min(t[0] for t in pms[2:]):.1f}, max {max(t[0] for t in pms[2:]):.1f}) = "
                          f"{pfma / kp / 1e9:.2f} T FP64 multiply-adds/s; host fold {np.median([t[1] for t in pms[2:]]):.1f} ms; "
                          f"{sum(r['n_ge'] == 0 for r in A.perm_results())} of {len(pheno)} phenotypes with p_perm = 1 / (B + 1)", flush=True)
                    A.set_permutations(0)
            A.close()
        P.close()


def perm_yardstick(lib, ylib, nss, ntr, kpl, ppl, B, reps=7):
    import torch

    nk = ntr * kpl
    nk_cum = (np.arange(1, ntr + 1, dtype=np.uint64) * kpl).astype(np.uint32)
    for ns in nss:
        g = torch.Generator(device="cuda").manual_seed(5)
        G = torch.rand((nk, ns), dtype=torch.float32, device="cuda", generator=g) * 3.0 + 0.5
        torch.cuda.synchronize()
        pheno, off, idx = tables(ns, ntr, ppl)
        npheno = len(pheno)
        perms = pkg.assoc_perm_generate(lib, ns, B, 1)
        # the yardstick: every (phenotype, b) an explicit phenotype, slot 0 the identity, the loci's lists widened to match
        explicit = np.empty((npheno * (B + 1), ns))
        explicit[0::B + 1] = pheno
        for b in range(B):
            explicit[b + 1::B + 1] = pheno[:, perms[b]]
        eidx = (idx.astype(np.uint64)[:, None] * (B + 1) + np.arange(B + 1, dtype=np.uint64)[None, :]).astype(np.uint32).ravel()
        eoff = off * (B + 1)
        E = pkg.Assoc(ylib, ns, np.arange(ns), explicit)
        E.set_pairs(eoff, eidx)
        A = pkg.Assoc(lib, ns, np.arange(ns), pheno)
        A.set_pairs(off, idx)

        def timed(call, read):
            ms = []
            for _ in range(reps):
                call()
                ms.append(read())
            return float(np.median(ms[2:])), min(ms[2:]), max(ms[2:])

        ys = timed(lambda: E.scan_device(G, nk, nk_cum=nk_cum), lambda: E.times()[0])
        A.set_permutations(B, perms=perms)
        ps = timed(lambda: A.perm_scan_device(G, nk, nk_cum=nk_cum), lambda: A.perm_times()[0])
        eb = np.array([b["r"] ** 2 for b in E.best()]).reshape(npheno, B + 1)
        T = np.array([A.perm_stats(p) for p in range(0, npheno, max(1, npheno // 50))])
        worst = float(np.abs(T - eb[::max(1, npheno // 50)]).max())
        A.set_permutations(B, perms=np.tile(np.arange(ns, dtype=np.uint32), (B, 1)))
        ident = timed(lambda: A.perm_scan_device(G, nk, nk_cum=nk_cum), lambda: A.perm_times()[0])
        fma = float(ppl) * (B + 1) * nk * ns
        print(f"{ns} samples x {nk} rows ({ntr} loci x {kpl}), {ppl} phenotypes per locus, B = {B}: {ppl * (B + 1)} columns per row\n"
              f"  k_assoc_scan fed the permuted vectors ({'the yardstick library' if ylib is not lib else 'this library'}): {ys[0]:.2f} ms (min {ys[1]:.2f}, max {ys[2]:.2f}) = {fma / ys[0] / 1e9:.2f} T multiply-adds/s\n"
              f"  k_assoc_perm: {ps[0]:.2f} ms (min {ps[1]:.2f}, max {ps[2]:.2f}) = {fma / ps[0] / 1e9:.2f} T multiply-adds/s; {ys[0] / ps[0]:.2f} x the yardstick's speed; largest |T - r^2 of the scan| {worst:.2e}\n"
              f"  k_assoc_perm with identity permutations (the gather a plain read): {ident[0]:.2f} ms: the scattered gather costs {(ps[0] - ident[0]) / ps[0]:.1%} of the kernel's time", flush=True)
        A.close()
        E.close()
        del G


def workflow(lib, ns, ntr, kpl, ppl=5):
    P, nk_cum, nk = cohort(lib, ns, ntr, kpl)
    pheno, off, idx = tables(ns, ntr, ppl)
    A = pkg.Assoc(lib, ns, np.arange(ns), pheno)
    A.set_pairs(off, idx)
    A.scan_pred(P)
    t0 = time.perf_counter()
    A.scan_pred(P)
    best = A.best()
    t_scan = time.perf_counter() - t0
    fn = "/dev/shm/dbtk_assoc_bench.gt"
    t0 = time.perf_counter()
    M = P.matrix()
    with open(fn, "wb") as f:
        f.write(np.array([ns, nk], np.uint32).tobytes())
        M.tofile(f)
    t_write = time.perf_counter() - t0
    del M
    t0 = time.perf_counter()
    M = np.fromfile(fn, np.float32, offset=8).reshape(nk, ns)
    dy = pheno - pheno.mean(axis=1, keepdims=True)
    syy = (dy * dy).sum(axis=1)

    def locus(l):
        x = M[l * kpl:(l + 1) * kpl].astype(np.float64)
        d = x - x.mean(axis=1, keepdims=True)
        sxx = (d * d).sum(axis=1)
        ph = idx[int(off[l]):int(off[l + 1])]
        with np.errstate(invalid="ignore", divide="ignore"):
            r = (d @ dy[ph].T) / np.sqrt(sxx[:, None] * syy[None, ph])
        return ph, np.nanmax(r * r, axis=0)

    top = np.zeros(len(pheno))
    with ThreadPoolExecutor(16) as ex:
        for ph, r2 in ex.map(locus, range(ntr)):
            top[ph] = np.maximum(top[ph], r2)
    t_loop = time.perf_counter() - t0
    os.unlink(fn)
    got = np.array([b["r"] ** 2 for b in best])
    assert np.allclose(got[top > 0], top[top > 0], rtol=1e-9), "the two ways disagree"
    print(f"workflow, {ns} samples x {nk} k-mers ({4.0 * nk * ns / 1e9:.2f} GB), {ntr} loci, {ppl} phenotypes per locus: matrix to /dev/shm {t_write:.2f} s + "
          f"16-thread numpy loop (read included) {t_loop:.2f} s = {t_write + t_loop:.2f} s; scan of the resident matrix, fold and p-values included, {t_scan * 1e3:.1f} ms "
          f"({(t_write + t_loop) / t_scan:.0f} x)")
    A.close()
    P.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default=None)
    ap.add_argument("--ppl", default="5,20")
    ap.add_argument("--ntr", type=int, default=None)
    ap.add_argument("--kpl", type=int, default=184)
    ap.add_argument("--covar", default="0")
    ap.add_argument("--workflow", action="store_true")
    ap.add_argument("--perm", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--perm-yardstick", action="store_true")
    ap.add_argument("--yardstick-lib", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (before libdbtk_hip.so is loaded, so that both bind to the one HIP runtime: INTEGRATION.md 5)
    lib = pkg.Dbtk()
    if a.perm_yardstick:
        ylib = pkg.Dbtk(a.yardstick_lib) if a.yardstick_lib else lib
        perm_yardstick(lib, ylib, [int(v) for v in (a.ns or "256,879").split(",")], a.ntr or 1000, a.kpl, int(a.ppl.split(",")[0]), a.perm or 100, a.reps)
    elif a.workflow:
        workflow(lib, int((a.ns or "256").split(",")[0]), a.ntr or 2000, a.kpl)
    else:
        rates(lib, [int(v) for v in (a.ns or "256,879").split(",")], [int(v) for v in a.ppl.split(",")], a.ntr or 20000, a.kpl, [int(v) for v in a.covar.split(",")], a.perm, a.reps)


if __name__ == "__main__":
    main()
