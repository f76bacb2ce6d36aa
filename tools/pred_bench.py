#!/usr/bin/env python3
"""Throughput of the danbing-tk-pred kernels on one MI355X (include/dbtk_pred.h): a synthetic cohort of ns samples over an
RPGG of ntr loci x kpl k-mers, a tenth of them invariant.  Prints the kernel times and their HBM rates (algorithmic bytes:
bias sums 4 B per (invariant k-mer, sample); correction 8 B per matrix entry, read + write).
    python tools/pred_bench.py [ns] [ntr] [kpl]
    python tools/pred_bench.py --dosage [nk ...]     the per-sample pass of the dosage tables (k_dosage_sample) against the matrix
                                                     path's column kernel (k_pred_load_col) on the same counts in HBM"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("danbing-tk_amd")


def main():
    ns = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    ntr = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
    kpl = int(sys.argv[3]) if len(sys.argv) > 3 else 184
    rng = np.random.default_rng(1)
    nk = ntr * kpl
    nk_cum = (np.arange(1, ntr + 1) * kpl).astype(np.uint32)
    nikl = max(1, kpl // 10)
    iki = (np.arange(ntr)[:, None] * kpl + np.sort(rng.integers(0, kpl, (ntr, nikl)), axis=1)).astype(np.uint32).ravel()
    nik_cum = (np.arange(1, ntr + 1) * nikl).astype(np.uint32)
    ikmc = rng.integers(1, 4, len(iki)).astype(np.uint8)
    depths = rng.uniform(10, 50, ns).astype(np.float32)
    lib = pkg.Dbtk()
    P = pkg.Pred(lib, ns, nk_cum, nik_cum, iki, ikmc, nk=nk)
    t0 = time.time()
    B = 16
    for s0 in range(0, ns, B):
        n = min(B, ns - s0)
        P.load(s0, rng.integers(0, 200, (n, nk), dtype=np.uint64), depths[s0:s0 + n])
    t_load = time.time() - t0
    P.correct()
    P.correct()
    ms = P.times()
    bytes_bias, bytes_cor = 4.0 * len(iki) * ns, 8.0 * nk * ns
    print(f"cohort {ns} samples x {nk} k-mers ({4 * nk * ns / 1e9:.2f} GB matrix), {ntr} loci, {len(iki)} invariant k-mers; load (host RNG + PCIe) {t_load:.1f}s")
    print(f"k_pred_bias {ms[0]:.3f} ms = {bytes_bias / ms[0] / 1e6:.0f} GB/s   k_pred_bias_norm {ms[1]:.3f} ms   "
          f"k_pred_correct {ms[2]:.3f} ms = {bytes_cor / ms[2] / 1e6:.0f} GB/s ({bytes_cor / ms[2] / 1e6 / 8000:.1%} of 8 TB/s)")
    P.close()


def dosage_leg(nks):
    """One sample's counts in HBM -> (i) its column of the matrix (dbtk_pred_load_device, n = 1), (ii) its kms and raw-bias entries
    (dbtk_dosage_load_device).  Both calls launch on the handle's stream and wait for it: the wall time of a call is launch + kernel
    + wait for both, taken as the median of 20 after 3 warm-ups; for (ii) the HIP-event time of the kernels alone is printed too.
    Bytes of (ii): 8 * nk of counts + 16 per invariant k-mer (index, expected count, the gathered count)."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    lib = pkg.Dbtk()
    rng = np.random.default_rng(2)
    for nk in nks:
        for kpl in (184, 40, 3000):                              # k-mers per locus: the release's mean, small loci, loci of two work items
            ntr = nk // kpl
            nk_cum = (np.arange(1, ntr + 1, dtype=np.uint64) * kpl).astype(np.uint32)
            nk_cum[-1] = nk
            nikl = max(1, kpl // 10)
            iki = (np.arange(ntr, dtype=np.uint64)[:, None] * kpl + np.sort(rng.integers(0, kpl, (ntr, nikl)), axis=1)).astype(np.uint32).ravel()
            nik_cum = (np.arange(1, ntr + 1, dtype=np.uint64) * nikl).astype(np.uint32)
            ikmc = rng.integers(1, 4, len(iki)).astype(np.uint8)
            counts = rng.integers(0, 200, nk, dtype=np.uint64)
            d = C.c_void_p()
            assert hip.hipMalloc(C.byref(d), counts.nbytes) == 0 and hip.hipMemcpy(d, counts.ctypes.data_as(C.c_void_p), counts.nbytes, 1) == 0
            ns = 64
            depth = np.array([30.0], np.float32)
            P = pkg.Pred(lib, ns, nk_cum, nik_cum, iki, ikmc, nk=nk)
            D = pkg.Dosage(lib, ns, nk_cum, nik_cum, iki, ikmc, nk=nk)
            wall = {}
            for name, h in (("k_pred_load_col", P), ("k_dosage_sample", D)):
                ts, ev = [], []
                for i in range(23):
                    t0 = time.perf_counter()
                    h.load_device(i % ns, 1, d.value, depth)
                    ts.append(time.perf_counter() - t0)
                    if h is D:
                        ev.append(D.times()[0])
                wall[name] = (float(np.median(ts[3:])) * 1e3, float(np.median(ev[3:])) if ev else None)
            e = C.sizeof(C.c_uint64) * nk + 16.0 * len(iki)
            w_col, w_dos, ev_dos = wall["k_pred_load_col"][0], wall["k_dosage_sample"][0], wall["k_dosage_sample"][1]
            print(f"nk {nk} ({ntr} loci x {kpl}, {len(iki)} invariant): k_pred_load_col call {w_col:.3f} ms; k_dosage_sample call {w_dos:.3f} ms, "
                  f"kernels (HIP events) {ev_dos:.3f} ms = {e / ev_dos / 1e6:.0f} GB/s ({e / ev_dos / 1e6 / 8000:.1%} of 8 TB/s); "
                  f"handle {D.nbytes() / 1e6:.1f} MB at ns {ns}", flush=True)
            P.close(); D.close()
            hip.hipFree(d)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--dosage":
        dosage_leg([int(x) for x in sys.argv[2:]] or [14_750_000, 31_200_000])
    else:
        main()
