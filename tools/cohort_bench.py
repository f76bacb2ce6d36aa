#!/usr/bin/env python3
"""Cohort mode against what it replaces, at release scale: S samples of R reads over the synthetic 80 000-locus RPGG, files in /dev/shm.
  (i)  S single `danbing-tk` runs + one `danbing-tk-pred` over their count files   (binaries under --parent: the commit before cohort mode)
  (ii) one `danbing-tk --cohort MANIFEST --pred ...` run of this tree              (and once more with DBTK_COHORT_CONTEXTS=1)
Each leg runs twice and the second is reported (the first pass over freshly written tmpfs files is bound by the first touch of their
pages).  Checks that both legs wrote the same bytes (every OUT.trkmc.ar, RAW.gt), then prints one JSON line.
    python tools/cohort_bench.py [--samples 16] [--reads 8000000] [--distinct D] [--nloci 80000] [--parent DIR]
--dosage: only the two cohort legs that differ in what they keep in HBM — `--cohort --pred` of --parent (the matrix) and `--cohort
--dosage --no-trkmc` of this tree (the per-locus tables) — twice each; prints both passes of both, and whether the two bias tables
are the same bytes.
--distinct D: only D different reads files are generated, the samples cycle through them (less tmpfs, the same work per sample)."""
import argparse
import ctypes as C
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
pkg = importlib.import_module("danbing-tk_amd")
import pred_oracle as PO  # noqa: E402

FLAGS = ["-k", "21", "-kf", "4", "1", "-cth", "45", "-ka", "-qs", "pan"]


def timed(argv, cwd, env=None, limit=300):
    """One step under a time limit of its own (a step that hangs ends the tool: subprocess.TimeoutExpired kills the child)."""
    t0 = time.perf_counter()
    r = subprocess.run(argv, cwd=cwd, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=limit)
    dt = time.perf_counter() - t0
    if r.returncode:
        sys.exit(f"{' '.join(argv)}: rc {r.returncode}\n{r.stderr[-3000:]}")
    return dt, r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--reads", type=int, default=8_000_000)
    ap.add_argument("--distinct", type=int, default=0)
    ap.add_argument("--nloci", type=int, default=80000)
    ap.add_argument("--dosage", action="store_true", help="only `--cohort --pred` (of --parent) against `--cohort --dosage --no-trkmc` (of this tree)")
    ap.add_argument("--parent", default=None, help="tree holding danbing-tk_amd/bin of the commit before cohort mode [this tree]")
    a = ap.parse_args()
    S, D = a.samples, a.distinct or a.samples
    here = os.path.join(ROOT, "danbing-tk_amd", "bin")
    par = os.path.join(os.path.abspath(a.parent), "danbing-tk_amd", "bin") if a.parent else here
    d = tempfile.mkdtemp(prefix="dbtk_cohort_", dir="/dev/shm")
    try:
        t0 = time.perf_counter()
        syn = pkg.Synth(nloci=a.nloci, nthreads=16)
        syn.write_files(os.path.join(d, "pan"))
        arr = syn.arrays()
        nl = int(arr.nloci)
        tr_cnt = np.ctypeslib.as_array(arr.tr_cnt, shape=(nl,)).astype(np.uint64)
        nk_cum = np.cumsum(tr_cnt).astype(np.uint32)
        has = tr_cnt > 0
        iki = (nk_cum - tr_cnt.astype(np.uint32))[has]           # the first k-mer of every locus as its invariant k-mer
        PO.write_ikmer_meta(os.path.join(d, "ikmer.meta"), int(nk_cum[-1]), nk_cum, np.cumsum(has).astype(np.uint32), iki, np.ones(len(iki), np.uint8))
        buf = None
        for j in range(D):
            buf, _ = syn.reads(a.reads // 2, hit_frac=0.02, seed=100 + j, out=buf, nthreads=16)
            syn.write_fasta(buf, a.reads // 2, os.path.join(d, f"r{j}.fa"))
        del buf
        syn.close()
        print(f"# {S} samples x {a.reads} reads ({D} distinct files), nk {int(nk_cum[-1])}, made in {time.perf_counter() - t0:.1f} s in {d}", flush=True)
        depths = [20.0 + 0.5 * i for i in range(S)]
        with open(os.path.join(d, "m.tsv"), "w") as f, open(os.path.join(d, "gt.meta"), "w") as g:
            for i in range(S):
                f.write(f"r{i % D}.fa\tc{i}\t{depths[i]!r}\n")
                g.write(f"s{i}.trkmc.ar\t{depths[i]!r}\n")
        res = dict(samples=S, reads=a.reads, distinct=D, nk=int(nk_cum[-1]))
        if a.dosage:
            legs = dict(pred=[os.path.join(par, "danbing-tk")] + FLAGS + ["--cohort", "m.tsv", "--pred", "ikmer.meta", "coh.raw.gt", "coh.cor.gt", "coh.bias.tsv"],
                        dosage=[os.path.join(here, "danbing-tk")] + FLAGS + ["--cohort", "m.tsv", "--dosage", "ikmer.meta", "dos.tsv", "dos.bias.tsv", "--kms", "dos.kms", "--no-trkmc"])
            for name, argv in legs.items():
                for rep in range(2):
                    dt, _ = timed(argv, d)
                    res[f"{name}_pass{rep}_s"] = dt
                    print(f"# --cohort --{name} pass {rep}: {dt:.2f} s", flush=True)
            res.update(same_bias=open(os.path.join(d, "coh.bias.tsv"), "rb").read() == open(os.path.join(d, "dos.bias.tsv"), "rb").read(),
                       parent_spread_s=abs(res["pred_pass0_s"] - res["pred_pass1_s"]), dosage_minus_pred_s=res["dosage_pass1_s"] - res["pred_pass1_s"])
            print(json.dumps(res))
            if not res["same_bias"]:
                sys.exit("bias tables differ")
            return
        for rep in range(2):                                      # (i)
            t_runs = 0.0
            for i in range(S):
                dt, _ = timed([os.path.join(par, "danbing-tk")] + FLAGS + ["-fa", f"r{i % D}.fa", "-o", f"s{i}"], d)
                t_runs += dt
            t_pred, _ = timed([os.path.join(par, "danbing-tk-pred"), "gt.meta", "ikmer.meta", "two.raw.gt", "two.cor.gt", "two.bias.tsv"], d)
            res.update(separate_s=t_runs + t_pred, separate_runs_s=t_runs, separate_pred_s=t_pred)
            print(f"# (i) pass {rep}: {S} runs {t_runs:.2f} s + pred {t_pred:.2f} s", flush=True)
        coh = [os.path.join(here, "danbing-tk")] + FLAGS + ["--cohort", "m.tsv", "--pred", "ikmer.meta", "coh.raw.gt", "coh.cor.gt", "coh.bias.tsv"]
        for rep in range(2):                                      # (ii)
            dt, err = timed(coh, d, {"DBTK_VERBOSE": "1"})
            res.update(cohort_s=dt)
            print(f"# (ii) pass {rep}: {dt:.2f} s", flush=True)
        keep = [l for l in err.splitlines() if l.startswith(("cohort:", "load:", "timeline:"))]
        dt1, err1 = timed(coh, d, {"DBTK_VERBOSE": "1", "DBTK_COHORT_CONTEXTS": "1"})
        keep += ["(one context) " + l for l in err1.splitlines() if l.startswith("cohort:")]
        dtn, _ = timed(coh + ["--no-trkmc"], d)
        res.update(cohort_one_context_s=dt1, cohort_no_trkmc_s=dtn)
        for l in keep:
            print("#   " + l[:300])
        same = all(open(os.path.join(d, f"s{i}.trkmc.ar"), "rb").read() == open(os.path.join(d, f"c{i}.trkmc.ar"), "rb").read() for i in range(S))
        same_raw = open(os.path.join(d, "two.raw.gt"), "rb").read() == open(os.path.join(d, "coh.raw.gt"), "rb").read()
        res.update(same_counts=same, same_raw=same_raw, per_sample_separate_s=res["separate_s"] / S, per_sample_cohort_s=res["cohort_s"] / S,
                   ratio=res["separate_s"] / res["cohort_s"])
        print(json.dumps(res))
        if not (same and same_raw):
            sys.exit("outputs differ")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
