#!/usr/bin/env python3
"""--eval at release scale, through the command line on files in /dev/shm: the workload of tools/sim_bench.py (the synthetic
80 000-locus RPGG and an assembly of at least --min-mb megabases on 24 contigs), every TR span under its own locus.
  (a) `--sim ASSEMBLY BED -ka` by the binary under --parent (the commit before --eval; by default this tree's, without the flag);
  (b) the same run of this tree with `--eval`: its wall time against (a), the time of k_eval_truth with its look-ups per second, and
      the time of k_eval_sums with the bytes it reads per second (16 per TR k-mer) against the 8 TB/s of the HBM;
  (c) the truth by files, for comparison (--files; needs no GPU): the per-locus FASTA ctg[START - k, END + k) cut with numpy, and the
      compiled reference's `fa2kmers -tr` over it (oracle/_ref/fa2kmers, one thread over hash maps).  The regression script itself
      (kmers.linreg.py) needs statsmodels and is not timed.
Each GPU leg runs three times; the faster of the last two passes is reported (all three are listed).  One JSON line.
    python tools/eval_bench.py [--min-mb 200] [--nloci 80000] [--parent DIR] [--files | --no-gpu]"""
import argparse
import importlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
pkg = importlib.import_module("danbing-tk_amd")
import sim_bench  # noqa: E402

K = 21
HBM_GBPS = 8000.0


def eval_figures(err):
    m = re.search(r"--eval: (\d+) loci scored, (\d+) windows, (\d+) look-ups in ([0-9.]+) ms of k_eval_truth \(([0-9.]+) M/s\), k_eval_sums ([0-9.]+) ms \(([0-9.]+) GB/s\); "
                  r"handle made in ([0-9.]+) s, truth passes ([0-9.]+) s, scored and written in ([0-9.]+) s", err)
    if not m:
        sys.exit("no --eval line on stderr:\n" + err[-2000:])
    out = dict(loci=int(m.group(1)), windows=int(m.group(2)), lookups=int(m.group(3)), truth_ms=float(m.group(4)), lookups_per_s=float(m.group(5)) * 1e6,
               sums_ms=float(m.group(6)), sums_GBps=float(m.group(7)), handle_s=float(m.group(8)), truth_pass_s=float(m.group(9)), score_write_s=float(m.group(10)))
    out["sums_fraction_of_hbm"] = out["sums_GBps"] / HBM_GBPS
    return out


def truth_by_files(d, contigs, bed, res):
    """the per-locus FASTA of the reference's pipelines, then fa2kmers -tr over it"""
    exe = os.path.join(ROOT, "oracle", "_ref", "fa2kmers")
    t0 = time.perf_counter()
    with open(os.path.join(d, "loci.fa"), "wb") as f:
        for n, (c, st, en, _) in enumerate(bed):
            f.write(b">%d\n" % n + contigs[c][1][st - K:en + K].tobytes() + b"\n")
    res["files_cut_fasta_s"] = time.perf_counter() - t0
    res["files_fasta_bytes"] = os.path.getsize(os.path.join(d, "loci.fa"))
    if not os.path.exists(exe):
        res["files_fa2kmers_s"] = None
        return
    t0 = time.perf_counter()
    subprocess.run([exe, "-tr", "-k", str(K), "-fsi", str(K), "-fso", "0", "-on", "T", "-fa", "1", "loci.fa"], cwd=d, check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=3000)
    res["files_fa2kmers_s"] = time.perf_counter() - t0
    res["files_tr_kmers_bytes"] = os.path.getsize(os.path.join(d, "T.tr.kmers"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-mb", type=int, default=200)
    ap.add_argument("--nloci", type=int, default=80000)
    ap.add_argument("--parent", default=None, help="tree holding danbing-tk_amd/bin of the commit before --eval [this tree, without the flag]")
    ap.add_argument("--files", action="store_true", help="also the truth by files (fa2kmers)")
    ap.add_argument("--no-gpu", action="store_true", help="the truth by files alone")
    a = ap.parse_args()
    here = os.path.join(ROOT, "danbing-tk_amd", "bin", "danbing-tk")
    par = os.path.join(os.path.abspath(a.parent), "danbing-tk_amd", "bin", "danbing-tk") if a.parent else here
    d = tempfile.mkdtemp(prefix="dbtk_eval_", dir="/dev/shm")
    try:
        syn = pkg.Synth(nloci=a.nloci, nthreads=16)
        syn.write_files(os.path.join(d, "pan"))
        contigs, bed = sim_bench.build_assembly(syn, a.nloci, a.min_mb * 1_000_000, mislabel=False)
        contigs = [(n, s.copy()) for n, s in contigs]
        syn.close()
        with open(os.path.join(d, "asm.fa"), "wb") as f:
            for name, s in contigs:
                f.write(b">" + name.encode() + b"\n" + s.tobytes() + b"\n")
        with open(os.path.join(d, "asm.bed"), "w") as f:
            f.write("".join(f"{contigs[c][0]}\t{s}\t{e}\t{l}\n" for c, s, e, l in bed))
        res = dict(nloci=a.nloci, assembly_bases=int(sum(len(s) for _, s in contigs)), contigs=len(contigs), tr_bases=int(sum(e - s for _, s, e, _ in bed)))
        if a.files or a.no_gpu:
            truth_by_files(d, contigs, bed, res)
        del contigs
        if not a.no_gpu:
            sim = ["--sim", "asm.fa", "asm.bed"]
            legs = dict(sim_parent=[par] + sim_bench.COMMON + sim + ["-o", "p"],
                        sim_eval=[here] + sim_bench.COMMON + sim + ["-o", "e", "--eval", "ev"])
            for name, argv in legs.items():
                walls = []
                for rep in range(3):
                    dt, err, nout = sim_bench.timed(argv, d)
                    walls.append(dt)
                    print(f"# {name} pass {rep}: {dt:.2f} s", flush=True)
                res[name] = dict(wall_s=min(walls[1:]), walls_s=walls, **sim_bench.figures(err))
                if name == "sim_eval":
                    res[name].update(eval_figures(err))
            res["same_counts"] = open(os.path.join(d, "p.trkmc.ar"), "rb").read() == open(os.path.join(d, "e.trkmc.ar"), "rb").read()
            res["eval_minus_parent_wall_s"] = res["sim_eval"]["wall_s"] - res["sim_parent"]["wall_s"]
            res["tr_kmers"] = (os.path.getsize(os.path.join(d, "e.trkmc.ar")) - 8) // 8
            rows = [l.split("\t") for l in open(os.path.join(d, "ev.eval.tsv")).read().split("\n")[1:] if l]
            r2 = np.array([float(r[15]) for r in rows])
            res["loci_with_slope"] = int(sum(float(r[11]) > 0 for r in rows))
            res["median_r2_present"] = float(np.median(r2))
        print(json.dumps(res), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
