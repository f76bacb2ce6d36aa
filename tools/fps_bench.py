#!/usr/bin/env python3
"""--bait-fps at release scale, through the command line on files in /dev/shm, on the inputs of tools/sim_bench.py: the synthetic
80 000-locus RPGG and --genomes assemblies of at least --min-mb megabases each.  Genome 0 is sim_bench's (haplotype 0, one locus in
ten under the next locus' index: the false positives); genome g > 0 lays out haplotype g of every locus under its true labels.
  (a) the existing way: one `--sim ... --bait-profile` run per genome (the first in both classes, the others --tp-only), every
      profile written as text, then `ktools fps` over the FP profile and the TP profiles (binary under --parent: the commit before
      --bait-fps; by default this tree's, whose path there is that commit's);
  (b) one `--bait-fps OUT --genome G0 --sim ... --genome G1 --sim ...` run of this tree: no profile text at all.
Both must make the same file.  One JSON line: both wall times, per run of (a) the profile export, and of (b) the end-of-genome steps
(begin, apply, reset), the milliseconds in k_kcp_fps_apply and its look-ups per second.
    python tools/fps_bench.py [--genomes 3] [--min-mb 200] [--nloci 80000] [--parent DIR]"""
import argparse
import json
import os
import re
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sim_bench  # noqa: E402  (the assembly builder, the timed step and the figures of a run)

pkg = sim_bench.pkg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=3)
    ap.add_argument("--min-mb", type=int, default=200)
    ap.add_argument("--nloci", type=int, default=80000)
    ap.add_argument("--parent", default=None, help="tree holding danbing-tk_amd/bin of the commit before --bait-fps [this tree]")
    a = ap.parse_args()
    here = os.path.join(ROOT, "danbing-tk_amd", "bin")
    par = os.path.join(os.path.abspath(a.parent), "danbing-tk_amd", "bin") if a.parent else here
    d = tempfile.mkdtemp(prefix="dbtk_fps_", dir="/dev/shm")
    try:
        syn = pkg.Synth(nloci=a.nloci, nthreads=16)
        syn.write_files(os.path.join(d, "pan"))
        res = dict(nloci=a.nloci, genomes=a.genomes, assembly_bases=[])
        for g in range(a.genomes):
            contigs, bed = sim_bench.build_assembly(syn, a.nloci, a.min_mb * 1_000_000, seed=5 + g, hap=g, mislabel=g == 0)
            with open(os.path.join(d, f"g{g}.fa"), "wb") as f:
                for name, s in contigs:
                    f.write(b">" + name.encode() + b"\n" + s.tobytes() + b"\n")
            with open(os.path.join(d, f"g{g}.bed"), "w") as f:
                f.write("".join(f"{contigs[c][0]}\t{s}\t{e}\t{l}\n" for c, s, e, l in bed))
            res["assembly_bases"].append(int(sum(len(s) for _, s in contigs)))
            del contigs, bed
        syn.close()
        exe, ktools = os.path.join(par, "danbing-tk"), os.path.join(par, "ktools")
        # (a) per genome a run and its profile text, then ktools fps
        runs, t_a = [], 0.0
        for g in range(a.genomes):
            argv = [exe] + sim_bench.COMMON + ["--sim", f"g{g}.fa", f"g{g}.bed", "--bait-profile", f"p{g}", "-o", f"a{g}"] + (["--tp-only"] if g else [])
            dt, err, _ = sim_bench.timed(argv, d)
            print(f"# existing way, genome {g}: {dt:.2f} s", flush=True)
            t_a += dt
            runs.append(dict(wall_s=dt, **sim_bench.figures(err)))
        dt, _, _ = sim_bench.timed([ktools, "fps", str(a.nloci), "21", "ref.fps", "p0.FP_pf.txt"] + [f"p{g}.TP_pf.txt" for g in range(a.genomes)], d, limit=1500)
        print(f"# existing way, ktools fps: {dt:.2f} s", flush=True)
        names = [f"p0.FP_pf.txt"] + [f"p{g}.TP_pf.txt" for g in range(a.genomes)]
        res["existing"] = dict(wall_s=t_a + dt, runs=runs, ktools_fps_s=dt, export_s=sum(r.get("export_s", 0.0) for r in runs),
                               profile_text_bytes=sum(os.path.getsize(os.path.join(d, n)) for n in names))
        # (b) one run
        argv = [os.path.join(here, "danbing-tk")] + sim_bench.COMMON + ["--bait-fps", "one.fps", "-o", "b"]
        for g in range(a.genomes):
            argv += ["--genome", f"G{g}", "--sim", f"g{g}.fa", f"g{g}.bed"]
        dt, err, _ = sim_bench.timed(argv, d)
        print(f"# one --bait-fps --genome run: {dt:.2f} s", flush=True)
        one = dict(wall_s=dt, **sim_bench.figures(err))
        m = re.search(r"bait fps: (\d+) candidates, (\d+) alive; (\d+) look-ups in ([0-9.]+) ms of the apply kernel; begin, apply and reset ([0-9.]+) s, written in ([0-9.]+) s", err)
        if m:
            one.update(candidates=int(m.group(1)), alive=int(m.group(2)), lookups=int(m.group(3)), apply_ms=float(m.group(4)), genome_steps_s=float(m.group(5)),
                       write_s=float(m.group(6)))
            one["lookups_per_s"] = one["lookups"] / (one["apply_ms"] / 1e3) if one["apply_ms"] > 0 else 0.0
        one["genome_lines"] = re.findall(r"^# genome \d+ \S+: \d+ candidates, \d+ alive$", err, re.M)
        res["one_run"] = one
        res["same_file"] = open(os.path.join(d, "ref.fps"), "rb").read() == open(os.path.join(d, "one.fps"), "rb").read()
        res["fps_file_bytes"] = os.path.getsize(os.path.join(d, "one.fps"))
        res["one_run_minus_existing_wall_s"] = one["wall_s"] - res["existing"]["wall_s"]
        print(json.dumps(res), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    t0 = time.perf_counter()
    main()
    print(f"# fps_bench: {time.perf_counter() - t0:.1f} s in all", flush=True)
