#!/usr/bin/env python3
"""--sim at release scale, through the command line on files in /dev/shm: the synthetic 80 000-locus RPGG and an assembly of at
least --min-mb megabases that holds haplotype 0 of every locus between random spacers, on 24 contigs; the BED names every TR span,
one locus in ten under the next locus' index (so that false positives exist).
  (a) the head of the reference's workflow as a file: the annotated FASTA (what sim_reads | bedtools map | awk leave) written here
      with numpy (its time is reported apart), then `-s 2 -ka --bait-profile -fa` on it, page cache warm (binary under --parent:
      the commit before --sim; by default this tree's, whose -fa path that commit's is);
  (b) `--sim ASSEMBLY BED -ka --bait-profile` of this tree: no file of reads at all;
  (c) bytes per second k_sim_tile wrote (HIP events, summed over the batches).
Each leg runs twice and the second pass is reported.  One JSON line.
    python tools/sim_bench.py [--min-mb 200] [--nloci 80000] [--parent DIR]"""
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
pkg = importlib.import_module("danbing-tk_amd")

FLEN, RLEN, CV, NCTG, FLANK = 500, 150, 15, 24, 700
SHFT, NBEG = 2 * RLEN // CV, FLEN - RLEN
COMMON = ["-k", "21", "-kf", "4", "1", "-cth", "45", "-qs", "pan", "-ka", "-p", "1"]


def timed(argv, cwd, limit=900):
    """One step under a time limit of its own (a step that hangs ends the tool: subprocess.TimeoutExpired kills the child)."""
    t0 = time.perf_counter()
    r = subprocess.run(argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, DBTK_VERBOSE="1"), timeout=limit)
    dt = time.perf_counter() - t0
    err = r.stderr.decode("latin1")
    if r.returncode:
        sys.exit(f"{' '.join(argv)}: rc {r.returncode}\n{err[-3000:]}")
    return dt, err, len(r.stdout)


def digits(v, width):
    out = np.empty((len(v), width), np.uint8)
    v = v.astype(np.uint64)
    for i in range(width - 1, -1, -1):
        out[:, i] = 48 + v % 10
        v = v // 10
    return out


def build_assembly(syn, nloci, min_bases, seed=5, hap=0, mislabel=True):
    """[(name, uint8 array)] and the BED rows (contig index, start, end, label) — loci in order, NCTG contigs of equal locus count.
    hap: the haplotype of every locus that is laid out (its last where it has fewer); mislabel: one locus in ten under the next
    locus' index (tools/fps_bench.py lays out further genomes with true labels)."""
    seq, hap_beg, lh0 = syn.sequences()
    lh0 = np.array([min(int(lh0[l]) + hap, int(lh0[l + 1]) - 1) for l in range(nloci)] + [0])
    rng = np.random.default_rng(seed)
    size0 = int(sum(int(hap_beg[lh0[l] + 1] - hap_beg[lh0[l]]) for l in range(nloci)))
    gap = max(100, -(-(min_bases - size0) // nloci))
    bases = np.frombuffer(b"ACGT", np.uint8)
    contigs, bed = [], []
    per = -(-nloci // NCTG)
    for c in range(NCTG):
        parts, pos = [], 0
        for l in range(c * per, min(nloci, (c + 1) * per)):
            g = bases[rng.integers(0, 4, int(rng.integers(gap // 2, gap + gap // 2 + 1)))]
            h = seq[int(hap_beg[lh0[l]]):int(hap_beg[lh0[l] + 1])]
            pos += len(g)
            bed.append((c, pos + FLANK, pos + len(h) - FLANK, (l + 1) % nloci if mislabel and l % 10 == 0 else l))
            pos += len(h)
            parts += [g, h]
        if parts:
            contigs.append((f"ctg{c:02d}", np.concatenate(parts)))
    return contigs, bed


def write_annotated(fn, contigs, bed, nloci):
    """>ctgNN:BBBBBBBBB-EEEEEEEEE:LLLLLLLL/1, read, .../2, read — numbers zero-padded (the aligner's stoull reads them the same);
    a fragment without a locus gets '.' in front of the field.  Returns the pairs written."""
    comp = np.zeros(256, np.uint8)
    for a, b in zip(b"ACGTN", b"TGCAN"):
        comp[a] = b
    total = 0
    with open(fn, "wb") as f:
        for c, (name, s) in enumerate(contigs):
            rows = [(st, en, lab) for cc, st, en, lab in bed if cc == c]
            S, E, L = (np.array(x, np.int64) for x in zip(*rows))
            rc = comp[s[::-1]]
            begs = np.arange(0, len(s) - FLEN + 1, SHFT, dtype=np.int64)
            fw = np.lib.stride_tricks.sliding_window_view(s, RLEN)
            rv = np.lib.stride_tricks.sliding_window_view(rc, RLEN)
            for b0 in range(0, len(begs), 1 << 19):
                bg = begs[b0:b0 + (1 << 19)]
                n = len(bg)
                i = np.minimum(np.searchsorted(E, bg, side="right"), len(E) - 1)  # the first interval that ends behind beg
                hit = (S[i] < bg + FLEN) & (bg < E[i])
                title = np.empty((n, 1 + 5 + 1 + 9 + 1 + 9 + 1 + 8), np.uint8)
                title[:, 0] = ord(">")
                title[:, 1:6] = np.frombuffer(name.encode(), np.uint8)
                title[:, 6] = ord(":")
                title[:, 7:16] = digits(bg, 9)
                title[:, 16] = ord("-")
                title[:, 17:26] = digits(bg + FLEN, 9)
                title[:, 26] = ord(":")
                title[:, 27:35] = digits(np.where(hit, L[i], 0), 8)
                title[~hit, 27] = ord(".")
                w = title.shape[1]
                out = np.empty((n, 2 * (w + 3 + RLEN + 1)), np.uint8)
                half = w + 3 + RLEN + 1
                for m, reads in ((0, fw[bg]), (1, rv[len(s) - FLEN - bg])):
                    o = m * half
                    out[:, o:o + w] = title
                    out[:, o + w] = ord("/")
                    out[:, o + w + 1] = ord("1") + m
                    out[:, o + w + 2] = 10
                    out[:, o + w + 3:o + w + 3 + RLEN] = reads
                    out[:, o + half - 1] = 10
                f.write(out.tobytes())
                total += n
    return total


def figures(err):
    out = {}
    m = re.search(r"ingest: ([0-9.]+) s for (\d+) reads", err)
    if m:
        out["batch_loop_s"], out["reads"] = float(m.group(1)), int(m.group(2))
    m = re.search(r"k_sim_tile wrote (\d+) bytes of reads in ([0-9.]+) ms \(([0-9.]+) GB/s\); (\d+) bytes of assembly uploaded; profile feed ([0-9.]+) s", err)
    if m:
        out.update(tile_bytes=int(m.group(1)), tile_ms=float(m.group(2)), tile_GBps=float(m.group(3)), uploaded_bytes=int(m.group(4)), profile_feed_s=float(m.group(5)))
    m = re.search(r"--sim: assemblies and BED files read in ([0-9.]+) s", err)
    if m:
        out["host_pass_s"] = float(m.group(1))
    m = re.search(r"bait profile: compacted, sorted and written in ([0-9.]+) s", err)
    if m:
        out["export_s"] = float(m.group(1))
    m = re.search(r"(\d+) reads assigned to TR region", err)
    if m:
        out["assigned"] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-mb", type=int, default=200)
    ap.add_argument("--nloci", type=int, default=80000)
    ap.add_argument("--parent", default=None, help="tree holding danbing-tk_amd/bin of the commit before --sim [this tree]")
    a = ap.parse_args()
    here = os.path.join(ROOT, "danbing-tk_amd", "bin", "danbing-tk")
    par = os.path.join(os.path.abspath(a.parent), "danbing-tk_amd", "bin", "danbing-tk") if a.parent else here
    d = tempfile.mkdtemp(prefix="dbtk_sim_", dir="/dev/shm")
    try:
        syn = pkg.Synth(nloci=a.nloci, nthreads=16)
        syn.write_files(os.path.join(d, "pan"))
        contigs, bed = build_assembly(syn, a.nloci, a.min_mb * 1_000_000)
        contigs = [(n, s.copy()) for n, s in contigs]
        syn.close()
        with open(os.path.join(d, "asm.fa"), "wb") as f:
            for name, s in contigs:
                f.write(b">" + name.encode() + b"\n" + s.tobytes() + b"\n")
        with open(os.path.join(d, "asm.bed"), "w") as f:
            f.write("".join(f"{contigs[c][0]}\t{s}\t{e}\t{l}\n" for c, s, e, l in bed))
        res = dict(nloci=a.nloci, assembly_bases=int(sum(len(s) for _, s in contigs)), contigs=len(contigs))
        t0 = time.perf_counter()
        res["pairs"] = write_annotated(os.path.join(d, "annot.fa"), contigs, bed, a.nloci)
        res["annotated_fasta_write_s"] = time.perf_counter() - t0
        res["annotated_fasta_bytes"] = os.path.getsize(os.path.join(d, "annot.fa"))
        del contigs
        legs = dict(fa_parent=[par] + COMMON + ["-s", "2", "-fa", "annot.fa", "--bait-profile", "pfa", "-o", "a"],
                    sim=[here] + COMMON + ["--sim", "asm.fa", "asm.bed", "--bait-profile", "pfs", "-o", "s"])
        for name, argv in legs.items():
            for rep in range(2):
                dt, err, nout = timed(argv, d)
                print(f"# {name} pass {rep}: {dt:.2f} s", flush=True)
            res[name] = dict(wall_s=dt, stdout_bytes=nout, **figures(err))
        same = lambda x, y: open(os.path.join(d, x), "rb").read() == open(os.path.join(d, y), "rb").read()
        res["same_counts"] = same("a.trkmc.ar", "s.trkmc.ar")
        res["same_profiles"] = same("pfa.TP_pf.txt", "pfs.TP_pf.txt") and same("pfa.FP_pf.txt", "pfs.FP_pf.txt")
        res["profile_file_bytes"] = [os.path.getsize(os.path.join(d, "pfs." + x)) for x in ("TP_pf.txt", "FP_pf.txt")]
        res["sim_minus_fa_wall_s"] = res["sim"]["wall_s"] - res["fa_parent"]["wall_s"]
        print(json.dumps(res), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
