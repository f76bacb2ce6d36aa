#!/usr/bin/env python3
"""-bu at release scale: the event log + host replay (plain `-bu`, binaries under --parent: the commit before the device table)
against `-bu --bu-table` of this tree, and the same run without -bu, through the command line on a file in /dev/shm.
The synthetic 80 000-locus RPGG and the two mixes of bench.py (all-hit; WGS-like: 2 % of the pairs from a locus), every read
with 0.3 % substitutions.  Each leg runs twice and the second pass is reported (the first pass over a freshly written tmpfs file is
bound by the first touch of its pages).  Per leg: wall time, batch-loop time (the `ingest:` line), and for the table run the
entries and events it holds at the end, the slots it grew to, the number of growths and the merge + compact + write time.
One JSON line per mix.
    python tools/bu_bench.py [--reads 10000000] [--nloci 80000] [--parent DIR] [--mix all_hit|wgs|both]"""
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

FLAGS = ["-k", "21", "-kf", "4", "1", "-cth", "45", "-ka", "-qs", "pan"]
SUB = 0.003


def timed(argv, cwd, limit=600):
    """One step under a time limit of its own (a step that hangs ends the tool: subprocess.TimeoutExpired kills the child)."""
    t0 = time.perf_counter()
    r = subprocess.run(argv, cwd=cwd, capture_output=True, text=True, env=dict(os.environ, DBTK_VERBOSE="1"), timeout=limit)
    dt = time.perf_counter() - t0
    if r.returncode:
        sys.exit(f"{' '.join(argv)}: rc {r.returncode}\n{r.stderr[-3000:]}")
    return dt, r.stderr


def substitute(buf, rate, seed):
    """rate of the bases replaced by another base, in place."""
    rng = np.random.default_rng(seed)
    n = int(len(buf) * rate)
    at = rng.integers(0, len(buf), n)
    code = np.zeros(256, np.uint8)
    for i, b in enumerate(b"ACGT"):
        code[b] = i
    buf[at] = np.frombuffer(b"ACGT", np.uint8)[(code[buf[at]] + rng.integers(1, 4, n).astype(np.uint8)) & 3]


def figures(err):
    out = {}
    m = re.search(r"ingest: ([0-9.]+) s for (\d+) reads", err)
    if m:
        out["batch_loop_s"] = float(m.group(1))
    m = re.search(r"bubbles: merged and written in ([0-9.]+) s", err)
    if m:
        out["compact_write_s"] = float(m.group(1))
    m = re.search(r"bubble table: (\d+) entries in (\d+) slots, (\d+) events", err)
    if m:
        out.update(entries=int(m.group(1)), slots=int(m.group(2)), events=int(m.group(3)))
    out["growths"] = len(re.findall(r"bubble table: grown to", err))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--nloci", type=int, default=80000)
    ap.add_argument("--mix", default="both", choices=["all_hit", "wgs", "both"])
    ap.add_argument("--parent", default=None, help="tree holding danbing-tk_amd/bin of the commit before the device table [this tree]")
    a = ap.parse_args()
    here = os.path.join(ROOT, "danbing-tk_amd", "bin", "danbing-tk")
    par = os.path.join(os.path.abspath(a.parent), "danbing-tk_amd", "bin", "danbing-tk") if a.parent else here
    d = tempfile.mkdtemp(prefix="dbtk_bu_", dir="/dev/shm")
    try:
        syn = pkg.Synth(nloci=a.nloci, nthreads=16)
        syn.write_files(os.path.join(d, "pan"))
        for mix, hit in (("all_hit", 1.0), ("wgs", 0.02)):
            if a.mix not in (mix, "both"):
                continue
            buf, _ = syn.reads(a.reads // 2, hit_frac=hit, seed=7, nthreads=16)
            substitute(buf, SUB, 8)
            syn.write_fasta(buf, a.reads // 2, os.path.join(d, "r.fa"))
            del buf
            res = dict(mix=mix, reads=a.reads, sub=SUB)
            legs = dict(no_bu=[here] + FLAGS + ["-fa", "r.fa", "-o", "n"], bu_log_parent=[par] + FLAGS + ["-bu", "-fa", "r.fa", "-o", "l"],
                        bu_table=[here] + FLAGS + ["-bu", "--bu-table", "-fa", "r.fa", "-o", "t"])
            for name, argv in legs.items():
                for rep in range(2):
                    dt, err = timed(argv, d)
                    print(f"# {mix} {name} pass {rep}: {dt:.2f} s", flush=True)
                res[name] = dict(wall_s=dt, **figures(err))
            # the same set per locus, and the same count files
            la, ta = np.fromfile(os.path.join(d, "l.bub.kmdb"), np.uint64), np.fromfile(os.path.join(d, "t.bub.kmdb"), np.uint64)
            nl = int(la[0])
            res["same_index"] = bool(len(la) == len(ta) and (la[:3 + nl] == ta[:3 + nl]).all())
            res["same_counts"] = open(os.path.join(d, "n.trkmc.ar"), "rb").read() == open(os.path.join(d, "t.trkmc.ar"), "rb").read()
            res["table_minus_no_bu_batch_loop_s"] = res["bu_table"].get("batch_loop_s", 0) - res["no_bu"].get("batch_loop_s", 0)
            print(json.dumps(res), flush=True)
        syn.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
