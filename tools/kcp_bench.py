#!/usr/bin/env python3
"""--bait-profile at release scale, through the command line on a file in /dev/shm: the synthetic 80 000-locus RPGG, all-hit pairs
titled >LOCUS.PAIR for -s 1 (one title in ten names the next locus, so that false positives exist), 0.3 % substitutions.
  (i)   `-s 1` with the kam text to /dev/null — what feeds baitBuilder today (binary under --parent: the commit before this table);
  (ii)  `-s 1 -ka --bait-profile` of this tree — no kam text, the profiles counted in the table in HBM;
  (iii) inserts per second of the add kernel (HIP events, summed over the batches);
  (iv)  bytes of the table at the end, its slots and entries.
Each leg runs twice and the second pass is reported (the first pass over a freshly written tmpfs file is bound by the first touch
of its pages).  One JSON line.
    python tools/kcp_bench.py [--reads 8000000] [--nloci 80000] [--parent DIR]"""
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

FLAGS = ["-s", "1", "-k", "21", "-kf", "4", "1", "-cth", "45", "-qs", "pan", "-fa", "r.fa"]
SUB, LIE, RLEN = 0.003, 0.1, 150


def timed(argv, cwd, stdout, limit=900):
    """One step under a time limit of its own (a step that hangs ends the tool: subprocess.TimeoutExpired kills the child)."""
    t0 = time.perf_counter()
    with open(stdout, "wb") as out:
        r = subprocess.run(argv, cwd=cwd, stdout=out, stderr=subprocess.PIPE, text=False, env=dict(os.environ, DBTK_VERBOSE="1"), timeout=limit)
    dt = time.perf_counter() - t0
    err = r.stderr.decode("latin1")
    if r.returncode:
        sys.exit(f"{' '.join(argv)}: rc {r.returncode}\n{err[-3000:]}")
    return dt, err


def substitute(buf, rate, seed):
    """rate of the bases replaced by another base, in place."""
    rng = np.random.default_rng(seed)
    n = int(len(buf) * rate)
    at = rng.integers(0, len(buf), n)
    code = np.zeros(256, np.uint8)
    for i, b in enumerate(b"ACGT"):
        code[b] = i
    buf[at] = np.frombuffer(b"ACGT", np.uint8)[(code[buf[at]] + rng.integers(1, 4, n).astype(np.uint8)) & 3]


def digits(v, width):
    """v (uint64 array) as zero-padded decimal ASCII, one row each."""
    out = np.empty((len(v), width), np.uint8)
    for i in range(width - 1, -1, -1):
        out[:, i] = 48 + v % 10
        v = v // 10
    return out


def write_titled_fasta(fn, buf, loci_of_pair, first_pair):
    """>LLLLLLL.PPPPPPPPP/M then the read: the title carries the (claimed) source locus in front of the first '.'"""
    npairs = len(loci_of_pair)
    rows = np.empty((2 * npairs, 1 + 7 + 1 + 9 + 3 + RLEN + 1), np.uint8)
    rows[:, 0] = ord(">")
    rows[:, 1:8] = np.repeat(digits(loci_of_pair.astype(np.uint64), 7), 2, axis=0)
    rows[:, 8] = ord(".")
    rows[:, 9:18] = np.repeat(digits(np.arange(first_pair, first_pair + npairs, dtype=np.uint64), 9), 2, axis=0)
    rows[:, 18] = ord("/")
    rows[0::2, 19] = ord("1")
    rows[1::2, 19] = ord("2")
    rows[:, 20] = 10
    rows[:, 21:21 + RLEN] = buf.reshape(2 * npairs, RLEN)
    rows[:, -1] = 10
    with open(fn, "ab") as f:
        f.write(rows.tobytes())


def figures(err):
    out = {}
    m = re.search(r"ingest: ([0-9.]+) s for (\d+) reads", err)
    if m:
        out["batch_loop_s"] = float(m.group(1))
    m = re.search(r"bait profile: (\d+) entries in (\d+) slots, (\d+) bytes; (\d+) inserts in ([0-9.]+) ms of the add kernel; ([0-9.]+) s in dbtk_kcp_add", err)
    if m:
        out.update(entries=int(m.group(1)), slots=int(m.group(2)), table_bytes=int(m.group(3)), inserts=int(m.group(4)), add_kernel_ms=float(m.group(5)),
                   kcp_add_host_s=float(m.group(6)))
        out["inserts_per_s"] = out["inserts"] / max(out["add_kernel_ms"], 1e-9) * 1e3
    m = re.search(r"bait profile: compacted, sorted and written in ([0-9.]+) s", err)
    if m:
        out["export_s"] = float(m.group(1))
    out["growths"] = len(re.findall(r"bait profile table: grown", err))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8_000_000)
    ap.add_argument("--nloci", type=int, default=80000)
    ap.add_argument("--parent", default=None, help="tree holding danbing-tk_amd/bin of the commit before the profile table [this tree]")
    a = ap.parse_args()
    here = os.path.join(ROOT, "danbing-tk_amd", "bin", "danbing-tk")
    par = os.path.join(os.path.abspath(a.parent), "danbing-tk_amd", "bin", "danbing-tk") if a.parent else here
    d = tempfile.mkdtemp(prefix="dbtk_kcp_", dir="/dev/shm")
    try:
        syn = pkg.Synth(nloci=a.nloci, nthreads=16)
        syn.write_files(os.path.join(d, "pan"))
        rng = np.random.default_rng(11)
        order = rng.permutation(a.nloci).astype(np.uint32)
        npairs, step = a.reads // 2, 500_000
        for p0 in range(0, npairs, step):
            n = min(step, npairs - p0)
            buf, _ = syn.reads_loci(n, order, rlen=RLEN, odd_frac=0.0, seed=7, first_pair=p0, nthreads=16)
            substitute(buf, SUB, 8 + p0)
            src = order[(p0 + np.arange(n)) % a.nloci].astype(np.int64)
            lie = rng.random(n) < LIE
            src[lie] = (src[lie] + 1) % a.nloci
            write_titled_fasta(os.path.join(d, "r.fa"), buf, src, p0)
            del buf
        syn.close()
        res = dict(reads=a.reads, nloci=a.nloci, sub=SUB, mistitled=LIE)
        legs = dict(kam_text_parent=([par] + FLAGS + ["-o", "k"], "/dev/null"),
                    bait_profile_ka=([here] + FLAGS + ["-ka", "--bait-profile", "pf", "-o", "p"], os.path.join(d, "p.stdout")))
        for name, (argv, out) in legs.items():
            for rep in range(2):
                dt, err = timed(argv, d, out)
                print(f"# {name} pass {rep}: {dt:.2f} s", flush=True)
            res[name] = dict(wall_s=dt, **figures(err))
        res["same_counts"] = open(os.path.join(d, "k.trkmc.ar"), "rb").read() == open(os.path.join(d, "p.trkmc.ar"), "rb").read()
        res["profile_stdout_bytes"] = os.path.getsize(os.path.join(d, "p.stdout"))
        res["profile_file_bytes"] = [os.path.getsize(os.path.join(d, "pf." + x)) for x in ("TP_pf.txt", "FP_pf.txt")]
        res["profile_minus_kam_wall_s"] = res["bait_profile_ka"]["wall_s"] - res["kam_text_parent"]["wall_s"]
        print(json.dumps(res), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
