#!/usr/bin/env python3
"""Steady state of dbtk_align_batch_device with timers off, whole batches against slices (dbtk_hip.hip, DBTK_SLICE_PAIRS): in one
process, contexts created alternately with DBTK_SLICE_PAIRS=0 and with the default (and, on the headline mix, with 2^19, 2^20 and
2^21), DBTK_LANES=1 as in bench.py, each timed on bench.py's headline mix, its genome-like mix and its all-hit mix.  The latter two
must not be sliced: their step times with the default equal the unsliced context's, and with --launches a child process under
DBTK_TRACE_LAUNCHES=1 counts the encode kernel's launches per step of every mix (1 = whole).  Also: free HBM before a context is made
and after its warm-up (hipMemGetInfo), so what a context's scratch costs whole and sliced.  One JSON line.
    python tools/slice_bench.py [--nloci 80000] [--reads 10000000] [--steps 50] [--rounds 3] [--launches] [--lib PATH]"""
import argparse
import ctypes as C
import importlib
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch  # (before the library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("danbing-tk_amd")
abi = pkg.abi
RLEN = 150


def genome_like(seq, ah_seq, mp):
    """bench.py's genome-like mix: 15 % of the background pairs carry, in each mate, a 64-base stretch of some locus over a sampled window"""
    rng = np.random.default_rng(7)
    gseq = seq[:2 * mp * RLEN].copy()
    pick = np.nonzero(rng.random(mp) < 0.15)[0]
    src = rng.integers(0, mp, len(pick))
    cand = np.array([0, (RLEN - 21 + 1) // 3, 2 * ((RLEN - 21 + 1) // 3), RLEN - 64])
    at = np.minimum(rng.choice(cand, len(pick)), RLEN - 64)
    at2 = np.minimum(rng.choice(cand, len(pick)), RLEN - 64)
    for q in range(64):
        gseq[2 * pick * RLEN + at + q] = ah_seq[2 * src * RLEN + 40 + q]
        gseq[(2 * pick + 1) * RLEN + at2 + q] = ah_seq[(2 * src + 1) * RLEN + 40 + q]
    return gseq


def free_hbm(hip):
    f, t = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
    return f.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nloci", type=int, default=80000)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", action="store_true", help="also count the encode kernel's launches per step in a traced child process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if args.launches and not args.child:
        env = dict(os.environ, DBTK_TRACE_LAUNCHES="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--nloci", str(args.nloci), "--reads", str(args.reads), "--steps", "2", "--rounds", "1"]
                           + (["--lib", args.lib] if args.lib else []), env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        k1, cur = {}, None
        for line in r.stderr.splitlines():
            m = re.match(r"\[mark\] (\S+) (begin|end)", line)
            if m:
                cur = m.group(1) if m.group(2) == "begin" else None
                if cur:
                    k1[cur] = 0
            elif cur and re.match(r"\[launch\] \(?k_encode_subfilter\w*\)? grid", line):
                k1[cur] += 1
        assert k1 and all(v >= 2 for v in k1.values()), f"a mix without an encode launch per step in the trace: {k1}"
        launches = {n: v / 2 for n, v in k1.items()}
    else:
        launches = None
    os.environ["DBTK_LANES"] = "1"
    os.environ.pop("DBTK_SLICE_PAIRS", None)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib = pkg.Dbtk(args.lib) if args.lib else pkg.Dbtk()
    syn = pkg.Synth(nloci=args.nloci, k=21, flank=700, seed=20250808)
    arr = syn.arrays()
    h = C.c_void_p()
    lib._chk(lib.L.dbtk_rpgg_from_arrays(C.byref(arr), C.byref(h)))
    g = pkg.Rpgg(lib, h)
    p = abi.default_params(ksize=21, n_filter=4, nm_filter=1, cthreshold=45, okam=0)
    mp = args.reads // 2
    seq, off = syn.reads(mp, rlen=RLEN, hit_frac=0.02, seed=1)
    ah_seq, _ = syn.reads(mp, rlen=RLEN, hit_frac=1.0, seed=2)
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    mixes = {"headline": torch.from_numpy(seq).cuda(), "genome_like": torch.from_numpy(genome_like(seq, ah_seq, mp)).cuda(), "all_hit": torch.from_numpy(ah_seq).cuda()}
    keep = lib.context(g, p)  # (holds the shared tables while the timed contexts come and go)
    torch.cuda.synchronize()

    def timed(mix, setting, tag):
        if setting is None:
            os.environ.pop("DBTK_SLICE_PAIRS", None)
        else:
            os.environ["DBTK_SLICE_PAIRS"] = str(setting)
        m0 = free_hbm(hip)
        ctx = lib.context(g, p)
        ctx.timers_enable(False)
        d = mixes[mix]
        for _ in range(3):
            ctx.align_device(d.data_ptr(), d_off.data_ptr(), mp, RLEN)
            ctx.synchronize()  # (a caller that waits between batches: the hint words are the batch before's)
        for _ in range(3):
            ctx.align_device(d.data_ptr(), d_off.data_ptr(), mp, RLEN)
        ctx.synchronize()
        m1 = free_hbm(hip)
        ctx.reset()
        print(f"[mark] {tag} begin", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ctx.align_device(d.data_ptr(), d_off.data_ptr(), mp, RLEN)
        ctx.synchronize()
        dt = (time.perf_counter() - t0) / args.steps * 1e3
        print(f"[mark] {tag} end", file=sys.stderr, flush=True)
        ctx.close()
        return dt, (m0 - m1) / 1e9

    out = {"pairs_per_step": mp, "steps": args.steps, "ms_per_step": {}, "context_gb_after_warmup": {}}
    for mix in mixes:
        settings = [("whole", 0), ("default", None)] + ([("2^19", 1 << 19), ("2^20", 1 << 20), ("2^21", 1 << 21)] if mix == "headline" and not args.child else [])
        for rnd in range(args.rounds):
            for name, s in settings:
                dt, gb = timed(mix, s, f"{mix}:{name}")
                out["ms_per_step"].setdefault(f"{mix}:{name}", []).append(round(dt, 4))
                out["context_gb_after_warmup"][f"{mix}:{name}"] = round(gb, 3)
    if launches is not None:
        out["encode_launches_per_step"] = launches
    keep.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
