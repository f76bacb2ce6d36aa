"""`--assoc-perm B --assoc-seed S` on the two command lines: `danbing-tk --cohort --pred --assoc ... --assoc-perm 9 --assoc-seed 5` and
`danbing-tk-pred --assoc ... --assoc-perm 9 --assoc-seed 5` over the cohort's count files write the same OUTPREF.assoc.perm.tsv bytes,
which are those of dbtk_assoc_perm_write through the library on the matrix the run wrote; best.tsv, hits.tsv and every other output are
byte for byte what they are without the flag (the numbers themselves are held by tests/test_assoc_perm_gpu.py)."""
import os
import subprocess

import numpy as np
import pytest

import bind
import cases
from test_assoc_cli import PRED, read_bytes, write_pairs, write_table
from test_cohort import SETS, golden_ikmer_meta, make_samples, manifest, run
from test_pred_device import _Hip

pkg = bind.pkg
pytestmark = pytest.mark.gpu
PERM = ".assoc.perm.tsv"


def test_cohort_and_pred_tool_write_the_librarys_permutation_table(tmp_path):
    spec = SETS["g1"]
    gdir = os.path.join(cases.GOLDEN, spec["dir"])
    tmp = str(tmp_path)
    files = make_samples(gdir, tmp)
    ns = len(files)
    depths = [30.5, 0.75, 41.0, 17.25, 3.0, 55.125][:ns]
    ik = os.path.join(tmp, "ikmer.meta")
    meta = golden_ikmer_meta(gdir, ik)
    with open(os.path.join(tmp, "gt.meta.txt"), "w") as f:
        for i, d in enumerate(depths):
            f.write("%s.trkmc.ar\t%r\n" % (os.path.join(tmp, "coh", "c%d" % i), d))
    rng = np.random.default_rng(6)
    sample_of = [5, 0, 2, 3, 1]
    names = ["a", "b", "c"]
    pheno = rng.normal(0, 1, (3, len(sample_of)))
    table, pairs = os.path.join(tmp, "pheno.tsv"), os.path.join(tmp, "pairs.tsv")
    write_table(table, sample_of, pheno, names)
    off = list(range(meta["ntr"] + 1))
    idx = [l % 3 for l in range(meta["ntr"])]
    write_pairs(pairs, off, idx, names)

    def groups(tag, pv):
        g0 = ["--assoc", table, os.path.join(tmp, tag + "0"), "--assoc-p", "0.5"] + pv
        return g0 + ["--assoc", table, os.path.join(tmp, tag + "1"), "--assoc-pairs", pairs] + pv[:2]

    os.makedirs(os.path.join(tmp, "coh"))
    rows = [(f, os.path.join(tmp, "coh", "c%d" % i), repr(dp)) for i, (f, dp) in enumerate(zip(files, depths))]
    coh = [os.path.join(tmp, "coh." + x) for x in ("raw.gt", "cor.gt", "bias.tsv")]
    two = [os.path.join(tmp, "two." + x) for x in ("raw.gt", "cor.gt", "bias.tsv")]
    pv = ["--assoc-perm", "9", "--assoc-seed", "5"]
    r = run(spec["flags"] + ["--cohort", manifest(tmp_path / "m.tsv", rows), "--pred", ik] + coh + groups("c", pv), cwd=gdir)
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-3000:]
    assert b"# assoc " + os.path.join(tmp, "c0").encode() + b": 9 permutations, seed 5, " in r.stderr
    assert b"# assoc " + os.path.join(tmp, "c1").encode() + b": 9 permutations, seed 1, " in r.stderr      # the second group has no --assoc-seed
    outputs = [open(f, "rb").read() for f in coh]
    r = subprocess.run([PRED] + groups("p", pv) + [os.path.join(tmp, "gt.meta.txt"), ik] + two, capture_output=True)
    assert r.returncode == 0, r.stderr
    with_flag = [open(f, "rb").read() for f in two]
    r = subprocess.run([PRED] + groups("n", []) + [os.path.join(tmp, "gt.meta.txt"), ik] + two, capture_output=True)
    assert r.returncode == 0 and b"permutations" not in r.stderr, r.stderr
    assert [open(f, "rb").read() for f in two] == with_flag == outputs        # the other outputs do not change
    # the library on the matrix the run wrote
    cor = np.fromfile(coh[1], np.float32, offset=8).reshape(meta["nk"], ns)
    lib, hip = pkg.Dbtk(), _Hip()
    d = hip.put(np.ascontiguousarray(cor))
    try:
        for i, (seed, pr) in enumerate(((5, None), (1, (off, idx)))):
            c, p, n = (os.path.join(tmp, t + str(i)) for t in "cpn")
            assert read_bytes(c) == read_bytes(p) == read_bytes(n) and read_bytes(c)[0] is not None      # best.tsv and hits.tsv as without the flag
            assert not os.path.exists(n + PERM)
            text = open(c + PERM, "rb").read()
            assert text == open(p + PERM, "rb").read() and text.count(b"\n") == 4 and text.startswith(b"pheno\tn_tests\trow\tr2\tn_perm\tn_ge\tp_perm\tq_perm\na\t")
            A = pkg.Assoc(lib, ns, sample_of, pheno, names=names)
            if pr:
                A.set_pairs(*pr)
            A.set_permutations(9, seed=seed)
            A.perm_scan_device(d, meta["nk"], nk_cum=meta["nk_cum"], p_threshold=0.5 if i == 0 else -1.0)
            A.perm_write(c + "lib")
            A.close()
            assert open(c + "lib" + PERM, "rb").read() == text
    finally:
        hip.free(d)
