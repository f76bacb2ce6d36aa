"""danbing-tk-pred --window-rows: the three output files of the windowed run are the unwindowed run's, byte for byte; the dosage
tables do not notice the flag; a count file of another RPGG build ends both paths with the reference's assertion (status 134)."""
import filecmp
import os
import struct
import subprocess

import numpy as np
import pytest

import bind
from test_pred_window import LARGEST, PO, cohort

EXE = os.path.join(bind.ROOT, "danbing-tk_amd", "bin", "danbing-tk-pred")
NS = 5


def write_inputs(d):
    meta, counts, depths = cohort(NS)
    PO.write_ikmer_meta(os.path.join(d, "ikmer.meta"), meta["nk"], meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"])
    with open(os.path.join(d, "gt.meta"), "w") as f:
        for s in range(NS):
            fn = os.path.join(d, f"s{s}.trkmc.ar")
            with open(fn, "wb") as g:
                g.write(struct.pack("<Q", meta["nk"]) + counts[s].tobytes())
            f.write(f"{fn}\t{float(depths[s])!r}\n")
    return meta


def run(d, tag, flags):
    out = [os.path.join(d, f"{tag}.{x}") for x in ("raw.gt", "cor.gt", "bias.tsv")]
    r = subprocess.run([EXE] + flags + [os.path.join(d, "gt.meta"), os.path.join(d, "ikmer.meta")] + out, capture_output=True, text=True)
    return r, out


@pytest.mark.gpu
def test_windowed_files_are_the_unwindowed_files(tmp_path):
    d = str(tmp_path)
    meta = write_inputs(d)
    nk = meta["nk"]
    r, plain = run(d, "plain", [])
    assert r.returncode == 0, r.stderr
    assert os.path.getsize(plain[0]) == 8 + 4 * NS * nk
    for i, (flag, v) in enumerate([("--window-rows", LARGEST), ("--window-rows", max(nk // 3, LARGEST)), ("--window-rows", nk), ("--window-bytes", 4 * NS * LARGEST + 3)]):
        r, out = run(d, f"w{i}", [flag, str(v)])
        assert r.returncode == 0, r.stderr
        for a, b in zip(plain, out):
            assert filecmp.cmp(a, b, shallow=False), (flag, v, b)
    r, _ = run(d, "small", ["--window-rows", str(LARGEST - 1)])         # a locus that no window holds
    assert r.returncode == 1 and "locus 7 " in r.stderr

    def dosage(tag, flags):
        out = [os.path.join(d, f"{tag}.{x}") for x in ("dosage.tsv", "kms", "bias.tsv")]
        r = subprocess.run([EXE] + flags + ["--dosage", out[0], "--kms", out[1], os.path.join(d, "gt.meta"), os.path.join(d, "ikmer.meta"), out[2]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return out
    for a, b in zip(dosage("dplain", []), dosage("dwin", ["--window-rows", str(LARGEST)])):
        assert filecmp.cmp(a, b, shallow=False), b
    assert filecmp.cmp(os.path.join(d, "dplain.bias.tsv"), plain[2], shallow=False)    # (the dosage tables' Bias is the matrix path's)


@pytest.mark.gpu
def test_wrong_nk_header_ends_both_paths_with_134(tmp_path):
    d = str(tmp_path)
    meta = write_inputs(d)
    _, counts, _ = cohort(NS)
    with open(os.path.join(d, "s2.trkmc.ar"), "wb") as g:
        g.write(struct.pack("<Q", meta["nk"] + 1) + counts[2].tobytes() + b"\0" * 8)
    msg = f"nk {meta['nk'] + 1} != nk_ {meta['nk']}\n"
    for tag, flags in (("plain", []), ("win", ["--window-rows", str(LARGEST)])):
        r, _ = run(d, tag, flags)
        assert r.returncode == 134 and r.stderr == msg, (flags, r.returncode, r.stderr)
