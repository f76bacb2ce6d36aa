"""The slice plan of dbtk_align_batch_device (danbing-tk_amd/csrc/dbtk_slices.h), on the host: tests/slice_plan_check.cpp, a stand-alone
program with its own main, built with the address and undefined-behaviour sanitizers and run directly.  It goes over batches of
0, 1, 15, 16, 17, ... 2^32 - 2 pairs, slices of 1, 16, 48, 2^19 .. 2^21 pairs and the cap of 64 slices, and asserts that the slices
are contiguous, add up to the batch, are whole tiles of 16 pairs except the last, are never empty, and that a batch with fewer than
two full slices stays whole; then the rule that decides without DBTK_SLICE_PAIRS (dbtk_slices::decide): a slice's survivors scaled to
the call's pairs, the sort's threshold per batch, sorted and mostly-surviving launches never WGS-like, both transitions and the
words the first slices are seeded with.  No GPU."""
import os
import subprocess

import bind


def build_check(tmp_path):
    src = os.path.join(bind.ROOT, "tests", "slice_plan_check.cpp")
    exe = str(tmp_path / "slice_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(bind.ROOT, "danbing-tk_amd", "csrc"),
                    "-o", exe, src], check=True)
    return exe


def test_slice_planning_under_sanitizers(tmp_path):
    exe = build_check(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "slice planning ok\n", r.stdout + r.stderr
    # the form tests/test_slices.py asks for the number of slices in
    for npairs, slice_pairs, want in ((17, 16, 1), (49, 16, 4), (200, 48, 5), (5_000_000, 1 << 20, 5)):
        r = subprocess.run([exe, str(npairs), str(slice_pairs)], capture_output=True, text=True)
        assert r.returncode == 0 and int(r.stdout) == want, (npairs, slice_pairs, r.stdout + r.stderr)
