"""What danbing-tk-pred --window-* decides without a device: flag parsing, refusals, the usage text; and the window planning
(csrc/dbtk_pred_plan.h) under AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone host program."""
import os
import re
import subprocess

import bind

pkg = bind.pkg
EXE = os.path.join(bind.ROOT, "danbing-tk_amd", "bin", "danbing-tk-pred")


def pred(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True)


def test_usage_lists_the_window_flags():
    r = pred()
    assert r.returncode == 0 and "--window-rows <INT>" in r.stderr and "--window-bytes <INT>" in r.stderr


def test_window_flags_are_refused_before_any_file_or_device(tmp_path):
    files = ["no.meta", "no.ikmer", "raw", "cor", "bias"]
    for flag in ("--window-rows", "--window-bytes"):
        r = pred(flag, "0", *files)
        assert r.returncode == 1 and r.stderr == f"{flag} must be positive\n"
        for bad in ("abc", "12x", "-3", "", "1e6"):
            r = pred(flag, bad, *files)
            assert r.returncode == 1 and r.stderr == f"{flag}: not a number: {bad}\n", (flag, bad, r.stderr)
    r = pred("--window-rows")                     # the value is missing
    assert r.returncode == 1 and "invalid option" in r.stderr
    assert not any(os.path.exists(f) for f in files)


def test_conflicting_window_flags(tmp_path):
    gt = tmp_path / "gt.meta"
    gt.write_text("a.trkmc.ar\t30.5\nb.trkmc.ar\t28.25\n")                  # 2 samples: 800 bytes are 100 k-mers
    out = [str(tmp_path / x) for x in ("raw", "cor", "bias")]
    r = pred("--window-rows", "50", "--window-bytes", "800", str(gt), "no.ikmer", *out)
    assert r.returncode == 1 and "disagree" in r.stderr and "100 k-mers" in r.stderr
    r = pred("--window-bytes", "7", str(gt), "no.ikmer", *out)             # less than one k-mer of 2 samples
    assert r.returncode == 1 and "holds no k-mer" in r.stderr
    r = pred("--window-rows", "100", "--window-bytes", "807", str(gt), str(tmp_path / "no.ikmer"), *out)   # they agree: the run goes on to ikmer.meta
    assert r.returncode == 1 and "disagree" not in r.stderr
    assert not any(os.path.exists(f) for f in out)


def test_binding_knows_the_window_entry_points():
    hdr = open(os.path.join(bind.ROOT, "include", "dbtk_pred.h")).read()
    lib = pkg.Dbtk()
    for s in ("dbtk_pred_create_windowed", "dbtk_pred_create_windowed_from_file", "dbtk_pred_window", "dbtk_pred_window_submit", "dbtk_pred_window_outputs",
              "dbtk_pred_window_outputs_pinned", "dbtk_pred_window_stage", "dbtk_pred_max_rows"):
        assert s in pkg.EXPORTS_PRED and hasattr(lib.L, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    assert hasattr(pkg, "PredWindowed")


def test_window_planning_under_sanitizers(tmp_path):
    src = os.path.join(bind.ROOT, "tests", "pred_plan_check.cpp")
    exe = str(tmp_path / "pred_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(bind.ROOT, "danbing-tk_amd", "csrc"),
                    "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "window planning ok\n", r.stdout + r.stderr
