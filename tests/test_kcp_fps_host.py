"""The text-exact statistics of the FP-specific filter on the host: csrc/dbtk_kcp.h (kcp_dec4, kcp_text_float, kcp_mean_text,
kcp_sd_text, kcp_fps_inside, kcp_fps_step) compiled for the host and run under AddressSanitizer and UndefinedBehaviorSanitizer in a
stand-alone program against snprintf / strtof; and what the binding knows of the new entry points of include/dbtk_kcp.h."""
import os
import re
import subprocess

import bind

pkg = bind.pkg

NEW = ("dbtk_kcp_set_tp_only", "dbtk_kcp_fps_begin", "dbtk_kcp_fps_apply", "dbtk_kcp_fps_count", "dbtk_kcp_fps_read", "dbtk_kcp_fps_write", "dbtk_kcp_fps_times",
       "dbtk_kcp_fps_free", "dbtk_kcp_text_stats")


def test_text_exact_statistics_under_sanitizers(tmp_path):
    src = os.path.join(bind.ROOT, "tests", "kcp_fps_check.cpp")
    exe = str(tmp_path / "kcp_fps_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I",
                    os.path.join(bind.ROOT, "danbing-tk_amd", "csrc"), "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "kcp fps ok\n", r.stdout + r.stderr


def test_binding_knows_the_new_entry_points_and_neither_version_moved():
    hdr = open(os.path.join(bind.ROOT, "include", "dbtk_kcp.h")).read()
    main = open(os.path.join(bind.ROOT, "include", "dbtk.h")).read()
    assert "#define DBTK_KCP_API_VERSION 1u" in hdr and pkg.abi.KCP_API_VERSION == 1
    assert re.search(r"#define\s+DBTK_ABI_VERSION\s+11u?\b", main) and pkg.abi.ABI_VERSION == 11
    lib = pkg.Dbtk()
    for s in NEW:
        assert s in pkg.EXPORTS_KCP and hasattr(lib.L, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    assert hasattr(pkg, "KcpFps") and hasattr(pkg, "kcp_text_stats") and hasattr(pkg.Kcp, "set_tp_only")
    assert (pkg.abi.KCP_FPS_MI_NONE, pkg.abi.KCP_FPS_MA_NONE) == (255, 0)
    lib.L.dbtk_kcp_api_version.restype = bind.C.c_uint32
    assert lib.L.dbtk_kcp_api_version() == 1


def test_text_stats_checks_its_arguments_before_it_asks_for_a_device():
    lib = pkg.Dbtk()
    for n, s, q in (([0], [0], [0]), ([2], [4], [7])):  # no reads; n * sumsq < sum^2
        try:
            pkg.kcp_text_stats(lib, n, s, q)
        except pkg.DbtkError as e:
            assert e.status == pkg.abi.ERR_ARG and "moments" in str(e)
        else:
            raise AssertionError(f"{(n, s, q)} was accepted")
