"""The profile table of --bait-profile on the host: csrc/dbtk_kcp.h (slot claim, multiplicity step, rehash move) compiled for the host
with its own accessor and run under AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone program; and what the binding
knows of include/dbtk_kcp.h."""
import os
import re
import subprocess

import bind

pkg = bind.pkg


def test_profile_table_under_sanitizers(tmp_path):
    src = os.path.join(bind.ROOT, "tests", "kcp_table_check.cpp")
    exe = str(tmp_path / "kcp_table_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I",
                    os.path.join(bind.ROOT, "danbing-tk_amd", "csrc"), "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "kcp table ok\n", r.stdout + r.stderr


def test_binding_knows_the_profile_entry_points_and_the_abi_did_not_move():
    hdr = open(os.path.join(bind.ROOT, "include", "dbtk_kcp.h")).read()
    assert "#define DBTK_KCP_API_VERSION 1u" in hdr and pkg.abi.KCP_API_VERSION == 1 and pkg.abi.ABI_VERSION == 11
    lib = pkg.Dbtk()
    for s in ("dbtk_kcp_api_version", "dbtk_kcp_create", "dbtk_kcp_add", "dbtk_kcp_count", "dbtk_kcp_read", "dbtk_kcp_write", "dbtk_kcp_reset", "dbtk_kcp_free"):
        assert s in pkg.EXPORTS_KCP and hasattr(lib.L, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    lib.L.dbtk_kcp_api_version.restype = bind.C.c_uint32
    assert lib.L.dbtk_kcp_api_version() == 1


def test_create_checks_its_arguments_before_it_asks_for_a_device():
    lib = pkg.Dbtk()
    for k in (0, 1, 32, 64):
        try:
            pkg.Kcp(lib, k, 4)
        except pkg.DbtkError as e:
            assert e.status == pkg.abi.ERR_ARG and "ksize" in str(e)
        else:
            raise AssertionError(f"ksize {k} was accepted")
    for nloci in (0, 1 << 31):
        try:
            pkg.Kcp(lib, 21, nloci)
        except pkg.DbtkError as e:
            assert e.status == pkg.abi.ERR_ARG and "nloci" in str(e)
        else:
            raise AssertionError(f"nloci {nloci} was accepted")
