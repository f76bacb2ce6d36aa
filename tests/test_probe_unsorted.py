"""The lean probe kernel (dbtk_probe2.h) on a survivor list that was not sorted: its instances without the cache of overflow look-ups
(body_probe2's CACHE = false).

CPU part: the kernel body on the emulator, the named cases against the oracle, in both forms.  The emulator's driver does not choose a
form and runs the body's default, the one without the cache; tests/emu/emu_p2cache.cpp, compiled here, is the same driver with the cached
form as the default.  Every pair goes through the lean body (EMU_NO_LOCUS=1); the cached form also takes the rest lists the
locus-resident body leaves, as on the device.
GPU part: the batches of tests/probe_unsorted.py, each built to hit one edge, on a context whose hint words say "not sorted"; then the
same batches with the cache forced off and on (DBTK_P2_CACHE, read once per process: a child process per setting)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bind
import cases
import probe_unsorted as pu

abi = bind.abi
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def O():
    return bind.Oracle()


@pytest.fixture(scope="module")
def E():
    return bind.Emu()


@pytest.fixture(scope="module")
def E_cached(tmp_path_factory):
    """The emulator built from tests/emu/emu_p2cache.cpp: the lean probe body with the wave's cache of overflow look-ups."""
    emu, csrc = os.path.join(HERE, "emu"), os.path.join(HERE, "..", "danbing-tk_amd", "csrc")
    lib = str(tmp_path_factory.mktemp("emu_p2cache") / "libdbtk_emu_p2cache.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-w", "-DDBTK_LOC_Q=40", "-o", lib, os.path.join(emu, "emu_p2cache.cpp"),
                    os.path.join(csrc, "dbtk_rpgg.cpp"), "-lpthread"], check=True)
    old = os.environ.get("DBTK_EMU_LIB")
    os.environ["DBTK_EMU_LIB"] = lib
    try:
        return bind.Emu()
    finally:
        if old is None:
            os.environ.pop("DBTK_EMU_LIB", None)
        else:
            os.environ["DBTK_EMU_LIB"] = old


@pytest.fixture(scope="module")
def dbtk():
    return bind.pkg.Dbtk()


@pytest.fixture(scope="module")
def SC():
    return pu.scenarios()


def _emu_lean_alone(E, O, prefix, k, qc_file, reads, param_sets, grids=((11, 3),), no_locus=True):
    """Every pair through the lean body (no_locus; otherwise what the locus-resident body leaves), with and without a record buffer (the
    body's unfused and fused forms).  Returns the keys level 1 of the tables turned away, and the pairs the lean body resolved itself."""
    go = O.load(prefix, k, qc_file)
    g = E.load(prefix, k, qc_file)
    T = E.tables(g)
    order = g.output_order().astype(np.int64)
    seq, off = reads.packed()
    E.probe_stats()
    E.path_stats()
    if no_locus:
        os.environ["EMU_NO_LOCUS"] = "1"
    try:
        for kw in param_sets:
            for extra in (dict(trace=1), dict(okam=0)):
                p = abi.default_params(ksize=k, **{**kw, **extra})
                a = O.align(go, p, seq, off, trace=bool(p.trace))
                co = np.zeros(g.ntrkmers, np.uint64)
                np.add.at(co, order, a["counts_file"])
                for gk1, gp in grids:
                    b = E.align(g, T, p, seq, off, grid_k1=gk1, grid_pair=gp)
                    assert (co == b["counts"]).all(), (kw, extra)
                    assert (a["kmc"] == b["kmc"]).all() and (a["nmapread"] == b["nmapread"]).all(), (kw, extra)
                    assert (a["counters"] == b["counters"]).all(), (kw, extra, a["counters"], b["counters"])
                    if p.trace:
                        d = bind.recs_equal(a["recs"], b["recs"], reads.npairs)
                        assert d < 0, f"{bind.rec_str(a['recs'][d])}\n{bind.rec_str(b['recs'][d])}"
    finally:
        os.environ.pop("EMU_NO_LOCUS", None)
    general, lean, turned = E.probe_stats()
    ps = E.path_stats()
    assert not no_locus or sum(ps["probe_pairs"]) == 0  # (no locus-resident body)
    E.L.emu_tables_free(T)
    O.free(go)
    g.close()
    return general, lean, turned, ps["lean_done"]


NAMED = ["clean", "mixed", "shared", "spliced", "lengths", "short21", "short25", "k25", "kf", "qc"]


@pytest.mark.parametrize("case", NAMED)
def test_lean_body_without_cache_matches_oracle(case, O, E, tmp_path):
    c = cases.make_case(case, str(tmp_path))
    general, lean, turned, done = _emu_lean_alone(E, O, c.prefix, c.k, c.qc_file, c.reads, c.param_sets)
    assert (lean > 0 and general == 0) if case in cases.LEAN_PROBE else (general > 0 and lean == 0), (general, lean)
    if case == "shared":
        assert turned > 0  # (keys in the overflow table: looked up without the cache)
    if case in ("clean", "shared", "qc", "spliced", "k25"):
        assert done > 0


@pytest.mark.parametrize("case", NAMED)
def test_lean_body_with_cache_matches_oracle(case, O, E_cached, tmp_path):
    """The cached form (what a list in locus order runs on the device): the cache's set-up, its reads, the token election and the insert,
    over the whole list and over the rest list of the locus-resident body."""
    E = E_cached
    c = cases.make_case(case, str(tmp_path))
    _emu_lean_alone(E, O, c.prefix, c.k, c.qc_file, c.reads, c.param_sets[:1], no_locus=False)
    general, lean, turned, done = _emu_lean_alone(E, O, c.prefix, c.k, c.qc_file, c.reads, c.param_sets)
    assert (lean > 0 and general == 0) if case in cases.LEAN_PROBE else (general > 0 and lean == 0), (general, lean)
    if case == "shared":
        assert turned > 0  # (keys in the overflow table: looked up without the cache)
    if case in ("clean", "shared", "qc", "spliced", "k25"):
        assert done > 0


@pytest.mark.parametrize("form", ["without", "cached"])
def test_overflow_batch_has_overflow_keys(form, O, E, E_cached, SC, tmp_path):
    """The tandem-repeat loci of the GPU part's "overflow" batch do fill buckets (their keys are in the overflow table), and the lean body
    looks them up right on the emulator in both forms, for more than one wave and for one (one wave: the pairs of a locus meet one cache)."""
    loci, batches, param_sets, _ = SC["overflow"]
    pref = cases._np_rpgg(str(tmp_path), "overflow", loci, pu.K)
    general, lean, turned, done = _emu_lean_alone(E_cached if form == "cached" else E, O, pref, pu.K, None, batches[0], param_sets[:1],
                                                  grids=((3, 3), (2, 1)))
    assert lean > 0 and general == 0 and turned > 0 and done > 0


GPU_BATCHES = ["ranges", "none", "one", "lengths", "n_bases", "overflow", "shared", "spliced", "two_batches", "chunks"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_BATCHES)
def test_unsorted_batch_matches_oracle(name, dbtk, O, SC, tmp_path):
    lean, surv = pu.run_scenario(name, dbtk, O, str(tmp_path), SC)
    print(f"{name}: survivors {surv}, {lean} pairs resolved by the lean kernel")
    if name == "none":
        assert set(surv) == {0} and lean == 0
    elif name == "one":
        assert set(surv) == {1} and lean > 0
    elif name == "two_batches":
        assert surv[1] < surv[0] and lean > 0
    else:
        assert min(surv) > 0 and lean > 0


def test_batches_cover_the_list():
    assert sorted(GPU_BATCHES) == sorted(pu.scenarios())


@pytest.mark.gpu
@pytest.mark.parametrize("cache", ["0", "1"])
def test_unsorted_batches_cache_forced(cache):
    """The same batches with the wave's cache of overflow look-ups forced off and on, whatever the list: never a matter of results."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "probe_unsorted.py")], capture_output=True, text=True,
                       env=dict(os.environ, DBTK_P2_CACHE=cache), timeout=600)
    n = len(GPU_BATCHES)
    assert r.returncode == 0 and f"{n}/{n} batches bit-exact" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
