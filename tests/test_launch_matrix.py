"""Every instance in the launcher's nine kernel tables (dbtk_hip.hip) is run on the device against the oracle, or shown unreachable; and
the lean kernels are run at every k they serve (19 .. 26), not only 21 and 25.

tests/launch_matrix.py holds the scenarios, the restatement of launch_batch's selection rules (declared) and the child-process driver.
GPU part: one child per environment set (the launcher reads its switches once per process) with DBTK_TRACE_LAUNCHES=1; every scenario is
bit-exact, launches exactly the instances the model declares, and the instances it claims show work in the path statistics.  The union
over the sets is the 73 names of the built library minus UNREACHABLE.
CPU part: the tables' dimensions and the library's names agree; the model claims every reachable name; every batch gives the oracle
something to do; the image classes are the designed ones; the emulator agrees with the oracle on the k-class scenarios (so a failure on
the device can be told from a bug in a kernel body)."""
import functools
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import bind
import launch_matrix as lm

abi = bind.abi
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def O():
    return bind.Oracle()


@pytest.fixture(scope="module")
def E():
    return bind.Emu()


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("launch_matrix"))


@pytest.fixture(scope="module")
def oracle_handles(O, tmp):
    """(oracle handle with its graph, prefix) per (loci, k): loaded once, read by every CPU test."""
    cache = {}

    def get(sc):
        key = (sc.loci, sc.k)
        if key not in cache:
            pref = lm.make_prefix(tmp, sc.loci, sc.k)
            go = O.load(pref, sc.k)
            O.load_graph(go, pref + ".graph.kmers")
            cache[key] = (go, pref)
        return cache[key]
    return get


# ------------------------------------------------------------------ CPU --
def test_tables_have_73_instances_and_the_library_names_them():
    dims = lm.table_dims()
    assert len(dims) == 9, dims
    assert sum(int(np.prod(d)) for d in dims.values()) == 73, dims
    names = lm.library_names()
    assert len(names) == 73, names


def test_unreachable_is_short_and_named_by_the_library():
    assert len(lm.UNREACHABLE) <= 3 and set(lm.UNREACHABLE) <= set(lm.library_names())
    assert all(len(why) > 80 for why in lm.UNREACHABLE.values())


def test_model_claims_every_reachable_instance():
    got = set()
    for sc in lm.scenarios():
        got |= lm.claimed(sc)
    names = set(lm.library_names())
    assert got <= names, sorted(got - names)
    assert names - got == set(lm.UNREACHABLE), sorted(names - got)
    assert sorted({sc.part for sc in lm.scenarios()}) == sorted(lm.PARTS)


def test_no_rule_of_the_model_reaches_the_unreachable():
    """Over every k, length, mode, hint state and environment set the model can express — not only the scenarios."""
    class Any:
        pass
    for env in lm.ENV_SETS.values():
        for k in range(15, 32):
            for maxlen in list(range(k, 300, 7)) + [110, 174, 175, 172, 171]:
                for params in list(lm.MODES.values()) + [dict(okam=0, bubbles=abi.BUBBLES_TABLE)]:
                    for primer in (False, True):
                        sc = Any()
                        sc.k, sc.maxlen, sc.params, sc.primer = k, maxlen, params, primer
                        assert not (lm.declared(sc, env)[0] & set(lm.UNREACHABLE))


def test_scenarios_select_the_lengths_they_name():
    for sc in lm.scenarios():
        assert sc.maxlen == sc.L, sc.name
        lens = {len(s) for s in sc.reads.seqs}
        assert {sc.k, sc.k + 1, 60} <= lens, sc.name
        assert any(t.startswith("tail") for t in sc.reads.titles), sc.name  # pairs that end inside the TR at full length
        assert 100 <= sc.reads.npairs <= 500, (sc.name, sc.reads.npairs)
    for k in lm.K_CLASSES + (21, 25):
        l3, l5 = lm.lean_limits(k)
        m = lm.mz_m_for_k(k)
        assert (l3, l5) == (96 + m - 1, 160 + m - 1)
    # the first length past the last form selects the general probe kernel; k = 18 and 27 do at any length
    for sc in lm.scenarios():
        general = any(n.startswith("(k_probe_general") for n in lm.declared(sc, sc.env)[0])
        assert general == (sc.L > lm.lean_limits(sc.k)[1] or not 19 <= sc.k <= 26 or bool(sc.params.get("bubbles"))), sc.name


def test_even_k_loci_carry_a_self_complementary_kmer_read_on_both_strands():
    for k in (20, 22, 24, 26):
        pal = lm._palindrome(k, 900 + k)
        assert (lm.synth.revcomp(pal) == pal).all()
        loci = lm.loci_plain(k)
        assert all(pal.tobytes() in loci.haps[h][0].tobytes() for h in range(loci.nhap))
        sc = next(s for s in lm.scenarios() if s.k == k and s.part == "default:k")
        hits = [i for i, s in enumerate(sc.reads.seqs) if pal.tobytes() in s]
        assert len(hits) >= 4 and {i % 2 for i in hits} == {0, 1}, (k, hits)  # in first and second mates: both strands


def image_lg(view, k):
    """bind.locus_image_lg of an RPGG view.  Loci that share no k-mer have no vv list (a null pointer, which that function does not take):
    it then gets a list of one unused word — no index value refers to it."""
    if not view.nvv:
        import ctypes as C
        import types
        view = types.SimpleNamespace(nkeys=view.nkeys, nloci=view.nloci, vals=view.vals, nvv=1, vv=C.cast((C.c_uint32 * 1)(0), bind.u32p))
    return bind.locus_image_lg(view, k)[0].copy()


def test_image_classes_come_out_as_designed(E, oracle_handles):
    """The three groups of loci_classes() are XS, S and L at k = 21; and every scenario that claims a class has a locus of that class
    with at least LOC_MIN_PAIRS pairs (bind.locus_image_lg: the sizes as dbtk_locus.h computes them)."""
    lg_of = {}
    for sc in lm.scenarios():
        if not sc.classes:
            continue
        key = (sc.loci, sc.k)
        if key not in lg_of:
            g = E.load(oracle_handles(sc)[1], sc.k)
            lg_of[key] = image_lg(g.view(), sc.k)
            g.close()
        lg = lg_of[key]
        cls = [0 if l <= 9 else l - 9 for l in lg[:-1]]  # (the last locus has too few pairs for an item)
        assert sc.per_locus >= 16 and lm.FEW < 16
        assert {lm.CLASSES.index(c) for c in sc.classes} <= set(cls), (sc.name, lg)
    n = lm.N_PER_CLASS
    assert list(lg_of[("classes", 21)]) == [9] * n + [10] * n + [11] * n, lg_of[("classes", 21)]


def test_every_batch_gives_the_oracle_work(O, oracle_handles):
    for sc in lm.scenarios():
        go, _ = oracle_handles(sc)
        _, o = lm.oracle_run(O, go, sc)
        c = o["counters"]
        assert lm.nontrivial(sc, o), (sc.name, c)
        assert lm.assigned(sc, c) >= sc.reads.npairs // 4, (sc.name, c)  # (most pairs assigned: a miscount would show)
        if sc.walking:
            assert o["nres"] > 0 and int(c[abi.C_THREADING]) > 0, sc.name


def test_a_kernel_one_position_short_would_miscount(O, oracle_handles):
    """The pairs at the length limit carry locus k-mers in their last positions: without the last base of every longest read the oracle's
    counts are other counts — so would those of an instance with too few positions per lane."""
    for sc in lm.scenarios():
        if sc.params != lm.MODES["okam0"] or sc.primer or sc.part not in ("default", "default:k"):
            continue
        go, _ = oracle_handles(sc)
        p, o = lm.oracle_run(O, go, sc)
        cut = lm.synth.Reads(seqs=[s[:-1] if len(s) == sc.L else s for s in sc.reads.seqs], titles=sc.reads.titles)
        oc = O.align(go, p, *cut.packed(), trace=False)
        assert (oc["counts_file"] != o["counts_file"]).any(), sc.name


def _emu_scenario(E, O, oracle_handles, tables, sc):
    go, pref = oracle_handles(sc)
    key = (sc.loci, sc.k)
    if key not in tables:
        g = E.load(pref, sc.k, flags=abi.LOAD_GRAPH)
        tables[key] = (g, E.tables(g), g.output_order().astype(np.int64))
    g, T, order = tables[key]
    p, o = lm.oracle_run(O, go, sc)
    seq, off = sc.reads.packed()
    if sc.primer:
        os.environ["EMU_NO_LOCUS"] = "1"
    try:
        b = E.align(g, T, p, seq, off, grid_k1=3, grid_pair=3)
    finally:
        os.environ.pop("EMU_NO_LOCUS", None)
    walk = E.walk_results(sc.reads.npairs) if sc.walking else None
    return lm.compare(sc, g, order, o, b, b["recs"], walk, g.nloci)


@pytest.mark.parametrize("k", lm.K_CLASSES)
def test_emulated_bodies_match_the_oracle_at_the_lean_k_classes(k, E, O, oracle_handles):
    """The kernel bodies on the emulator, the k-class scenarios of the default set (sorted and locus-resident; the unsorted ones with every
    pair through the lean body): counts, counters, records and walk results."""
    tables = {}
    E.path_stats()
    E.locus_stats()
    n = 0
    for sc in lm.by_part("default:k"):
        if sc.k != k:
            continue
        assert _emu_scenario(E, O, oracle_handles, tables, sc) == "", sc.name
        n += 1
    ps = E.path_stats()
    took = E.locus_stats()[0]  # pairs the locus-resident probe body took, per class (k = 26 has no images)
    assert n == 14 and (sum(took) > 0) == (k != 26) and ps["lean_done"] > 0 and (ps["fused_done"] > 0) == (k != 26), (n, took, ps)
    for g, T, _ in tables.values():
        E.L.emu_tables_free(T)
        g.close()


# ------------------------------------------------------------------ GPU --
LAUNCH = re.compile(r"^\[launch\] (.+) grid \d+ block \d+$")
MARK = re.compile(r"^\[scenario\] (.+) (begin|end)$")


def parse_launches(stderr):
    """{scenario: [names launched between its delimiters, in order]}"""
    out, cur = {}, None
    for line in stderr.splitlines():
        m = MARK.match(line)
        if m:
            cur = m.group(1) if m.group(2) == "begin" else None
            if cur:
                out[cur] = []
            continue
        m = LAUNCH.match(line)
        if m and cur:
            out[cur].append(m.group(1))
    return out


@functools.lru_cache(maxsize=None)
def run_child(part):
    """One child for the part: its set's switches and DBTK_TRACE_LAUNCHES=1.  Returns (exit status, {name: result}, {name: launches}, s)."""
    env = {k_: v for k_, v in os.environ.items() if not k_.startswith("DBTK_")}
    env.update(lm.ENV_SETS[part.split(":")[0]], DBTK_TRACE_LAUNCHES="1")
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(HERE, "launch_matrix.py"), part], capture_output=True, text=True, env=env, timeout=600)
    dt = time.time() - t0
    res = {}
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            d = json.loads(line[7:])
            res[d["name"]] = d
    return r.returncode, res, parse_launches(r.stderr), dt, r.stdout[-1500:] + r.stderr[-1500:]


def check_part(part):
    """Returns {instance: scenario} of the instances launched with evidence of work."""
    rc, res, launches, dt, tail = run_child(part)
    print(f"{part}: {len(res)} results in {dt:.1f} s")
    assert rc == 0, tail
    table = set(lm.library_names())
    worked = {}
    scs = lm.by_part(part)
    assert scs
    for sc in scs:
        assert sc.name in res, (sc.name, tail)
        d = res[sc.name]
        assert d["exact"], (sc.name, d["diff"])
        names, sorts = lm.declared(sc, sc.env)
        got = launches[sc.name]
        assert set(got) & table == names, (sc.name, sorted(set(got) & table), sorted(names))
        assert ("k_surv_key" in got) == sorts, (sc.name, got)  # the sort runs exactly where the hints say "sorted"
        assert not set(got) & set(lm.UNREACHABLE)
        if not sorts:  # ... and no pair went through the locus-resident kernel or onto its rest list
            assert sum(d["ps"]["probe_pairs"]) == 0 and d["ps"]["probe_rest"] == 0, (sc.name, d["ps"])
        for n in lm.claimed(sc):
            assert lm.evidence(sc, n, d["ps"], d["ctr"]), (sc.name, n, d["ps"], d["ctr"])
            worked.setdefault(n, sc.name)
    for name, d in res.items():
        assert d["exact"], (name, d["diff"])  # (the -ae text scenarios too)
    return worked


@pytest.mark.gpu
@pytest.mark.parametrize("part", lm.PARTS)
def test_scenarios_are_exact_and_launch_what_the_model_declares(part):
    check_part(part)


@pytest.mark.gpu
def test_every_instance_is_launched_with_evidence_or_unreachable():
    worked, launched = {}, set()
    for part in lm.PARTS:
        worked.update(check_part(part))
        for got in run_child(part)[2].values():
            launched |= set(got)
    names = set(lm.library_names())
    assert len(names) == 73
    assert set(worked) | set(lm.UNREACHABLE) == names, sorted(names - set(worked) - set(lm.UNREACHABLE))
    assert not launched & set(lm.UNREACHABLE)
