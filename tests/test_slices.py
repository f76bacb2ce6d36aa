"""Large device batches in slices (dbtk_hip.hip: dbtk_align_batch_device, dbtk_slices.h): one call cut into slices of whole pairs, each
enqueued as the complete batch it is, slices alternating between two streams.  Every result here is the oracle's, bit-exact: counts,
kmc, nmapread and all counters.  The batches and the child process are in tests/slices.py; slices are forced with DBTK_SLICE_PAIRS =
16 or 48 (read when a context is created), timers off, the reads uploaded as tests/test_lanes.py does."""
import json
import os
import re
import subprocess
import sys

import pytest

import bind
import slices as sl
from probe_unsorted import primer

abi = bind.abi
pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
COUNTING = dict(ksize=sl.K, cthreshold=45, okam=0)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = sl.World(str(tmp_path_factory.mktemp("slices")))
    yield w
    w.close()


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    """tests/slice_plan_check.cpp (no sanitizers here: tests/test_slice_plan.py runs it under them): `exe NPAIRS SLICE` prints the plan's slice count"""
    exe = str(tmp_path_factory.mktemp("plan") / "slice_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O0", "-I", os.path.join(bind.ROOT, "danbing-tk_amd", "csrc"), "-o", exe, os.path.join(HERE, "slice_plan_check.cpp")], check=True)
    return exe


def nslices(plan_exe, npairs, slice_pairs):
    return int(subprocess.run([plan_exe, str(npairs), str(slice_pairs)], capture_output=True, text=True, check=True).stdout)


def run(world, p, batches, maxlen=None):
    """The batches back to back on a fresh context with timers off, no sync between them; the context, not yet waited for."""
    ctx = world.dbtk.context(world.g, p)
    ctx.timers_enable(False)
    devs = [sl.DevReads(r) for r in batches]
    for d in devs:
        d.align(ctx, maxlen)
    return ctx, devs


@pytest.mark.parametrize("slice_pairs", [16, 48])
def test_slice_count_is_the_plans_and_whole_contexts_stay_whole(plan_exe, slice_pairs):
    """One child with DBTK_TRACE_LAUNCHES=1 per slice size.  Batches of 1, 15, 16, 17, 47, 48, 49 and 200 pairs, half from loci and half
    background, on a counting context: the encode kernel is launched once per slice of the plan.  A walking context (threading = 2), a
    -bu context and a trace context under the same forced slice size: one encode launch for the batch.  All results the oracle's."""
    env = {k_: v for k_, v in os.environ.items() if not k_.startswith("DBTK_")}
    env.update(DBTK_TRACE_LAUNCHES="1", DBTK_SLICE_PAIRS=str(slice_pairs))
    r = subprocess.run([sys.executable, os.path.join(HERE, "slices.py"), "launches"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "slices child ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    k1, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.match(r"\[mark\] (\S+) (begin|end)", line)
        if m:
            cur = m.group(1) if m.group(2) == "begin" else None
            if cur:
                k1[cur] = 0
        elif cur and re.match(r"\[launch\] \(?k_encode_subfilter\w*\)? grid", line):
            k1[cur] += 1
    res = {}
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            d = json.loads(line[7:])
            res[d["name"]] = d
    cut = 0
    for n in sl.SIZES:
        d = res[f"n{n}"]
        assert d["npairs"] == n and d["diff"] == "", d
        want = nslices(plan_exe, n, slice_pairs)
        assert k1[f"n{n}"] == want, (n, slice_pairs, k1)
        cut += want > 1
    assert cut >= 1  # (200 pairs are cut at both sizes)
    for name in sl.WHOLE:
        assert res[name]["diff"] == "" and k1[name] == 1, (name, res[name], k1)


@pytest.mark.parametrize("slice_pairs", [16, 48])
def test_read_shapes_across_slice_boundaries(world, monkeypatch, slice_pairs):
    """Reads of 21, 22, 150 and 174 bases, slice boundaries at offsets that are no multiple of 16, an N in each mate of the pairs on both
    sides of both boundaries, a slice without a survivor before one with survivors, a last slice of one pair."""
    monkeypatch.setenv("DBTK_SLICE_PAIRS", str(slice_pairs))
    p = abi.default_params(**COUNTING)
    reads = sl.shapes(world.loci, slice_pairs)
    ctx, devs = run(world, p, [reads])
    got = ctx.counts()
    assert world.diff(world.want(p, [reads]), got) == ""
    assert int(got["counters"][abi.C_SURVIVORS]) > 0
    ctx.close()
    for d in devs:
        d.free()


@pytest.mark.parametrize("lanes", [1, 2, 3])
def test_three_batches_back_to_back_then_reset_and_again(world, monkeypatch, lanes):
    """Three batches of different sizes (13, 3 and 4 slices of 16 pairs, the last ones of 8, 15 and 1) with no sync between them, on a
    ring of one, two and three lanes: the totals are the oracle's sum; after dbtk_ctx_reset the same again."""
    monkeypatch.setenv("DBTK_SLICE_PAIRS", "16")
    monkeypatch.setenv("DBTK_LANES", str(lanes))
    p = abi.default_params(**COUNTING)
    batches = [sl.half_and_half(world.loci, n, 200 + n) for n in (200, 47, 49)]
    want = world.want(p, batches)
    ctx, devs = run(world, p, batches)
    assert world.diff(want, ctx.counts()) == ""
    ctx.reset()
    assert not ctx.counts()["counters"].any()
    for d in devs:
        d.align(ctx)
    assert world.diff(want, ctx.counts()) == ""
    ctx.close()
    for d in devs:
        d.free()


@pytest.mark.parametrize("lanes", [1, 2])
def test_error_word_of_a_middle_slice_is_reported_once(world, monkeypatch, lanes):
    """A pair of 150 bases in the second of four slices, 100 promised: the probe kernel clamps it and raises the sticky error word of
    the lane that slice ran on (with one lane in the ring the slices alternate between it and the lane made for them).
    dbtk_ctx_synchronize reports it once; it is clear afterwards, and after a reset the context counts the batch, now with the 150
    bases promised, as the oracle does."""
    monkeypatch.setenv("DBTK_SLICE_PAIRS", "16")
    monkeypatch.setenv("DBTK_LANES", str(lanes))
    p = abi.default_params(**COUNTING)
    bad = sl.too_long_in_the_middle(world.loci, 16)
    ctx, devs = run(world, p, [bad], maxlen=100)
    with pytest.raises(bind.pkg.DbtkError) as e:
        ctx.synchronize()
    assert e.value.status == abi.ERR_READ_TOO_LONG
    ctx.synchronize()  # reported once
    ctx.reset()
    devs[0].align(ctx)  # (with the 150 it holds promised)
    assert world.diff(world.want(p, [bad]), ctx.counts()) == ""
    ctx.close()
    devs[0].free()


def test_a_timed_batch_runs_whole(world, monkeypatch):
    """Timers on (a context's default): kernel_times() shows exactly one encode launch per batch, DBTK_SLICE_PAIRS forced or not."""
    monkeypatch.setenv("DBTK_SLICE_PAIRS", "16")
    p = abi.default_params(**COUNTING)
    batches = [sl.half_and_half(world.loci, n, 200 + n) for n in (200, 49)]
    ctx = world.dbtk.context(world.g, p)
    devs = [sl.DevReads(r) for r in batches]
    for d in devs:
        d.align(ctx)
    assert world.diff(world.want(p, batches), ctx.counts()) == ""
    assert ctx.kernel_times()["k_encode_subfilter"][1] == len(batches)
    ctx.close()
    for d in devs:
        d.free()


def test_default_rule_cuts_wgs_like_batches_in_halves_and_finds_its_way_back():
    """No DBTK_SLICE_PAIRS, DBTK_LANES=1, a traced child (tests/slices.py hints): batches of 2^20 pairs, twice the default's smallest
    slice.  The first WGS-like batch runs whole (no hint yet), the second and third in two halves (two encode launches; this is
    the path that makes the second lane); the all-hit batch after them is still cut (the hint is the batch before's), its halves
    report dense, and the next one runs whole again.  The totals equal those of a context created under DBTK_SLICE_PAIRS=0 (whole
    batches are what every other test holds against the oracle, which is far too slow for these 5 M pairs).  The rule itself
    — scaling, thresholds, both transitions, the seeded words — is checked value by value on the host, tests/slice_plan_check.cpp."""
    env = {k_: v for k_, v in os.environ.items() if not k_.startswith("DBTK_")}
    env.update(DBTK_TRACE_LAUNCHES="1", DBTK_LANES="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "slices.py"), "hints"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "slices child ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    k1, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.match(r"\[mark\] (\S+) (begin|end)", line)
        if m:
            cur = m.group(1) if m.group(2) == "begin" else None
            if cur:
                k1[cur] = 0
        elif cur and re.match(r"\[launch\] \(?k_encode_subfilter\w*\)? grid", line):
            k1[cur] += 1
    res = [json.loads(line[7:]) for line in r.stdout.splitlines() if line.startswith("RESULT ")]
    assert len(res) == 1 and res[0]["diff"] == "" and res[0]["survivors"] > 0, res
    assert k1 == {"wgs1": 1, "wgs2": 2, "wgs3": 2, "allhit1": 2, "allhit2": 1}, k1


def test_hints_without_override_leave_small_batches_whole(world, monkeypatch):
    """No DBTK_SLICE_PAIRS: the default slice size, which only the environment could lower — and setting it is the override.  So after the
    primer of tests/probe_unsorted.py (the hint words then say WGS-like) a batch of 200 pairs, far from two slices of the default, stays
    whole and counts as the oracle does.  A batch large enough for two default slices is the test above; the rule that cuts it is
    checked on the host by tests/slice_plan_check.cpp."""
    monkeypatch.delenv("DBTK_SLICE_PAIRS", raising=False)
    p = abi.default_params(**COUNTING)
    ctx = world.dbtk.context(world.g, p)
    ctx.align(*primer().packed())
    ctx.reset()
    ctx.timers_enable(False)
    reads = sl.half_and_half(world.loci, 200, 400)
    dev = sl.DevReads(reads)
    for _ in range(2):
        dev.align(ctx)
    assert world.diff(world.want(p, [reads, reads]), ctx.counts()) == ""
    ctx.close()
    dev.free()
