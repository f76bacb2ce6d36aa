"""The ring of lanes of a context (dbtk_hip.hip: struct Lane, DBTK_LANES = 1..3): what every lane owns must be found, cleared and
sized on every position of the ring.  Companions of test_gpu_parity.py::test_device_entry_reports_a_read_longer_than_promised,
test_ingest.py::test_device_reader_asynchronous_blocks_and_flags and test_gpu_parity.py::test_bait_and_bubble_gates_match_oracle,
on their small cases."""
import ctypes as C

import numpy as np
import pytest

import bind
import synth
from cases import make_case

abi = bind.abi
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dbtk():
    return bind.pkg.Dbtk()


@pytest.fixture(scope="module")
def oracle():
    return bind.Oracle()


def _blocks(ing, data, chunk):
    """Every block of `data` submitted and waited for, one at a time: (slot, info) of each."""
    nblocks = (len(data) + chunk - 1) // chunk
    for j in range(nblocks):
        slot = ing.submit(data[j * chunk:(j + 1) * chunk], j == nblocks - 1)
        info = ing.wait(slot)
        assert info.flags == 0
        yield slot, info


def _text_of(reads, fn, fastq):
    synth.write_fasta(reads, fn, fastq=fastq)
    return open(fn, "rb").read()


@pytest.mark.parametrize("lanes,clean", [(1, 3), (2, 3), (3, 1), (3, 3)])
def test_error_word_is_reported_from_every_ring_position(dbtk, tmp_path, lanes, clean, monkeypatch):
    """A read longer than dbtk_align_batch_device was promised is clamped by the probe kernel, which raises the sticky error word
    of the lane the batch ran on; dbtk_ctx_synchronize reports it once, wherever in the ring that lane is by then.  With three
    lanes and one clean batch after it, the lane that holds the word is neither the current one nor the next."""
    monkeypatch.setenv("DBTK_LANES", str(lanes))
    c = make_case("mixed", str(tmp_path))
    g = dbtk.load(c.prefix, c.k, c.qc_file)
    seq, off = c.reads.packed()
    p = abi.default_params(ksize=c.k, **dict(c.param_sets[0], okam=0))
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    d_seq, d_off = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_seq), len(seq) + 64) == 0 and hip.hipMalloc(C.byref(d_off), off.nbytes) == 0
    assert hip.hipMemcpy(d_seq, seq.ctypes.data_as(C.c_void_p), len(seq), 1) == 0
    assert hip.hipMemcpy(d_off, off.ctypes.data_as(C.c_void_p), off.nbytes, 1) == 0
    maxlen = int(np.diff(off.astype(np.int64)).max())
    ctx = dbtk.context(g, p)
    ctx.align_device(d_seq.value, d_off.value, c.reads.npairs, 100)      # the reads are 150 bases
    for _ in range(clean):
        ctx.align_device(d_seq.value, d_off.value, c.reads.npairs, maxlen)
    with pytest.raises(bind.pkg.DbtkError) as e:
        ctx.synchronize()
    assert e.value.status == abi.ERR_READ_TOO_LONG
    ctx.synchronize()  # reported once
    ctx.close()
    hip.hipFree(d_seq); hip.hipFree(d_off)
    g.close()


def test_merged_batches_on_three_lanes_and_reset_of_every_lane(dbtk, tmp_path, monkeypatch):
    """dbtk_ingest_align_merged with three lanes in the ring: batches of >= 150 pairs, each merged in the buffers of the next lane, add
    up to the host-buffer result; and dbtk_ctx_reset discards two appended blocks that were not aligned yet: a flush after it finds
    nothing, every accumulator is zero."""
    monkeypatch.setenv("DBTK_LANES", "3")
    c = make_case("mixed", str(tmp_path))
    g = dbtk.load(c.prefix, c.k)
    p = abi.default_params(ksize=c.k, cthreshold=45, okam=0)
    seq, off = c.reads.packed()
    ctx = dbtk.context(g, p)
    ctx.align(seq, off)
    want = ctx.counts()
    ctx.close()
    data = _text_of(c.reads, str(tmp_path / "reads.fa"), False)
    chunk = 16384
    assert len(data) > 2 * chunk
    ctx = dbtk.context(g, p)
    ing = bind.pkg.Ingest(ctx, False, 0, chunk, nslots=4, with_spans=False)
    for slot, _ in _blocks(ing, data, chunk):
        ing.align_merged(slot, 150)
    ing.align_merged(None, 0, flush=True)
    got = ctx.counts()
    ing.close()
    ctx.close()
    for k_ in ("counts", "kmc", "nmapread", "counters"):
        assert (want[k_] == got[k_]).all(), k_
    ctx = dbtk.context(g, p)
    ing = bind.pkg.Ingest(ctx, False, 0, chunk, nslots=4, with_spans=False)
    for j in range(2):
        info = ing.wait(ing.submit(data[j * chunk:(j + 1) * chunk], False))
        assert info.flags == 0 and info.nkept > 0
        ing.align_merged(j, 10 ** 9)  # appended, not aligned
    ctx.reset()
    ing.align_merged(None, 0, flush=True)
    z = ctx.counts()
    assert not z["counts"].any() and not z["kmc"].any() and not z["nmapread"].any() and not z["counters"].any()
    ing.close()
    ctx.close()
    g.close()


@pytest.mark.skipif(not synth.have_ref(), reason="needs oracle/_ref (ktools serialize-bt builds the bait DB)")
@pytest.mark.parametrize("lanes", [2, 3])
def test_quality_masks_are_per_lane(dbtk, oracle, tmp_path, lanes, monkeypatch):
    """-b with FASTQ qualities through the device reader, every block aligned without waiting for the one before (sync = 0): the
    quality masks the probe kernel writes for a chunk are read by the resolve kernel of the same batch, so every lane has its own
    buffer for them.  The blocks of 16 KB go round the lanes and add up to the oracle's result for the whole read set.
    At this size the kernels of two lanes need not overlap: the test guards the sizing and the wiring of the per-lane buffer, it
    does not prove that two lanes can no longer meet in one."""
    monkeypatch.setenv("DBTK_LANES", str(lanes))
    loci = synth.make_loci(nloci=10, nhap=3, flank=500, seed=61, shared_frac=0.3)
    d = str(tmp_path)
    pref = synth.build_rpgg_with_reference(loci, d, k=21)
    reads = synth.sim_reads(loci, npairs=1500, seed=62, sub=0.01, indel=0.002, nrate=0.002, chimeric=0.3, background=0.1, with_qual=True)
    bait = synth.make_bait_db(loci, reads, d)
    go = oracle.load(pref, 21)
    oracle.load_bait(go, bait)
    g = dbtk.load(pref, 21, bait_file=bait)
    seq, off = reads.packed()
    qual = np.frombuffer(b"".join(reads.quals), np.uint8).copy()
    p = abi.default_params(ksize=21, bait=1, cthreshold=20, okam=0)
    o = oracle.align_ex(go, p, seq, off, qual)
    data = _text_of(reads, str(tmp_path / "reads.fq"), True)
    chunk = 16384
    assert len(data) > 2 * lanes * chunk
    ctx = dbtk.context(g, p)
    ing = bind.pkg.Ingest(ctx, True, 0, chunk, nslots=4, with_spans=False)
    npairs = 0
    for slot, info in _blocks(ing, data, chunk):
        ing.align(slot, info, sync=False)
        npairs += info.nkept
    ctx.synchronize()
    res = ctx.counts()
    ing.close()
    ctx.close()
    assert npairs == reads.npairs
    co = np.zeros(g.ntrkmers, np.uint64)
    np.add.at(co, g.output_order().astype(np.int64), o["counts_file"])
    assert (co == res["counts"]).all(), f"{int((co != res['counts']).sum())} k-mer counts differ"
    assert (o["kmc"] == res["kmc"]).all() and (o["nmapread"] == res["nmapread"]).all()
    assert (o["counters"] == res["counters"]).all(), (o["counters"], res["counters"])
    assert res["counters"][abi.C_BAITFILTERED] > 0
    oracle.free(go)
    g.close()
