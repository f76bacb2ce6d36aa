"""danbing-tk_amd — MI355X-native `danbing-tk align` hot path.

Import with importlib.import_module("danbing-tk_amd") (the hyphen follows the
reference's name).  `abi` mirrors include/dbtk.h; `Dbtk` binds the C-ABI of
libdbtk_hip.so (hand-written HIP for gfx950, built by csrc/Makefile) and raises
if that library is missing — there is no CPU execution path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdbtk_hip.so")

u64p, u32p, u8p = abi.u64p, abi.u32p, abi.u8p


class DbtkError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"dbtk status {status}: {msg}")
        self.status = status


def _ptr(a, t):
    return a.ctypes.data_as(t) if a is not None else None


def bind_common(L):
    """Prototypes of the host-side entry points (shared with the test emulator)."""
    L.dbtk_last_error.restype = C.c_char_p
    L.dbtk_abi_version.restype = C.c_uint32
    L.dbtk_rpgg_load.restype = C.c_int
    L.dbtk_rpgg_load.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.dbtk_rpgg_load_tr.restype = C.c_int
    L.dbtk_rpgg_load_tr.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.dbtk_rpgg_from_arrays.restype = C.c_int
    L.dbtk_rpgg_from_arrays.argtypes = [C.POINTER(abi.RpggArrays), C.POINTER(C.c_void_p)]
    L.dbtk_rpgg_free.argtypes = [C.c_void_p]
    L.dbtk_rpgg_serialize.restype = C.c_int
    L.dbtk_rpgg_serialize.argtypes = [C.c_char_p]
    for f in ("dbtk_rpgg_nloci", "dbtk_rpgg_ntrkmers", "dbtk_rpgg_nkeys"):
        getattr(L, f).restype = C.c_uint64
        getattr(L, f).argtypes = [C.c_void_p]
    L.dbtk_rpgg_view.restype = C.c_int
    L.dbtk_rpgg_view.argtypes = [C.c_void_p, C.POINTER(abi.RpggArrays)]
    L.dbtk_rpgg_output_order.restype = C.c_int
    L.dbtk_rpgg_output_order.argtypes = [C.c_void_p, u64p]
    L.dbtk_params_default.argtypes = [C.POINTER(abi.Params)]
    L.dbtk_write_outputs.restype = C.c_int
    L.dbtk_write_outputs.argtypes = [C.c_void_p, u64p, u64p, u32p, C.c_char_p, C.c_int]
    L.dbtk_aln_format.restype = C.c_size_t
    L.dbtk_aln_format.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t]


class Rpgg:
    """Immutable RPGG handle (dbtk_rpgg_t)."""

    def __init__(self, lib, handle):
        self._lib, self.h = lib, handle
        L = lib.L
        self.nloci = L.dbtk_rpgg_nloci(handle)
        self.ntrkmers = L.dbtk_rpgg_ntrkmers(handle)
        self.nkeys = L.dbtk_rpgg_nkeys(handle)

    def output_order(self):
        v = abi.RpggArrays()
        self._lib._chk(self._lib.L.dbtk_rpgg_view(self.h, C.byref(v)))
        n = int(sum(v.tr_cnt[i] for i in range(self.nloci)))
        out = np.zeros(n, np.uint64)
        self._lib._chk(self._lib.L.dbtk_rpgg_output_order(self.h, _ptr(out, u64p)))
        return out

    def set_index_cache(self, path, mode=1):
        """The sidecar of the GPU-layout index images: 0 none, 1 load when present, 2 load or write (dbtk_rpgg_set_index_cache)."""
        self._lib._chk(self._lib.L.dbtk_rpgg_set_index_cache(self.h, path.encode() if path else None, mode))

    def view(self):
        v = abi.RpggArrays()
        self._lib._chk(self._lib.L.dbtk_rpgg_view(self.h, C.byref(v)))
        return v

    def write_outputs(self, counts, kmc, nmapread, out_prefix, with_names=False):
        self._lib._chk(self._lib.L.dbtk_write_outputs(self.h, _ptr(counts, u64p), _ptr(kmc, u64p), _ptr(nmapread, u32p),
                                                      out_prefix.encode(), int(with_names)))

    def close(self):
        if self.h:
            self._lib.L.dbtk_rpgg_free(self.h)
            self.h = None


class _HostSide:
    def _chk(self, st):
        if st != abi.OK:
            raise DbtkError(st, self.L.dbtk_last_error().decode())

    def load(self, prefix, k=21, qc_file=None, bait_file=None, flags=0, tr_file=None) -> Rpgg:
        """tr_file: the TR k-mer file when it is not PREF.tr.kmers (`-t N`: PREF.tr.trimN.kmers)."""
        h = C.c_void_p()
        self._chk(self.L.dbtk_rpgg_load_tr(prefix.encode(), tr_file.encode() if tr_file else None, k, qc_file.encode() if qc_file else None,
                                           bait_file.encode() if bait_file else None, flags, C.byref(h)))
        return Rpgg(self, h)

    def serialize(self, prefix):
        """`ktools serialize PREF`: text k-mer files -> PREF.kmers.dbi / .fl.kdb / .tre.kdb."""
        self._chk(self.L.dbtk_rpgg_serialize(prefix.encode()))

    def from_arrays(self, k, keys, vals, vv, fl_cnt, fl_ks, tr_cnt, tr_ks, tre_cnt=None, tre_ks=None, qc=None, gr_cnt=None, gr_ks=None,
                    gr_ms=None) -> Rpgg:
        keep = [np.ascontiguousarray(x, t) if x is not None else None for x, t in
                ((keys, np.uint64), (vals, np.uint32), (vv, np.uint32), (fl_cnt, np.uint64), (fl_ks, np.uint64),
                 (tre_cnt, np.uint64), (tre_ks, np.uint64), (tr_cnt, np.uint64), (tr_ks, np.uint64), (qc, np.uint8),
                 (gr_cnt, np.uint64), (gr_ks, np.uint64), (gr_ms, np.uint8))]
        a = abi.RpggArrays(ksize=k, nloci=len(keep[7]), nkeys=len(keep[0]), keys=_ptr(keep[0], u64p), vals=_ptr(keep[1], u32p),
                           nvv=len(keep[2]), vv=_ptr(keep[2], u32p), fl_cnt=_ptr(keep[3], u64p), fl_ks=_ptr(keep[4], u64p),
                           tre_cnt=_ptr(keep[5], u64p), tre_ks=_ptr(keep[6], u64p), tr_cnt=_ptr(keep[7], u64p),
                           tr_ks=_ptr(keep[8], u64p), qc=_ptr(keep[9], u8p), gr_cnt=_ptr(keep[10], u64p),
                           gr_ks=_ptr(keep[11], u64p), gr_ms=_ptr(keep[12], u8p))
        h = C.c_void_p()
        self._chk(self.L.dbtk_rpgg_from_arrays(C.byref(a), C.byref(h)))
        return Rpgg(self, h)


class Context:
    """Per-GPU context (dbtk_ctx_t)."""

    def __init__(self, lib, rpgg: Rpgg, params: abi.Params, device=0):
        self._lib, self.rpgg, self.params = lib, rpgg, params
        h = C.c_void_p()
        lib._chk(lib.L.dbtk_ctx_create(rpgg.h, C.byref(params), device, C.byref(h)))
        self.h = h

    def align(self, seq, off, qual=None, rec_cap=None):
        """One batch of pairs from host buffers.  Returns the batch's records
        (ctypes array, pair order) — counts accumulate inside the context."""
        L = self._lib.L
        off = np.ascontiguousarray(off, np.uint64)
        seq = np.ascontiguousarray(seq, np.uint8)
        npairs = (len(off) - 1) // 2
        p = self.params
        want = bool(p.trace or p.okam or p.extract)
        cap = npairs if rec_cap is None else rec_cap
        recs = (abi.PairRec * max(cap, 1))() if want and cap else None
        nrec = C.c_uint64(0)
        seqp = _ptr(seq if seq.size else np.zeros(1, np.uint8), u8p)
        self._lib._chk(L.dbtk_align_batch(self.h, seqp, _ptr(off, u64p), _ptr(qual, u8p), npairs, recs, cap if recs else 0,
                                          C.byref(nrec)))
        return recs, int(nrec.value)

    def thread(self, seq, off, loci):
        """dbtk_thread_batch: read r walked through graphDB[loci[r]]; returns a ctypes array of abi.ThreadRec."""
        off = np.ascontiguousarray(off, np.uint64)
        seq = np.ascontiguousarray(seq, np.uint8)
        loci = np.ascontiguousarray(loci, np.uint32)
        n = len(off) - 1
        recs = (abi.ThreadRec * max(n, 1))()
        self._lib._chk(self._lib.L.dbtk_thread_batch(self.h, _ptr(seq if seq.size else np.zeros(1, np.uint8), u8p), _ptr(off, u64p),
                                                     _ptr(loci, u32p), n, recs))
        return recs

    def walk_results(self, cap, with_recs=False):
        """dbtk_ctx_walk_results of the last align(): (WalkRes array, ThreadRec array or None, n)."""
        res = (abi.WalkRes * max(cap, 1))()
        trecs = (abi.ThreadRec * max(2 * cap, 1))() if with_recs else None
        n = C.c_uint64(0)
        self._lib._chk(self._lib.L.dbtk_ctx_walk_results(self.h, res, trecs, cap, C.byref(n)))
        return res, trecs, int(n.value)

    def aln_records(self):
        """dbtk_ctx_aln_records of the last align(): list of (AlnHdr copy, "cigar2\\tannot2\\tcigar1\\tannot1")."""
        L = self._lib.L
        n, st, cap = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
        rc = L.dbtk_ctx_aln_records(self.h, None, 0, C.byref(n), C.byref(st), C.byref(cap))
        if rc not in (abi.OK, abi.ERR_OVERFLOW):
            self._lib._chk(rc)
        if not n.value:
            return []
        buf = (C.c_uint8 * (n.value * st.value))()
        self._lib._chk(L.dbtk_ctx_aln_records(self.h, buf, len(buf), C.byref(n), C.byref(st), C.byref(cap)))
        out = []
        txt = C.create_string_buffer(8192)
        for i in range(n.value):
            rec = C.byref(buf, i * st.value)
            hdr = abi.AlnHdr.from_buffer_copy(buf, i * st.value)
            L.dbtk_aln_format(rec, cap.value, txt, 8192)
            out.append((hdr, txt.value.decode()))
        return out

    def aln_text(self, npairs):
        """dbtk_ctx_aln_text of the last align() (params.aln | abi.ALN_TEXT): list of (pair, dst, "cigar2\\tannot2\\tcigar1\\tannot1")."""
        L = self._lib.L
        L.dbtk_ctx_aln_text.restype = C.c_int
        L.dbtk_ctx_aln_text.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        idx = np.zeros(max(npairs, 1), np.uint32)
        used = C.c_uint64(0)
        rc = L.dbtk_ctx_aln_text(self.h, idx.ctypes.data_as(C.POINTER(C.c_uint32)), npairs, None, 0, C.byref(used))
        if rc not in (abi.OK, abi.ERR_OVERFLOW):
            self._lib._chk(rc)
        arena = np.zeros(max(int(used.value), 4), np.uint8)
        self._lib._chk(L.dbtk_ctx_aln_text(self.h, idx.ctypes.data_as(C.POINTER(C.c_uint32)), npairs, arena.ctypes.data_as(C.c_void_p), len(arena), C.byref(used)))
        out = []
        for p_ in range(npairs):
            o = int(idx[p_])
            if o == 0xFFFFFFFF:
                continue
            dst, ln = int(arena[o:o + 4].view(np.uint32)[0]), int(arena[o + 4:o + 8].view(np.uint32)[0])
            out.append((p_, dst, arena[o + 8:o + 8 + ln].tobytes().decode()))
        return out

    def align_device(self, d_seq_ptr, d_off_ptr, npairs, max_read_len):
        self._lib._chk(self._lib.L.dbtk_align_batch_device(self.h, C.c_void_p(d_seq_ptr), C.c_void_p(d_off_ptr), npairs,
                                                           max_read_len))

    def write_bait_hits(self, out_prefix):
        self._lib._chk(self._lib.L.dbtk_ctx_write_bait_hits(self.h, out_prefix.encode()))

    def write_bubbles(self, out_prefix):
        self._lib._chk(self._lib.L.dbtk_ctx_write_bubbles(self.h, out_prefix.encode()))

    def bubbles(self, th=0):
        """dbtk_ctx_bubbles (params.bubbles = abi.BUBBLES_TABLE): (loci uint32, edges uint64, counts uint32) of the novel edges
        seen at least th times, sorted by (locus, edge)."""
        L = self._lib.L
        n = C.c_uint64(0)
        self._lib._chk(L.dbtk_ctx_bubbles(self.h, int(th), C.byref(n), None, None, None, 0))
        m = int(n.value)
        loci, edges, counts = np.zeros(m, np.uint32), np.zeros(m, np.uint64), np.zeros(m, np.uint32)
        if m:
            self._lib._chk(L.dbtk_ctx_bubbles(self.h, int(th), C.byref(n), _ptr(loci, u32p), _ptr(edges, u64p), _ptr(counts, u32p), m))
        return loci, edges, counts

    def merge_bubbles(self, src):
        self._lib._chk(self._lib.L.dbtk_ctx_merge_bubbles(self.h, src.h))

    def synchronize(self):
        self._lib._chk(self._lib.L.dbtk_ctx_synchronize(self.h))

    def counts(self):
        g = self.rpgg
        counts = np.zeros(g.ntrkmers, np.uint64)
        kmc = np.zeros(g.nloci, np.uint64)
        nmap = np.zeros(g.nloci, np.uint32)
        ctr = np.zeros(abi.C_COUNT, np.uint64)
        self._lib._chk(self._lib.L.dbtk_ctx_counts(self.h, _ptr(counts, u64p), _ptr(kmc, u64p), _ptr(nmap, u32p), _ptr(ctr, u64p)))
        return dict(counts=counts, kmc=kmc, nmapread=nmap, counters=ctr)

    def counters(self):
        ctr = np.zeros(abi.C_COUNT, np.uint64)
        self._lib._chk(self._lib.L.dbtk_ctx_counts(self.h, None, None, None, _ptr(ctr, u64p)))
        return ctr

    def accum_buffer(self):
        base = C.c_void_p()
        n = C.c_uint64()
        self._lib._chk(self._lib.L.dbtk_ctx_accum_buffer(self.h, C.byref(base), C.byref(n)))
        return base.value, int(n.value)

    def reset(self):
        self._lib._chk(self._lib.L.dbtk_ctx_reset(self.h))

    def kernel_times(self):
        """{kernel: (total_ms, launches)} since timers_reset()."""
        names = (C.c_char_p * 8)()
        ms = (C.c_double * 8)()
        cnt = (C.c_uint64 * 8)()
        n = self._lib.L.dbtk_ctx_kernel_times(self.h, names, ms, cnt, 8)
        return {names[i].decode(): (float(ms[i]), int(cnt[i])) for i in range(n)}

    def table_bytes(self):
        """{table: HBM bytes} of the context's RPGG tables ("index_images:from_cache": 1 when the images came from the sidecar)."""
        names = (C.c_char_p * 24)()
        b = (C.c_uint64 * 24)()
        n = self._lib.L.dbtk_ctx_table_bytes(self.h, names, b, 24)
        return {names[i].decode(): int(b[i]) for i in range(n)}

    def path_stats(self):
        """Which kernels took how many pairs since creation / reset (dbtk.h: DBTK_PS_*): a dict."""
        v = (C.c_uint64 * 24)()
        n = self._lib.L.dbtk_ctx_path_stats(self.h, v, 24)
        v = [int(x) for x in v[:n]] + [0] * (24 - n)
        return {"probe_items": v[0:3], "probe_pairs": v[3:6], "probe_rest": v[6], "walk_items": v[7:10], "walk_pairs": v[10:13],
                "walk_rest": v[13], "fused_done": v[14], "fused_redone": v[15], "fused_cls": v[16], "fused_inc": v[17], "walk_locus_ec": v[18], "fused_shared": v[19], "lean_done": v[20], "vote_vv": v[21], "pair_vv": v[22]}

    def timers_reset(self):
        self._lib.L.dbtk_ctx_timers_reset(self.h)

    def timers_enable(self, on=True):
        self._lib.L.dbtk_ctx_timers_enable(self.h, int(on))

    def close(self):
        if self.h:
            self._lib.L.dbtk_ctx_free(self.h)
            self.h = None


class Dbtk(_HostSide):
    """The product: C-ABI of libdbtk_hip.so.  Fails loudly when the HIP
    extension has not been built — nothing falls back to the CPU."""

    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found: build it with `make -C danbing-tk_amd/csrc` "
                                    "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        L = self.L = C.CDLL(path)
        bind_common(L)
        L.dbtk_ctx_create.restype = C.c_int
        L.dbtk_ctx_create.argtypes = [C.c_void_p, C.POINTER(abi.Params), C.c_int, C.POINTER(C.c_void_p)]
        L.dbtk_ctx_free.argtypes = [C.c_void_p]
        L.dbtk_align_batch.restype = C.c_int
        L.dbtk_align_batch.argtypes = [C.c_void_p, u8p, u64p, u8p, C.c_uint64, C.POINTER(abi.PairRec), C.c_uint64, u64p]
        L.dbtk_thread_batch.restype = C.c_int
        L.dbtk_thread_batch.argtypes = [C.c_void_p, u8p, u64p, u32p, C.c_uint64, C.POINTER(abi.ThreadRec)]
        L.dbtk_ctx_walk_results.restype = C.c_int
        L.dbtk_ctx_walk_results.argtypes = [C.c_void_p, C.POINTER(abi.WalkRes), C.POINTER(abi.ThreadRec), C.c_uint64, u64p]
        L.dbtk_ctx_aln_records.restype = C.c_int
        L.dbtk_ctx_aln_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, u64p, u32p, u32p]
        L.dbtk_align_batch_device.restype = C.c_int
        L.dbtk_align_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
        L.dbtk_ctx_synchronize.restype = C.c_int
        L.dbtk_ctx_synchronize.argtypes = [C.c_void_p]
        L.dbtk_ctx_counts.restype = C.c_int
        L.dbtk_ctx_counts.argtypes = [C.c_void_p, u64p, u64p, u32p, u64p]
        L.dbtk_ctx_accum_buffer.restype = C.c_int
        L.dbtk_ctx_accum_buffer.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), u64p]
        L.dbtk_ctx_reset.restype = C.c_int
        L.dbtk_ctx_reset.argtypes = [C.c_void_p]
        L.dbtk_ctx_kernel_times.restype = C.c_int
        L.dbtk_ctx_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_double), u64p, C.c_int]
        L.dbtk_ctx_path_stats.restype = C.c_int
        L.dbtk_ctx_path_stats.argtypes = [C.c_void_p, u64p, C.c_int]
        L.dbtk_ctx_table_bytes.restype = C.c_int
        L.dbtk_ctx_table_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), u64p, C.c_int]
        L.dbtk_ctx_timers_reset.argtypes = [C.c_void_p]
        L.dbtk_ctx_timers_enable.argtypes = [C.c_void_p, C.c_int]
        L.dbtk_ctx_write_bubbles.restype = C.c_int
        L.dbtk_ctx_write_bubbles.argtypes = [C.c_void_p, C.c_char_p]
        L.dbtk_ctx_merge_bubbles.restype = C.c_int
        L.dbtk_ctx_merge_bubbles.argtypes = [C.c_void_p, C.c_void_p]
        L.dbtk_ctx_bubbles.restype = C.c_int
        L.dbtk_ctx_bubbles.argtypes = [C.c_void_p, C.c_uint32, u64p, u32p, u64p, u32p, C.c_uint64]
        L.dbtk_ctx_write_bait_hits.restype = C.c_int
        L.dbtk_ctx_write_bait_hits.argtypes = [C.c_void_p, C.c_char_p]
        L.dbtk_ctx_merge_bait_hits.restype = C.c_int
        L.dbtk_ctx_merge_bait_hits.argtypes = [C.c_void_p, C.c_void_p]
        L.dbtk_allreduce.restype = C.c_int
        L.dbtk_allreduce.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        if L.dbtk_abi_version() != abi.ABI_VERSION:
            raise RuntimeError("libdbtk_hip.so ABI version mismatch")

    def context(self, rpgg: Rpgg, params: abi.Params, device=0) -> Context:
        return Context(self, rpgg, params, device)

    def reserve_host(self, device, chunk_bytes, nslots, lines_bytes=0):
        """dbtk_ingest_reserve_host: pin an ingest's host buffers ahead of its creation (ABI v8)."""
        self.L.dbtk_ingest_reserve_host.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint64]
        self._chk(self.L.dbtk_ingest_reserve_host(int(device), int(chunk_bytes), int(nslots), int(lines_bytes)))

    def allreduce(self, ctxs):
        arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
        self._chk(self.L.dbtk_allreduce(arr, len(ctxs)))


class Ingest:
    """dbtk_ingest_*: raw FASTA / FASTQ bytes in, parsed and paired on the device (include/dbtk.h)."""

    def __init__(self, ctx, fastq, min_read_size, chunk_bytes, nslots=3, with_spans=True):
        self.ctx, self.chunk, self.nslots, self.n = ctx, int(chunk_bytes), int(nslots), 0
        L = self.L = ctx._lib.L
        L.dbtk_ingest_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        L.dbtk_ingest_free.argtypes = [C.c_void_p]
        L.dbtk_ingest_free.restype = None
        L.dbtk_ingest_chunk_buffer.argtypes = [C.c_void_p, C.c_uint32]
        L.dbtk_ingest_chunk_buffer.restype = C.c_void_p
        L.dbtk_ingest_block.argtypes = [C.c_void_p, C.c_uint32]
        L.dbtk_ingest_block.restype = C.c_void_p
        L.dbtk_ingest_submit.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_int]
        L.dbtk_ingest_wait.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(abi.IngestInfo)]
        L.dbtk_ingest_align.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.POINTER(abi.PairRec), C.c_uint64, u64p]
        L.dbtk_ingest_spans.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(abi.IngestSpan), C.c_uint64]
        L.dbtk_ingest_align_merged.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int]
        self.h = C.c_void_p()
        ctx._lib._chk(L.dbtk_ingest_create(ctx.h, int(bool(fastq)), int(min_read_size), self.chunk, self.nslots, int(bool(with_spans)), C.byref(self.h)))

    def submit(self, data: bytes, last: bool):
        slot = self.n % self.nslots
        assert len(data) <= self.chunk
        C.memmove(self.L.dbtk_ingest_chunk_buffer(self.h, slot), data, len(data))
        self.ctx._lib._chk(self.L.dbtk_ingest_submit(self.h, slot, len(data), int(last)))
        self.n += 1
        return slot

    def wait(self, slot):
        info = abi.IngestInfo()
        self.ctx._lib._chk(self.L.dbtk_ingest_wait(self.h, slot, C.byref(info)))
        return info

    def align(self, slot, info, sync=True, ctx=None):
        p = self.ctx.params
        want = sync and bool(p.trace or p.okam or p.extract) and info.nkept
        recs = (abi.PairRec * info.nkept)() if want else None
        nrec = C.c_uint64(0)
        self.ctx._lib._chk(self.L.dbtk_ingest_align(self.h, slot, ctx.h if ctx else None, int(sync), recs, info.nkept if want else 0, C.byref(nrec)))
        return recs, int(nrec.value)

    def align_merged(self, slot, min_pairs, flush=False, ctx=None):
        """dbtk_ingest_align_merged: the block appended to the context's merged batch (slot None: flush only)."""
        self.ctx._lib._chk(self.L.dbtk_ingest_align_merged(self.h, 0xFFFFFFFF if slot is None else slot, ctx.h if ctx else None, int(min_pairs), int(flush)))

    def spans(self, slot, info):
        """[(title, read 2q, read 2q + 1, qual 2q, qual 2q + 1)] of the block's kept pairs, as bytes."""
        sp = (abi.IngestSpan * max(info.nkept, 1))()
        self.ctx._lib._chk(self.L.dbtk_ingest_spans(self.h, slot, sp, info.nkept))
        base = self.L.dbtk_ingest_block(self.h, slot)
        g = lambda o, n: C.string_at(base + o, n)
        return [(g(s.title, s.title_len), g(s.seq[0], s.seq_len[0]), g(s.seq[1], s.seq_len[1]), g(s.qual[0], s.qual_len[0]), g(s.qual[1], s.qual_len[1]))
                for s in sp[:info.nkept]]

    def aln_lines(self, slot, gz=False, ctx=None):
        """(bytes, lines, text bytes): the -a / -ae lines of the block aligned last, as text or as gzip members."""
        L = self.L
        L.dbtk_ingest_aln_lines.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), u64p, u64p, u64p]
        data, nb, nl, tb = C.c_void_p(), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self.ctx._lib._chk(L.dbtk_ingest_aln_lines(self.h, slot, ctx.h if ctx else None, int(gz), C.byref(data), C.byref(nb), C.byref(nl), C.byref(tb)))
        return (C.string_at(data.value, nb.value) if nb.value else b""), int(nl.value), int(tb.value)

    def close(self):
        if self.h:
            self.L.dbtk_ingest_free(self.h)
            self.h = None


# every symbol include/dbtk.h declares (checked by the CPU test-suite)
EXPORTS = [
    "dbtk_rpgg_load", "dbtk_rpgg_load_tr", "dbtk_rpgg_uid", "dbtk_rpgg_from_arrays", "dbtk_rpgg_free", "dbtk_rpgg_nloci", "dbtk_rpgg_ntrkmers", "dbtk_rpgg_nkeys",
    "dbtk_rpgg_view", "dbtk_rpgg_output_order", "dbtk_params_default", "dbtk_device_warmup", "dbtk_ctx_create", "dbtk_ctx_free", "dbtk_align_batch",
    "dbtk_align_batch_device", "dbtk_ctx_synchronize", "dbtk_ctx_counts", "dbtk_ctx_accum_buffer", "dbtk_ctx_reset",
    "dbtk_allreduce", "dbtk_rpgg_set_index_cache", "dbtk_ctx_table_bytes", "dbtk_ctx_path_stats", "dbtk_ctx_kernel_times", "dbtk_ctx_timers_reset", "dbtk_ctx_timers_enable", "dbtk_ctx_aln_text", "dbtk_ctx_write_bubbles", "dbtk_ctx_merge_bubbles", "dbtk_ctx_bubbles", "dbtk_ctx_write_bait_hits", "dbtk_ctx_merge_bait_hits", "dbtk_write_outputs", "dbtk_rpgg_serialize", "dbtk_last_error", "dbtk_abi_version",
    "dbtk_thread_batch", "dbtk_ctx_walk_results", "dbtk_ctx_aln_records", "dbtk_aln_format",
    "dbtk_ingest_reserve_host", "dbtk_ingest_create", "dbtk_ingest_free", "dbtk_ingest_chunk_buffer", "dbtk_ingest_block", "dbtk_ingest_submit", "dbtk_ingest_wait",
    "dbtk_ingest_align", "dbtk_ingest_align_merged", "dbtk_ingest_spans", "dbtk_ingest_aln_lines",
]

# include/dbtk_pred.h (the danbing-tk-pred step)
EXPORTS_PRED = [
    "dbtk_pred_create", "dbtk_pred_free", "dbtk_pred_create_from_file", "dbtk_pred_nk", "dbtk_pred_ntr", "dbtk_pred_load_samples",
    "dbtk_pred_load_device", "dbtk_pred_load_ctx",
    "dbtk_pred_correct", "dbtk_pred_matrix", "dbtk_pred_bias", "dbtk_pred_times",
    "dbtk_pred_create_windowed", "dbtk_pred_create_windowed_from_file", "dbtk_pred_max_rows", "dbtk_pred_window", "dbtk_pred_window_submit",
    "dbtk_pred_window_outputs", "dbtk_pred_window_outputs_pinned", "dbtk_pred_window_stage",
]

# ... and its dosage tables (ABI v10)
EXPORTS_DOSAGE = [
    "dbtk_dosage_create", "dbtk_dosage_create_from_file", "dbtk_dosage_create_from_rpgg", "dbtk_dosage_free", "dbtk_dosage_nk", "dbtk_dosage_ntr",
    "dbtk_dosage_bytes", "dbtk_dosage_load_ctx", "dbtk_dosage_load_device", "dbtk_dosage_load_samples", "dbtk_dosage_finish", "dbtk_dosage_kms",
    "dbtk_dosage_bias", "dbtk_dosage_values", "dbtk_dosage_times",
]


class Pred:
    """include/dbtk_pred.h through ctypes: the cohort matrix in HBM, normalisation and bias correction on the GPU."""

    def __init__(self, lib, ns, nk_cum, nik_cum, iki, ikmc, nk=None, device=0):
        self._lib = lib
        L = lib.L
        L.dbtk_pred_create.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, u32p, u32p, C.c_uint64, u32p, u8p, C.POINTER(C.c_void_p)]
        L.dbtk_pred_free.argtypes = [C.c_void_p]
        L.dbtk_pred_free.restype = None
        L.dbtk_pred_load_samples.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, u64p, C.POINTER(C.c_float)]
        L.dbtk_pred_load_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_float)]
        L.dbtk_pred_load_ctx.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_float]
        L.dbtk_pred_correct.argtypes = [C.c_void_p]
        L.dbtk_pred_matrix.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.dbtk_pred_bias.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.dbtk_pred_times.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self.nk_cum = np.ascontiguousarray(nk_cum, np.uint32)
        self.nik_cum = np.ascontiguousarray(nik_cum, np.uint32)
        self.iki = np.ascontiguousarray(iki, np.uint32)
        self.ikmc = np.ascontiguousarray(ikmc, np.uint8)
        self.ns, self.ntr = int(ns), len(self.nk_cum)
        self.nk = int(nk if nk is not None else (self.nk_cum[-1] if self.ntr else 0))
        self.h = C.c_void_p()
        create = getattr(self, "_create", L.dbtk_pred_create)  # (PredWindowed: dbtk_pred_create_windowed with its max_rows)
        lib._chk(create(device, self.ns, self.nk, self.ntr, _ptr(self.nk_cum, u32p), _ptr(self.nik_cum, u32p), len(self.iki),
                        _ptr(self.iki, u32p), _ptr(self.ikmc, u8p), C.byref(self.h)))

    def load(self, first, counts, depths):
        counts = np.ascontiguousarray(counts, np.uint64)
        depths = np.ascontiguousarray(depths, np.float32)
        self._lib._chk(self._lib.L.dbtk_pred_load_samples(self.h, first, counts.shape[0], _ptr(counts, u64p), depths.ctypes.data_as(C.POINTER(C.c_float))))

    def load_device(self, first, n, d_counts, depths):
        """dbtk_pred_load_device, in its argument order.  d_counts: address of n * nk uint64 counts in device memory (an int, or
        anything with data_ptr())."""
        depths = np.ascontiguousarray(depths, np.float32)
        ptr = d_counts.data_ptr() if hasattr(d_counts, "data_ptr") else int(d_counts)
        self._lib._chk(self._lib.L.dbtk_pred_load_device(self.h, first, n, C.c_void_p(ptr), depths.ctypes.data_as(C.POINTER(C.c_float))))

    def load_ctx(self, sample, ctx, depth):
        """Column `sample` from the accumulated counts of a Context, without a round trip through the host."""
        self._lib._chk(self._lib.L.dbtk_pred_load_ctx(self.h, sample, ctx.h, float(depth)))

    def correct(self):
        self._lib._chk(self._lib.L.dbtk_pred_correct(self.h))

    def matrix(self):
        out = np.empty((self.nk, self.ns), np.float32)
        self._lib._chk(self._lib.L.dbtk_pred_matrix(self.h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def bias(self):
        out = np.empty((self.ntr, self.ns), np.float32)
        self._lib._chk(self._lib.L.dbtk_pred_bias(self.h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def times(self):
        ms = (C.c_float * 3)()
        self._lib._chk(self._lib.L.dbtk_pred_times(self.h, ms))
        return list(ms)

    def close(self):
        if self.h:
            self._lib.L.dbtk_pred_free(self.h)
            self.h = None


class PredWindowed(Pred):
    """A windowed dbtk_pred_t (include/dbtk_pred.h, "Windows"): G holds at most max_rows k-mer columns, whole loci at a time.  load /
    load_device take the current window's counts (n x rows); matrix() returns rows x ns; bias() the whole table."""

    def __init__(self, lib, ns, nk_cum, nik_cum, iki, ikmc, max_rows, nk=None, device=0, ikmer_meta=None):
        L = lib.L
        fp = C.POINTER(C.c_float)
        L.dbtk_pred_create_windowed.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, u32p, u32p, C.c_uint64, u32p, u8p, C.c_uint64, C.POINTER(C.c_void_p)]
        L.dbtk_pred_create_windowed_from_file.argtypes = [C.c_int, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p)]
        L.dbtk_pred_max_rows.argtypes = [C.c_void_p]
        L.dbtk_pred_max_rows.restype = C.c_uint64
        for f in (L.dbtk_pred_nk, L.dbtk_pred_ntr):
            f.argtypes = [C.c_void_p]
            f.restype = C.c_uint64
        L.dbtk_pred_window.argtypes = [C.c_void_p, C.c_uint64, u64p, u64p, u64p]
        L.dbtk_pred_window_submit.argtypes = [C.c_void_p]
        L.dbtk_pred_window_outputs.argtypes = [C.c_void_p, fp, fp]
        L.dbtk_pred_window_outputs_pinned.argtypes = [C.c_void_p, C.POINTER(fp), C.POINTER(fp), u64p]
        L.dbtk_pred_window_stage.argtypes = [C.c_void_p, C.POINTER(u64p), u64p]
        self._create = lambda device, ns, nk, ntr, a, b, nik, c, d, out: (
            L.dbtk_pred_create_windowed_from_file(device, ns, os.fsencode(ikmer_meta), int(max_rows), out) if ikmer_meta is not None
            else L.dbtk_pred_create_windowed(device, ns, nk, ntr, a, b, nik, c, d, int(max_rows), out))
        if ikmer_meta is not None:
            nk_cum = nik_cum = iki = ikmc = []
        super().__init__(lib, ns, nk_cum, nik_cum, iki, ikmc, nk=nk, device=device)
        self.nk, self.ntr = int(L.dbtk_pred_nk(self.h)), int(L.dbtk_pred_ntr(self.h))
        self.max_rows = int(L.dbtk_pred_max_rows(self.h))
        self.first, self.end, self.row0, self.rows = 0, 0, 0, 0
        self.window(0)

    def window(self, first_locus):
        """dbtk_pred_window: (end_locus, first_row, rows) of the window that starts at first_locus; it becomes the current one."""
        e, r0, r = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._lib._chk(self._lib.L.dbtk_pred_window(self.h, int(first_locus), C.byref(e), C.byref(r0), C.byref(r)))
        self.first, self.end, self.row0, self.rows = int(first_locus), int(e.value), int(r0.value), int(r.value)
        return self.end, self.row0, self.rows

    def matrix(self):
        out = np.empty((self.rows, self.ns), np.float32)
        self._lib._chk(self._lib.L.dbtk_pred_matrix(self.h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def submit(self):
        self._lib._chk(self._lib.L.dbtk_pred_window_submit(self.h))
        self._sub_rows = self.rows

    def outputs(self):
        """dbtk_pred_window_outputs: (raw, corrected) of the submitted window — or of the current one —, rows x ns each."""
        rows = self.__dict__.pop("_sub_rows", self.rows)
        raw, cor = np.empty((rows, self.ns), np.float32), np.empty((rows, self.ns), np.float32)
        fp = C.POINTER(C.c_float)
        self._lib._chk(self._lib.L.dbtk_pred_window_outputs(self.h, raw.ctypes.data_as(fp), cor.ctypes.data_as(fp)))
        return raw, cor


class Dosage:
    """The dosage tables of include/dbtk_pred.h through ctypes: per sample and locus the exact k-mer sum (kms), the bias and the
    bias-corrected dosage, without the cohort matrix.  Built from metadata arrays, from an ikmer.meta file (ikmer_meta=) or from a
    loaded Rpgg (rpgg=: no invariant k-mers, every locus uncorrected)."""

    def __init__(self, lib, ns, nk_cum=None, nik_cum=None, iki=None, ikmc=None, nk=None, device=0, ikmer_meta=None, rpgg=None):
        self._lib = lib
        L = lib.L
        fp = C.POINTER(C.c_float)
        L.dbtk_dosage_create.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, u32p, u32p, C.c_uint64, u32p, u8p, C.POINTER(C.c_void_p)]
        L.dbtk_dosage_create_from_file.argtypes = [C.c_int, C.c_uint64, C.c_char_p, C.POINTER(C.c_void_p)]
        L.dbtk_dosage_create_from_rpgg.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]
        L.dbtk_dosage_free.argtypes = [C.c_void_p]
        L.dbtk_dosage_free.restype = None
        for f in (L.dbtk_dosage_nk, L.dbtk_dosage_ntr, L.dbtk_dosage_bytes):
            f.argtypes = [C.c_void_p]
            f.restype = C.c_uint64
        L.dbtk_dosage_load_samples.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, u64p, fp]
        L.dbtk_dosage_load_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, fp]
        L.dbtk_dosage_load_ctx.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_float]
        L.dbtk_dosage_finish.argtypes = [C.c_void_p]
        L.dbtk_dosage_kms.argtypes = [C.c_void_p, u64p]
        L.dbtk_dosage_bias.argtypes = [C.c_void_p, fp]
        L.dbtk_dosage_values.argtypes = [C.c_void_p, fp]
        L.dbtk_dosage_times.argtypes = [C.c_void_p, fp]
        self.ns = int(ns)
        self.h = C.c_void_p()
        if rpgg is not None:
            lib._chk(L.dbtk_dosage_create_from_rpgg(rpgg.h, device, self.ns, C.byref(self.h)))
        elif ikmer_meta is not None:
            lib._chk(L.dbtk_dosage_create_from_file(device, self.ns, os.fsencode(ikmer_meta), C.byref(self.h)))
        else:
            nk_cum = np.ascontiguousarray(nk_cum, np.uint32)
            nik_cum = np.ascontiguousarray(nik_cum, np.uint32)
            iki = np.ascontiguousarray(iki, np.uint32)
            ikmc = np.ascontiguousarray(ikmc, np.uint8)
            nk = int(nk if nk is not None else (nk_cum[-1] if len(nk_cum) else 0))
            lib._chk(L.dbtk_dosage_create(device, self.ns, nk, len(nk_cum), _ptr(nk_cum, u32p), _ptr(nik_cum, u32p), len(iki), _ptr(iki, u32p), _ptr(ikmc, u8p),
                                          C.byref(self.h)))
        self.nk, self.ntr = int(L.dbtk_dosage_nk(self.h)), int(L.dbtk_dosage_ntr(self.h))

    def nbytes(self):
        return int(self._lib.L.dbtk_dosage_bytes(self.h))

    def load(self, first, counts, depths):
        counts = np.ascontiguousarray(counts, np.uint64)
        depths = np.ascontiguousarray(depths, np.float32)
        self._lib._chk(self._lib.L.dbtk_dosage_load_samples(self.h, first, counts.shape[0], _ptr(counts, u64p), depths.ctypes.data_as(C.POINTER(C.c_float))))

    def load_device(self, first, n, d_counts, depths):
        depths = np.ascontiguousarray(depths, np.float32)
        ptr = d_counts.data_ptr() if hasattr(d_counts, "data_ptr") else int(d_counts)
        self._lib._chk(self._lib.L.dbtk_dosage_load_device(self.h, first, n, C.c_void_p(ptr), depths.ctypes.data_as(C.POINTER(C.c_float))))

    def load_ctx(self, sample, ctx, depth):
        self._lib._chk(self._lib.L.dbtk_dosage_load_ctx(self.h, sample, ctx.h, float(depth)))

    def finish(self):
        self._lib._chk(self._lib.L.dbtk_dosage_finish(self.h))

    def kms(self):
        """uint64 [ntr][ns]: entry (locus, sample)."""
        out = np.empty((self.ntr, self.ns), np.uint64)
        self._lib._chk(self._lib.L.dbtk_dosage_kms(self.h, _ptr(out, u64p)))
        return out

    def bias(self):
        out = np.empty((self.ntr, self.ns), np.float32)
        self._lib._chk(self._lib.L.dbtk_dosage_bias(self.h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def values(self):
        out = np.empty((self.ntr, self.ns), np.float32)
        self._lib._chk(self._lib.L.dbtk_dosage_values(self.h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def times(self):
        ms = (C.c_float * 2)()
        self._lib._chk(self._lib.L.dbtk_dosage_times(self.h, ms))
        return list(ms)

    def close(self):
        if self.h:
            self._lib.L.dbtk_dosage_free(self.h)
            self.h = None


EXPORTS_KCP = [
    "dbtk_kcp_api_version", "dbtk_kcp_create", "dbtk_kcp_free", "dbtk_kcp_add", "dbtk_kcp_count", "dbtk_kcp_read", "dbtk_kcp_write", "dbtk_kcp_reset",
    "dbtk_kcp_stats", "dbtk_kcp_times", "dbtk_kcp_add_device", "dbtk_kcp_set_tp_only", "dbtk_kcp_fps_begin", "dbtk_kcp_fps_apply", "dbtk_kcp_fps_count", "dbtk_kcp_fps_read",
    "dbtk_kcp_fps_write", "dbtk_kcp_fps_times", "dbtk_kcp_fps_free", "dbtk_kcp_text_stats",
]


class Kcp:
    """The bait k-mer count profile table of include/dbtk_kcp.h through ctypes: per (assigned locus, canonical k-mer) and class
    (0: true positives, 1: false positives) the exact n, sum, sum of squares, min and max of the k-mer's per-read count."""

    def __init__(self, lib, ksize, nloci, device=0, tp_only=False):
        self._lib = lib
        L = lib.L
        dp = C.POINTER(C.c_double)
        L.dbtk_kcp_api_version.restype = C.c_uint32
        L.dbtk_kcp_api_version.argtypes = []
        L.dbtk_kcp_create.argtypes = [C.c_uint32, C.c_uint64, C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
        L.dbtk_kcp_free.argtypes = [C.c_void_p]
        L.dbtk_kcp_free.restype = None
        L.dbtk_kcp_add.argtypes = [C.c_void_p, u8p, u64p, C.c_uint64, u32p, u32p]
        L.dbtk_kcp_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, u32p]
        L.dbtk_kcp_count.argtypes = [C.c_void_p, C.c_uint32, u64p]
        L.dbtk_kcp_read.argtypes = [C.c_void_p, C.c_uint32, u32p, u64p, u32p, u64p, u64p, u32p, u32p, C.c_uint64]
        L.dbtk_kcp_write.argtypes = [C.c_void_p, C.c_char_p]
        L.dbtk_kcp_reset.argtypes = [C.c_void_p]
        L.dbtk_kcp_stats.argtypes = [C.c_void_p, u64p, u64p, u64p]
        L.dbtk_kcp_times.argtypes = [C.c_void_p, dp, u64p]
        if L.dbtk_kcp_api_version() != abi.KCP_API_VERSION:
            raise RuntimeError("libdbtk_hip.so: dbtk_kcp.h version mismatch")
        self.h = C.c_void_p()
        lib._chk(L.dbtk_kcp_create(int(ksize), int(nloci), int(device), abi.KCP_TP_ONLY if tp_only else 0, C.byref(self.h)))

    def add(self, seq, off, src, dst):
        """seq / off as for Context.align (reads 2p, 2p + 1 = pair p); src / dst: one locus each per pair."""
        seq = np.ascontiguousarray(seq, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        src = np.ascontiguousarray(src, np.uint32)
        dst = np.ascontiguousarray(dst, np.uint32)
        npairs = (len(off) - 1) // 2
        if len(src) != npairs or len(dst) != npairs:
            raise ValueError("one src and one dst per pair")
        self._lib._chk(self._lib.L.dbtk_kcp_add(self.h, _ptr(seq, u8p), _ptr(off, u64p), npairs, _ptr(src, u32p), _ptr(dst, u32p)))

    def add_device(self, d_seq, d_off, npairs, d_src, dst):
        """The same for a batch in device memory (addresses as integers); dst: one locus per pair, on the host."""
        dst = np.ascontiguousarray(dst, np.uint32)
        if len(dst) != npairs:
            raise ValueError("one dst per pair")
        self._lib._chk(self._lib.L.dbtk_kcp_add_device(self.h, d_seq, d_off, int(npairs), d_src, _ptr(dst, u32p)))

    def count(self, cls):
        n = C.c_uint64()
        self._lib._chk(self._lib.L.dbtk_kcp_count(self.h, int(cls), C.byref(n)))
        return int(n.value)

    def read(self, cls):
        """{(locus, kmer): (n, sum, sumsq, min, max)} of the class; the library returns the entries sorted by (locus, k-mer)."""
        cap = self.count(cls)
        loci, n, mn, mx = (np.empty(cap, np.uint32) for _ in range(4))
        kmers, sm, sq = (np.empty(cap, np.uint64) for _ in range(3))
        self._lib._chk(self._lib.L.dbtk_kcp_read(self.h, int(cls), _ptr(loci, u32p), _ptr(kmers, u64p), _ptr(n, u32p), _ptr(sm, u64p), _ptr(sq, u64p), _ptr(mn, u32p),
                                                 _ptr(mx, u32p), cap))
        keys = list(zip(loci.tolist(), kmers.tolist()))
        if keys != sorted(keys):
            raise RuntimeError("dbtk_kcp_read: entries out of order")
        return dict(zip(keys, zip(n.tolist(), sm.tolist(), sq.tolist(), mn.tolist(), mx.tolist())))

    def write(self, prefix):
        self._lib._chk(self._lib.L.dbtk_kcp_write(self.h, os.fsencode(prefix)))

    def reset(self):
        self._lib._chk(self._lib.L.dbtk_kcp_reset(self.h))

    def stats(self):
        """(table bytes, slots, slots taken)"""
        b, s, o = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._lib._chk(self._lib.L.dbtk_kcp_stats(self.h, C.byref(b), C.byref(s), C.byref(o)))
        return int(b.value), int(s.value), int(o.value)

    def times(self):
        """(milliseconds in the add kernel, first occurrences inserted)"""
        ms, n = C.c_double(), C.c_uint64()
        self._lib._chk(self._lib.L.dbtk_kcp_times(self.h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def set_tp_only(self, on):
        """Switches the class filter between batches (what the table holds stays)."""
        self._lib.L.dbtk_kcp_set_tp_only.argtypes = [C.c_void_p, C.c_int]
        self._lib._chk(self._lib.L.dbtk_kcp_set_tp_only(self.h, 1 if on else 0))

    def close(self):
        if self.h:
            self._lib.L.dbtk_kcp_free(self.h)
            self.h = None


class KcpFps:
    """The FP-specific filter of include/dbtk_kcp.h (`baitBuilder v2` on the device): the FP entries of `kcp` as candidates in HBM,
    filtered against TP tables where they lie."""

    def __init__(self, kcp):
        self._lib = kcp._lib
        L = self._lib.L
        u8 = C.POINTER(C.c_uint8)
        L.dbtk_kcp_fps_begin.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.dbtk_kcp_fps_apply.argtypes = [C.c_void_p, C.c_void_p]
        L.dbtk_kcp_fps_count.argtypes = [C.c_void_p, u64p, u64p]
        L.dbtk_kcp_fps_read.argtypes = [C.c_void_p, u32p, u64p, u8, u8, C.c_uint64]
        L.dbtk_kcp_fps_write.argtypes = [C.c_void_p, C.c_char_p]
        L.dbtk_kcp_fps_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), u64p]
        L.dbtk_kcp_fps_free.argtypes = [C.c_void_p]
        L.dbtk_kcp_fps_free.restype = None
        self.h = C.c_void_p()
        self._lib._chk(L.dbtk_kcp_fps_begin(kcp.h, C.byref(self.h)))

    def apply(self, kcp_tp):
        self._lib._chk(self._lib.L.dbtk_kcp_fps_apply(self.h, kcp_tp.h))

    def count(self):
        """(candidates, of them alive)"""
        n, a = C.c_uint64(), C.c_uint64()
        self._lib._chk(self._lib.L.dbtk_kcp_fps_count(self.h, C.byref(n), C.byref(a)))
        return int(n.value), int(a.value)

    def read(self):
        """{(locus, kmer): (mi, ma)} of the living candidates; the library returns them sorted by (locus, k-mer)."""
        cap = self.count()[1]
        loci, kmers = np.empty(cap, np.uint32), np.empty(cap, np.uint64)
        mi, ma = np.empty(cap, np.uint8), np.empty(cap, np.uint8)
        u8 = C.POINTER(C.c_uint8)
        self._lib._chk(self._lib.L.dbtk_kcp_fps_read(self.h, _ptr(loci, u32p), _ptr(kmers, u64p), _ptr(mi, u8), _ptr(ma, u8), cap))
        keys = list(zip(loci.tolist(), kmers.tolist()))
        if keys != sorted(keys):
            raise RuntimeError("dbtk_kcp_fps_read: candidates out of order")
        return dict(zip(keys, zip(mi.tolist(), ma.tolist())))

    def write(self, path):
        self._lib._chk(self._lib.L.dbtk_kcp_fps_write(self.h, os.fsencode(path)))

    def times(self):
        """(milliseconds in k_kcp_fps_apply, living candidates looked up)"""
        ms, n = C.c_double(), C.c_uint64()
        self._lib._chk(self._lib.L.dbtk_kcp_fps_times(self.h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def close(self):
        if self.h:
            self._lib.L.dbtk_kcp_fps_free(self.h)
            self.h = None


def kcp_text_stats(lib, n, sm, sq, device=0):
    """(mean, sd) as float32 arrays: the floats `ktools fps` parses from the profile line of an entry with these moments, computed
    on the device (dbtk_kcp_text_stats)."""
    n = np.ascontiguousarray(n, np.uint32)
    sm = np.ascontiguousarray(sm, np.uint64)
    sq = np.ascontiguousarray(sq, np.uint64)
    if not (len(n) == len(sm) == len(sq)):
        raise ValueError("one n, sum and sumsq per entry")
    mean, sd = np.empty(len(n), np.float32), np.empty(len(n), np.float32)
    fp = C.POINTER(C.c_float)
    lib.L.dbtk_kcp_text_stats.argtypes = [C.c_int, u32p, u64p, u64p, C.c_uint64, fp, fp]
    lib._chk(lib.L.dbtk_kcp_text_stats(int(device), _ptr(n, u32p), _ptr(sm, u64p), _ptr(sq, u64p), len(n), _ptr(mean, fp), _ptr(sd, fp)))
    return mean, sd


EXPORTS_SIM = [
    "dbtk_sim_api_version", "dbtk_sim_open", "dbtk_sim_free", "dbtk_sim_info", "dbtk_sim_contig", "dbtk_sim_describe", "dbtk_sim_labels", "dbtk_sim_attach", "dbtk_sim_batch",
    "dbtk_sim_batch_wait", "dbtk_sim_align", "dbtk_sim_times",
]


class Sim:
    """The simulated read source of include/dbtk_sim.h through ctypes: an assembly tiled into error-free read pairs (what
    `sim_reads -pe -no-err` prints), with the source locus of every pair from a BED.  The constructor is the host pass (no device);
    attach() and what follows need the GPU."""

    def __init__(self, lib, fasta, bed, nloci, flen=500, rlen=150, cv=15, ml=50000):
        self._lib = lib
        L = lib.L
        vpp = C.POINTER(C.c_void_p)
        L.dbtk_sim_api_version.restype = C.c_uint32
        L.dbtk_sim_api_version.argtypes = []
        L.dbtk_sim_open.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, vpp]
        L.dbtk_sim_free.argtypes = [C.c_void_p]
        L.dbtk_sim_free.restype = None
        L.dbtk_sim_info.argtypes = [C.c_void_p, C.POINTER(abi.SimFacts)]
        L.dbtk_sim_contig.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p), vpp, u64p, u64p]
        L.dbtk_sim_describe.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, u32p, u64p, u32p]
        L.dbtk_sim_labels.argtypes = [C.c_void_p, C.c_uint64, u32p, C.c_uint32, u32p]
        L.dbtk_sim_attach.argtypes = [C.c_void_p, C.c_int]
        L.dbtk_sim_batch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, vpp, vpp, vpp, u32p]
        L.dbtk_sim_batch_wait.argtypes = [C.c_void_p]
        L.dbtk_sim_align.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(abi.PairRec), C.c_uint64, u64p]
        L.dbtk_sim_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), u64p, u64p]
        if L.dbtk_sim_api_version() != abi.SIM_API_VERSION:
            raise RuntimeError("libdbtk_hip.so: dbtk_sim.h version mismatch")
        self.h = C.c_void_p()
        lib._chk(L.dbtk_sim_open(os.fsencode(fasta), os.fsencode(bed), int(flen), int(rlen), int(cv), int(ml), int(nloci), C.byref(self.h)))
        self.rlen = int(rlen)
        self.npairs = 0  # of the batch made last

    def info(self) -> abi.SimFacts:
        f = abi.SimFacts()
        self._lib._chk(self._lib.L.dbtk_sim_info(self.h, C.byref(f)))
        return f

    def contig(self, c):
        """(header line, bases as read, number of its first fragment) of kept contig c"""
        hdr, bases, size, first = C.c_char_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        self._lib._chk(self._lib.L.dbtk_sim_contig(self.h, int(c), C.byref(hdr), C.byref(bases), C.byref(size), C.byref(first)))
        return hdr.value.decode(), C.string_at(bases.value, size.value) if size.value else b"", int(first.value)

    def describe(self, first=0, n=None):
        """(contig, beg, src) arrays of fragments first .. first + n - 1 (default: all)"""
        if n is None:
            n = int(self.info().nfrags) - first
        ctg, src = np.empty(n, np.uint32), np.empty(n, np.uint32)
        beg = np.empty(n, np.uint64)
        self._lib._chk(self._lib.L.dbtk_sim_describe(self.h, int(first), int(n), _ptr(ctg, u32p), _ptr(beg, u64p), _ptr(src, u32p)))
        return ctg, beg, src

    def labels(self, frag):
        """every locus overlapping the fragment, ascending (what distinct_sort_num writes into the title)"""
        n = C.c_uint32()
        self._lib._chk(self._lib.L.dbtk_sim_labels(self.h, int(frag), None, 0, C.byref(n)))
        out = np.empty(max(n.value, 1), np.uint32)
        self._lib._chk(self._lib.L.dbtk_sim_labels(self.h, int(frag), _ptr(out, u32p), n.value, C.byref(n)))
        return out[:n.value].tolist()

    def attach(self, device=0):
        self._lib._chk(self._lib.L.dbtk_sim_attach(self.h, int(device)))

    def batch(self, first, npairs):
        """Tiles the pairs into the next buffer set; returns the device addresses (d_seq, d_offsets, d_src) as integers."""
        seq, off, src = C.c_void_p(), C.c_void_p(), C.c_void_p()
        mx = C.c_uint32()
        self._lib._chk(self._lib.L.dbtk_sim_batch(self.h, int(first), int(npairs), C.byref(seq), C.byref(off), C.byref(src), C.byref(mx)))
        self.npairs = int(npairs)
        return seq.value, off.value, src.value

    def wait(self):
        self._lib._chk(self._lib.L.dbtk_sim_batch_wait(self.h))

    def align(self, ctx, sync=True):
        """The batch made last through ctx's hot path; with sync the records (ctypes array, pair order) and their number."""
        p = ctx.params
        want = sync and bool(p.trace or p.okam or p.extract)
        recs = (abi.PairRec * max(self.npairs, 1))() if want else None
        nrec = C.c_uint64(0)
        self._lib._chk(self._lib.L.dbtk_sim_align(self.h, ctx.h, 1 if sync else 0, recs, self.npairs if want else 0, C.byref(nrec)))
        return recs, int(nrec.value)

    def times(self):
        """(milliseconds in k_sim_tile, bytes of reads written, bytes of arena uploaded)"""
        ms, b, u = C.c_double(), C.c_uint64(), C.c_uint64()
        self._lib._chk(self._lib.L.dbtk_sim_times(self.h, C.byref(ms), C.byref(b), C.byref(u)))
        return float(ms.value), int(b.value), int(u.value)

    def close(self):
        if self.h:
            self._lib.L.dbtk_sim_free(self.h)
            self.h = None


EXPORTS_EVAL = [
    "dbtk_eval_api_version", "dbtk_eval_create", "dbtk_eval_free", "dbtk_eval_truth_sim", "dbtk_eval_truth_set", "dbtk_eval_truth", "dbtk_eval_truth_reset",
    "dbtk_eval_score_ctx", "dbtk_eval_score_device", "dbtk_eval_score_host", "dbtk_eval_sums", "dbtk_eval_columns", "dbtk_eval_write", "dbtk_eval_times",
]
EVAL_FIELDS = ("nk", "windows", "n1", "Sx", "Sy", "Sy1", "Sxy", "Sxx", "Syy", "Syy1")  # dbtk_eval_sums_t


def _bind_eval(L):
    vpp = C.POINTER(C.c_void_p)
    L.dbtk_eval_api_version.restype = C.c_uint32
    L.dbtk_eval_api_version.argtypes = []
    L.dbtk_eval_create.argtypes = [C.c_void_p, C.c_int, vpp]
    L.dbtk_eval_free.argtypes = [C.c_void_p]
    L.dbtk_eval_free.restype = None
    L.dbtk_eval_truth_sim.argtypes = [C.c_void_p, C.c_void_p]
    L.dbtk_eval_truth_set.argtypes = [C.c_void_p, u64p, u64p]
    L.dbtk_eval_truth.argtypes = [C.c_void_p, u64p, u64p]
    L.dbtk_eval_truth_reset.argtypes = [C.c_void_p]
    L.dbtk_eval_score_ctx.argtypes = [C.c_void_p, C.c_void_p]
    L.dbtk_eval_score_device.argtypes = [C.c_void_p, C.c_void_p]
    L.dbtk_eval_score_host.argtypes = [C.c_void_p, u64p]
    L.dbtk_eval_sums.argtypes = [C.c_void_p, C.POINTER(abi.EvalSums)]
    L.dbtk_eval_columns.argtypes = [C.POINTER(abi.EvalSums), C.c_uint64, C.POINTER(abi.EvalCols)]
    L.dbtk_eval_write.argtypes = [C.c_void_p, C.c_char_p]
    L.dbtk_eval_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), u64p]
    if L.dbtk_eval_api_version() != abi.EVAL_API_VERSION:
        raise RuntimeError("libdbtk_hip.so: dbtk_eval.h version mismatch")


def eval_columns(lib, sums):
    """dbtk_eval_columns over a list of dicts (or tuples in EVAL_FIELDS order): [(slope, pred, r2, pred_present, r2_present)]; no device."""
    _bind_eval(lib.L)
    n = len(sums)
    arr = (abi.EvalSums * max(n, 1))()
    for i, s in enumerate(sums):
        for j, f in enumerate(EVAL_FIELDS):
            setattr(arr[i], f, int(s[f] if isinstance(s, dict) else s[j]))
    out = (abi.EvalCols * max(n, 1))()
    lib._chk(lib.L.dbtk_eval_columns(arr, n, out))
    return [(c.slope, c.pred, c.r2, c.pred_present, c.r2_present) for c in out[:n]]


class Eval:
    """The genotype score of include/dbtk_eval.h through ctypes: truth counts from attached Sim handles (or from the host), a context's
    or any count vector scored against them per locus: exact sums, and the derived columns of kmers.linreg.py as closed forms."""

    def __init__(self, lib, rpgg, device=0):
        self._lib = lib
        _bind_eval(lib.L)
        self.nk, self.nloci = int(rpgg.ntrkmers), int(rpgg.nloci)
        self.h = C.c_void_p()
        lib._chk(lib.L.dbtk_eval_create(rpgg.h, int(device), C.byref(self.h)))

    def truth_sim(self, sim):
        self._lib._chk(self._lib.L.dbtk_eval_truth_sim(self.h, sim.h))

    def truth_set(self, counts, windows=None):
        c = np.ascontiguousarray(counts, np.uint64)
        w = np.ascontiguousarray(windows, np.uint64) if windows is not None else None
        assert len(c) == self.nk and (w is None or len(w) == self.nloci)
        self._lib._chk(self._lib.L.dbtk_eval_truth_set(self.h, _ptr(c, u64p), _ptr(w, u64p)))

    def truth(self):
        """(counts[nk] in OUT.trkmc.ar order, windows[nloci])"""
        c, w = np.zeros(self.nk, np.uint64), np.zeros(self.nloci, np.uint64)
        self._lib._chk(self._lib.L.dbtk_eval_truth(self.h, _ptr(c, u64p), _ptr(w, u64p)))
        return c, w

    def truth_reset(self):
        self._lib._chk(self._lib.L.dbtk_eval_truth_reset(self.h))

    def score_ctx(self, ctx):
        self._lib._chk(self._lib.L.dbtk_eval_score_ctx(self.h, ctx.h))
        return self.sums()

    def score_device(self, d_counts):
        self._lib._chk(self._lib.L.dbtk_eval_score_device(self.h, C.c_void_p(int(d_counts))))
        return self.sums()

    def score_host(self, counts):
        c = np.ascontiguousarray(counts, np.uint64)
        assert len(c) == self.nk
        self._lib._chk(self._lib.L.dbtk_eval_score_host(self.h, _ptr(c, u64p)))
        return self.sums()

    def sums(self):
        """per locus a dict of the ten integers of dbtk_eval_sums_t"""
        arr = (abi.EvalSums * max(self.nloci, 1))()
        self._lib._chk(self._lib.L.dbtk_eval_sums(self.h, arr))
        return [{f: int(getattr(arr[l], f)) for f in EVAL_FIELDS} for l in range(self.nloci)]

    def write(self, prefix):
        self._lib._chk(self._lib.L.dbtk_eval_write(self.h, os.fsencode(prefix)))

    def times(self):
        """(milliseconds in k_eval_truth, milliseconds in k_eval_sums, class-table look-ups)"""
        ms, n = (C.c_double * 2)(), C.c_uint64()
        self._lib._chk(self._lib.L.dbtk_eval_times(self.h, ms, C.byref(n)))
        return float(ms[0]), float(ms[1]), int(n.value)

    def close(self):
        if self.h:
            self._lib.L.dbtk_eval_free(self.h)
            self.h = None


EXPORTS_ASSOC = [
    "dbtk_assoc_api_version", "dbtk_assoc_create", "dbtk_assoc_free", "dbtk_assoc_set_pairs", "dbtk_assoc_scan_device", "dbtk_assoc_scan_pred",
    "dbtk_assoc_scan_dosage", "dbtk_assoc_best", "dbtk_assoc_hits", "dbtk_assoc_write", "dbtk_assoc_times", "dbtk_assoc_pvalue", "dbtk_assoc_bh",
    "dbtk_assoc_r2_threshold",
]


def _bind_assoc(L):
    dp = C.POINTER(C.c_double)
    L.dbtk_assoc_api_version.restype = C.c_uint32
    L.dbtk_assoc_api_version.argtypes = []
    L.dbtk_assoc_create.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, u64p, dp, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p)]
    L.dbtk_assoc_free.argtypes = [C.c_void_p]
    L.dbtk_assoc_free.restype = None
    L.dbtk_assoc_set_pairs.argtypes = [C.c_void_p, C.c_uint64, u64p, u32p]
    L.dbtk_assoc_scan_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, u32p, C.c_double]
    L.dbtk_assoc_scan_pred.argtypes = [C.c_void_p, C.c_void_p, C.c_double]
    L.dbtk_assoc_scan_dosage.argtypes = [C.c_void_p, C.c_void_p, C.c_double]
    L.dbtk_assoc_best.argtypes = [C.c_void_p, C.POINTER(abi.AssocBest)]
    L.dbtk_assoc_hits.argtypes = [C.c_void_p, C.POINTER(abi.AssocHit), C.c_uint64, u64p]
    L.dbtk_assoc_write.argtypes = [C.c_void_p, C.c_char_p]
    L.dbtk_assoc_times.argtypes = [C.c_void_p, dp]
    L.dbtk_assoc_pvalue.argtypes = [C.c_double, C.c_uint64, dp]
    L.dbtk_assoc_bh.argtypes = [dp, C.c_uint64, dp]
    L.dbtk_assoc_r2_threshold.argtypes = [C.c_double, C.c_uint64, dp]
    if L.dbtk_assoc_api_version() != abi.ASSOC_API_VERSION:
        raise RuntimeError("libdbtk_hip.so: dbtk_assoc.h version mismatch")


def assoc_pvalue(lib, r, n):
    """dbtk_assoc_pvalue: the two-sided Student-t tail of a correlation r over n samples; no device."""
    _bind_assoc(lib.L)
    p = C.c_double()
    lib._chk(lib.L.dbtk_assoc_pvalue(float(r), int(n), C.byref(p)))
    return p.value


def assoc_bh(lib, p):
    """dbtk_assoc_bh: Benjamini-Hochberg q-values of p, clipped at 1; no device."""
    _bind_assoc(lib.L)
    p = np.ascontiguousarray(p, np.float64)
    q = np.zeros(len(p), np.float64)
    lib._chk(lib.L.dbtk_assoc_bh(p.ctypes.data_as(C.POINTER(C.c_double)), len(p), q.ctypes.data_as(C.POINTER(C.c_double))))
    return q


def assoc_r2_threshold(lib, p_threshold, n):
    """dbtk_assoc_r2_threshold: the r^2 the scan kernel compares with for a p-value threshold; no device."""
    _bind_assoc(lib.L)
    r2 = C.c_double()
    lib._chk(lib.L.dbtk_assoc_r2_threshold(float(p_threshold), int(n), C.byref(r2)))
    return r2.value


EXPORTS_ASSOC_COVAR = ["dbtk_assoc_covar_api_version", "dbtk_assoc_covar_basis", "dbtk_assoc_covar_set", "dbtk_assoc_covar_get"]


def _bind_assoc_covar(L):
    dp = C.POINTER(C.c_double)
    L.dbtk_assoc_covar_api_version.restype = C.c_uint32
    L.dbtk_assoc_covar_api_version.argtypes = []
    L.dbtk_assoc_covar_basis.argtypes = [C.c_uint64, C.c_uint64, dp, dp, u64p]
    L.dbtk_assoc_covar_set.argtypes = [C.c_void_p, C.c_uint64, dp, C.POINTER(C.c_char_p)]
    L.dbtk_assoc_covar_get.argtypes = [C.c_void_p, u64p, u64p]
    if L.dbtk_assoc_covar_api_version() != abi.ASSOC_COVAR_API_VERSION:
        raise RuntimeError("libdbtk_hip.so: dbtk_assoc_covar.h version mismatch")


def assoc_covar_basis(lib, covar):
    """dbtk_assoc_covar_basis: covar[q][n] -> the orthonormal basis Q[q][n] of its centred columns; no device.  A DbtkError carries the
    offending column in .bad_column."""
    _bind_assoc_covar(lib.L)
    covar = np.ascontiguousarray(covar, np.float64)
    if covar.ndim == 1:
        covar = covar.reshape(1, -1)
    q, n = covar.shape
    Q = np.zeros((q, n), np.float64)
    bad = C.c_uint64(0)
    try:
        lib._chk(lib.L.dbtk_assoc_covar_basis(n, q, covar.ctypes.data_as(C.POINTER(C.c_double)), Q.ctypes.data_as(C.POINTER(C.c_double)), C.byref(bad)))
    except DbtkError as e:
        e.bad_column = int(bad.value)
        raise
    return Q


EXPORTS_ASSOC_PERM = [
    "dbtk_assoc_perm_api_version", "dbtk_assoc_perm_generate", "dbtk_assoc_perm_set", "dbtk_assoc_perm_seed", "dbtk_assoc_perm_get",
    "dbtk_assoc_perm_scan_device", "dbtk_assoc_perm_scan_pred", "dbtk_assoc_perm_scan_dosage", "dbtk_assoc_perm_results", "dbtk_assoc_perm_stats",
    "dbtk_assoc_perm_write", "dbtk_assoc_perm_times",
]


def _bind_assoc_perm(L):
    dp = C.POINTER(C.c_double)
    L.dbtk_assoc_perm_api_version.restype = C.c_uint32
    L.dbtk_assoc_perm_api_version.argtypes = []
    L.dbtk_assoc_perm_generate.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, u32p]
    L.dbtk_assoc_perm_set.argtypes = [C.c_void_p, C.c_uint64, u32p]
    L.dbtk_assoc_perm_seed.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    L.dbtk_assoc_perm_get.argtypes = [C.c_void_p, u64p, u32p, C.c_uint64]
    L.dbtk_assoc_perm_scan_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, u32p, C.c_double]
    L.dbtk_assoc_perm_scan_pred.argtypes = [C.c_void_p, C.c_void_p, C.c_double]
    L.dbtk_assoc_perm_scan_dosage.argtypes = [C.c_void_p, C.c_void_p, C.c_double]
    L.dbtk_assoc_perm_results.argtypes = [C.c_void_p, C.POINTER(abi.AssocPermResult)]
    L.dbtk_assoc_perm_stats.argtypes = [C.c_void_p, C.c_uint64, dp]
    L.dbtk_assoc_perm_write.argtypes = [C.c_void_p, C.c_char_p]
    L.dbtk_assoc_perm_times.argtypes = [C.c_void_p, dp]
    if L.dbtk_assoc_perm_api_version() != abi.ASSOC_PERM_API_VERSION:
        raise RuntimeError("libdbtk_hip.so: dbtk_assoc_perm.h version mismatch")


def assoc_perm_generate(lib, n, B, seed):
    """dbtk_assoc_perm_generate: perm[B][n] uint32, permutations 1 .. B of the splitmix64 stream of `seed`; no device."""
    _bind_assoc_perm(lib.L)
    perm = np.zeros((int(B), int(n)), np.uint32)
    lib._chk(lib.L.dbtk_assoc_perm_generate(int(n), int(B), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(perm, u32p) if perm.size else None))
    return perm


ASSOC_PERM_FIELDS = ("n_perm", "n_ge", "row", "r2", "p_perm", "q_perm")  # dbtk_assoc_perm_result_t
ASSOC_BEST_FIELDS = ("n_tests", "skipped", "row", "locus", "r", "se", "t", "p", "p_bonf", "q")  # dbtk_assoc_best_t


class Assoc:
    """The association scan of include/dbtk_assoc.h through ctypes: a phenotype table (P x n float64 over the samples sample_of) against
    the rows of a Pred, a Dosage or any float32 [nrows][ns] matrix in device memory; best row per phenotype and the hit list."""

    def __init__(self, lib, ns, sample_of, pheno, names=None, device=0):
        self._lib = lib
        _bind_assoc(lib.L)
        self.sample_of = np.ascontiguousarray(sample_of, np.uint64)
        self.pheno = np.ascontiguousarray(pheno, np.float64)
        if self.pheno.ndim == 1:
            self.pheno = self.pheno.reshape(1, -1)
        self.P, self.n = self.pheno.shape
        assert self.n == len(self.sample_of)
        cnames = None
        if names is not None:
            assert len(names) == self.P
            cnames = (C.c_char_p * self.P)(*[os.fsencode(s) for s in names])
        self.h = C.c_void_p()
        lib._chk(lib.L.dbtk_assoc_create(int(device), int(ns), self.P, self.n, _ptr(self.sample_of, u64p), self.pheno.ctypes.data_as(C.POINTER(C.c_double)),
                                         cnames, C.byref(self.h)))

    def set_pairs(self, off, pheno_idx):
        """CSR over the loci: off[ntr + 1], pheno_idx[off[ntr]]; set_pairs([], []) removes the list."""
        off = np.ascontiguousarray(off, np.uint64)
        idx = np.ascontiguousarray(pheno_idx, np.uint32)
        ntr = max(len(off) - 1, 0)
        self._lib._chk(self._lib.L.dbtk_assoc_set_pairs(self.h, ntr, _ptr(off, u64p) if ntr else None, _ptr(idx, u32p) if len(idx) else None))

    def set_covariates(self, covar, names=None):
        """dbtk_assoc_covar_set: covar[q][n], sample j = sample_of[j]; None or an empty array removes the covariates."""
        _bind_assoc_covar(self._lib.L)
        covar = np.zeros((0, self.n)) if covar is None else np.ascontiguousarray(covar, np.float64)
        if covar.ndim == 1:
            covar = covar.reshape(1, -1) if covar.size else covar.reshape(0, self.n)
        q = covar.shape[0]
        assert q == 0 or covar.shape[1] == self.n
        cnames = None
        if names is not None and q:
            assert len(names) == q
            cnames = (C.c_char_p * q)(*[os.fsencode(s) for s in names])
        self._lib._chk(self._lib.L.dbtk_assoc_covar_set(self.h, q, covar.ctypes.data_as(C.POINTER(C.c_double)) if q else None, cnames))

    def covariates(self):
        """(q, dof): the covariates of the handle and the degrees of freedom n - 2 - q of its tests"""
        _bind_assoc_covar(self._lib.L)
        q, dof = C.c_uint64(), C.c_uint64()
        self._lib._chk(self._lib.L.dbtk_assoc_covar_get(self.h, C.byref(q), C.byref(dof)))
        return int(q.value), int(dof.value)

    def scan_device(self, d_rows, nrows, nk_cum=None, p_threshold=-1.0):
        """d_rows: address of float32 [nrows][ns] in device memory (an int, a ctypes c_void_p, or anything with data_ptr())."""
        ptr = d_rows.data_ptr() if hasattr(d_rows, "data_ptr") else d_rows.value if isinstance(d_rows, C.c_void_p) else int(d_rows)
        nkc = np.ascontiguousarray(nk_cum, np.uint32) if nk_cum is not None else None
        self._lib._chk(self._lib.L.dbtk_assoc_scan_device(self.h, C.c_void_p(ptr), int(nrows), len(nkc) if nkc is not None else 0, _ptr(nkc, u32p), float(p_threshold)))

    def scan_pred(self, pred, p_threshold=-1.0):
        self._lib._chk(self._lib.L.dbtk_assoc_scan_pred(self.h, pred.h, float(p_threshold)))

    def scan_dosage(self, dosage, p_threshold=-1.0):
        self._lib._chk(self._lib.L.dbtk_assoc_scan_dosage(self.h, dosage.h, float(p_threshold)))

    def set_permutations(self, B, seed=None, perms=None):
        """dbtk_assoc_perm_seed (B permutations from `seed`, 1 when neither is given) or dbtk_assoc_perm_set (perms[B][n] over the positions
        0 .. n - 1 of the mask in ascending sample order); B == 0 removes the permutations."""
        _bind_assoc_perm(self._lib.L)
        if perms is not None:
            assert seed is None
            perms = np.ascontiguousarray(perms, np.uint32).reshape(int(B), self.n) if int(B) else np.zeros((0, self.n), np.uint32)
            self._lib._chk(self._lib.L.dbtk_assoc_perm_set(self.h, int(B), _ptr(perms, u32p) if perms.size else None))
        elif not int(B):
            self._lib._chk(self._lib.L.dbtk_assoc_perm_set(self.h, 0, None))
        else:
            self._lib._chk(self._lib.L.dbtk_assoc_perm_seed(self.h, int(B), (1 if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF))

    def permutations(self):
        """perm[B][n] as the handle holds them"""
        _bind_assoc_perm(self._lib.L)
        B = C.c_uint64()
        self._lib._chk(self._lib.L.dbtk_assoc_perm_get(self.h, C.byref(B), None, 0))
        perm = np.zeros((B.value, self.n), np.uint32)
        if perm.size:
            self._lib._chk(self._lib.L.dbtk_assoc_perm_get(self.h, C.byref(B), _ptr(perm, u32p), B.value))
        return perm

    def perm_scan_device(self, d_rows, nrows, nk_cum=None, p_threshold=-1.0):
        """scan_device, then the permutation pass over the same rows"""
        _bind_assoc_perm(self._lib.L)
        ptr = d_rows.data_ptr() if hasattr(d_rows, "data_ptr") else d_rows.value if isinstance(d_rows, C.c_void_p) else int(d_rows)
        nkc = np.ascontiguousarray(nk_cum, np.uint32) if nk_cum is not None else None
        self._lib._chk(self._lib.L.dbtk_assoc_perm_scan_device(self.h, C.c_void_p(ptr), int(nrows), len(nkc) if nkc is not None else 0, _ptr(nkc, u32p), float(p_threshold)))

    def perm_scan_pred(self, pred, p_threshold=-1.0):
        _bind_assoc_perm(self._lib.L)
        self._lib._chk(self._lib.L.dbtk_assoc_perm_scan_pred(self.h, pred.h, float(p_threshold)))

    def perm_scan_dosage(self, dosage, p_threshold=-1.0):
        _bind_assoc_perm(self._lib.L)
        self._lib._chk(self._lib.L.dbtk_assoc_perm_scan_dosage(self.h, dosage.h, float(p_threshold)))

    def perm_results(self):
        """per phenotype a dict of dbtk_assoc_perm_result_t"""
        _bind_assoc_perm(self._lib.L)
        arr = (abi.AssocPermResult * self.P)()
        self._lib._chk(self._lib.L.dbtk_assoc_perm_results(self.h, arr))
        return [{f: getattr(arr[p], f) for f in ASSOC_PERM_FIELDS} for p in range(self.P)]

    def perm_stats(self, p):
        """T[B + 1] of phenotype p: the observed maximum of r^2 and those of the B permutations"""
        _bind_assoc_perm(self._lib.L)
        B = C.c_uint64()
        self._lib._chk(self._lib.L.dbtk_assoc_perm_get(self.h, C.byref(B), None, 0))
        T = np.zeros(B.value + 1, np.float64)
        self._lib._chk(self._lib.L.dbtk_assoc_perm_stats(self.h, int(p), T.ctypes.data_as(C.POINTER(C.c_double))))
        return T

    def perm_write(self, prefix):
        _bind_assoc_perm(self._lib.L)
        self._lib._chk(self._lib.L.dbtk_assoc_perm_write(self.h, os.fsencode(prefix)))

    def perm_times(self):
        """(milliseconds in k_assoc_perm, milliseconds in the host fold) of the last permutation scan"""
        _bind_assoc_perm(self._lib.L)
        ms = (C.c_double * 2)()
        self._lib._chk(self._lib.L.dbtk_assoc_perm_times(self.h, ms))
        return float(ms[0]), float(ms[1])

    def best(self):
        """per phenotype a dict of dbtk_assoc_best_t"""
        arr = (abi.AssocBest * self.P)()
        self._lib._chk(self._lib.L.dbtk_assoc_best(self.h, arr))
        return [{f: getattr(arr[p], f) for f in ASSOC_BEST_FIELDS} for p in range(self.P)]

    def hits(self):
        """[(pheno, locus, row, r, t, p)] sorted by (pheno, row)"""
        n = C.c_uint64()
        self._lib._chk(self._lib.L.dbtk_assoc_hits(self.h, None, 0, C.byref(n)))
        arr = (abi.AssocHit * max(n.value, 1))()
        self._lib._chk(self._lib.L.dbtk_assoc_hits(self.h, arr, n.value, C.byref(n)))
        return [(h.pheno, h.locus, h.row, h.r, h.t, h.p) for h in arr[:n.value]]

    def write(self, prefix):
        self._lib._chk(self._lib.L.dbtk_assoc_write(self.h, os.fsencode(prefix)))

    def times(self):
        """(milliseconds in k_assoc_scan, milliseconds in the host fold) of the last scan"""
        ms = (C.c_double * 2)()
        self._lib._chk(self._lib.L.dbtk_assoc_times(self.h, ms))
        return float(ms[0]), float(ms[1])

    def close(self):
        if self.h:
            self._lib.L.dbtk_assoc_free(self.h)
            self.h = None


class Synth:
    """Seeded release-scale workload generator (csrc/dbtk_synth.cpp): a flat
    RPGG + 150 bp read pairs, for bench.py and the scale tests."""

    def __init__(self, nloci=80000, k=21, flank=700, seed=20250808, nthreads=0, path=os.path.join(_HERE, "libdbtk_synth.so")):
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found: run `make -C danbing-tk_amd/csrc`")
        L = self.L = C.CDLL(path)
        L.dbtk_synth_create.restype = C.c_void_p
        L.dbtk_synth_create.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32]
        L.dbtk_synth_free.argtypes = [C.c_void_p]
        L.dbtk_synth_arrays.argtypes = [C.c_void_p, C.POINTER(abi.RpggArrays)]
        L.dbtk_synth_nbases.restype = C.c_uint64
        L.dbtk_synth_nbases.argtypes = [C.c_void_p]
        L.dbtk_synth_reads.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_double, C.c_uint64, u8p, C.c_uint32]
        L.dbtk_synth_reads_loci.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_double, C.c_uint64, u8p, C.c_uint32]
        L.dbtk_synth_graph.argtypes = [C.c_void_p, C.c_uint32]
        L.dbtk_synth_write_files.restype = C.c_int
        L.dbtk_synth_write_files.argtypes = [C.c_void_p, C.c_char_p]
        L.dbtk_synth_write_fasta.restype = C.c_int
        L.dbtk_synth_write_fasta.argtypes = [u8p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_char_p]
        self.h = L.dbtk_synth_create(nloci, k, flank, seed, nthreads)
        self.k, self.nloci = k, nloci

    def arrays(self) -> abi.RpggArrays:
        a = abi.RpggArrays()
        self.L.dbtk_synth_arrays(self.h, C.byref(a))
        return a

    def graph(self, nthreads=0):
        """Build graphDB (both strands of every haplotype); arrays() then carries gr_cnt / gr_ks / gr_ms."""
        self.L.dbtk_synth_graph(self.h, nthreads)

    def write_files(self, prefix):
        """The RPGG as the HEAD files the reference binary loads (PREF.tr.kmers, .kmers.dbi, .fl.kdb, .tre.kdb)."""
        if self.L.dbtk_synth_write_files(self.h, prefix.encode()):
            raise IOError(f"could not write {prefix}.*")

    def write_fasta(self, seq, npairs, fn, rlen=150, first_pair=0):
        if self.L.dbtk_synth_write_fasta(_ptr(seq, u8p), npairs, rlen, first_pair, fn.encode()):
            raise IOError(f"could not write {fn}")

    def reads(self, npairs, rlen=150, hit_frac=1.0, seed=1, first_pair=0, out=None, nthreads=0):
        """(seq bytes, offsets) — read r is seq[r*rlen:(r+1)*rlen]."""
        if out is None:
            out = np.empty(npairs * 2 * rlen, np.uint8)
        self.L.dbtk_synth_reads(self.h, npairs, first_pair, rlen, float(hit_frac), seed, _ptr(out, u8p), nthreads)
        off = np.arange(2 * npairs + 1, dtype=np.uint64) * np.uint64(rlen)
        return out, off

    def reads_loci(self, npairs, loci, rlen=150, odd_frac=0.1, seed=1, first_pair=0, nthreads=0):
        """(seq bytes, offsets): pair p drawn from loci[p % len(loci)] — a DENSE slice (many pairs per locus: the regime of the
        locus-resident kernels); odd_frac of the pairs chimeric (mate 2 from any locus) or foreign (both from any locus)."""
        loci = np.ascontiguousarray(loci, np.uint32)
        out = np.empty(npairs * 2 * rlen, np.uint8)
        self.L.dbtk_synth_reads_loci(self.h, npairs, first_pair, rlen, _ptr(loci, C.POINTER(C.c_uint32)), len(loci), float(odd_frac), seed, _ptr(out, u8p), nthreads)
        off = np.arange(2 * npairs + 1, dtype=np.uint64) * np.uint64(rlen)
        return out, off

    def sequences(self):
        """(seq, hap_beg, locus_hap0) as numpy views of the generator's memory: haplotype j of locus l (flank + TR + flank) is
        seq[hap_beg[locus_hap0[l] + j]:hap_beg[locus_hap0[l] + j + 1]]"""
        self.L.dbtk_synth_sequences.argtypes = [C.c_void_p, C.POINTER(u8p), C.POINTER(u64p), C.POINTER(u32p)]
        self.L.dbtk_synth_sequences.restype = None
        seq, hb, lh = u8p(), u64p(), u32p()
        self.L.dbtk_synth_sequences(self.h, C.byref(seq), C.byref(hb), C.byref(lh))
        lh = np.ctypeslib.as_array(lh, (self.nloci + 1,))
        hb = np.ctypeslib.as_array(hb, (int(lh[-1]) + 1,))
        return np.ctypeslib.as_array(seq, (int(self.L.dbtk_synth_nbases(self.h)),)), hb, lh

    def close(self):
        if self.h:
            self.L.dbtk_synth_free(self.h)
            self.h = None
