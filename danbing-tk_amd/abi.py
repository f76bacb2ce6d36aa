"""ctypes mirror of include/dbtk.h (struct layouts and constants only)."""
import ctypes as C

MAX_READ_LEN = 256
NAN64 = 0xFFFFFFFFFFFFFFFF
NAN32 = 0xFFFFFFFF
ABI_VERSION = 11
KCP_API_VERSION = 1  # include/dbtk_kcp.h: DBTK_KCP_API_VERSION (a version of its own beside ABI_VERSION)
KCP_TP_ONLY = 1      # dbtk_kcp_create flags
KCP_FPS_MI_NONE, KCP_FPS_MA_NONE = 255, 0  # dbtk_kcp_fps_read: (mi, ma) of a living candidate that no TP table held
SIM_API_VERSION = 1  # include/dbtk_sim.h: DBTK_SIM_API_VERSION
EVAL_API_VERSION = 1  # include/dbtk_eval.h: DBTK_EVAL_API_VERSION
ASSOC_API_VERSION = 1  # include/dbtk_assoc.h: DBTK_ASSOC_API_VERSION
ASSOC_ALL_PAIRS_MAX = 64  # phenotypes up to which a table may be scanned without a pair list
ASSOC_NONE = 0xFFFFFFFF  # row / locus of a phenotype without tests
ASSOC_COVAR_API_VERSION = 1  # include/dbtk_assoc_covar.h: DBTK_ASSOC_COVAR_API_VERSION
ASSOC_COVAR_MAX = 128  # covariates of a table at most
ASSOC_COVAR_COLLINEAR = 1e-6  # the residual share at or below which a covariate, a row or a phenotype counts as explained
ASSOC_PERM_API_VERSION = 1  # include/dbtk_assoc_perm.h: DBTK_ASSOC_PERM_API_VERSION
ASSOC_PERM_MAX = 1000000  # permutations of a handle at most
BUBBLES_LOG, BUBBLES_TABLE = 1, 2  # params.bubbles: event log replayed on the host (reference order) | counts in a device table
ALN_TEXT = 4  # params.aln | ALN_TEXT: alignment records in text form (dbtk_ctx_aln_text)
THREAD_CAP = 384
ING_DIRTY, ING_LINES, ING_CARRY, ING_TAIL = 1, 2, 4, 8  # dbtk_ingest_info.flags
THREADING_HEAD, THREADING_V13 = 1, 2

(OK, ERR_ARG, ERR_IO, ERR_FORMAT, ERR_NO_DEVICE, ERR_HIP, ERR_READ_TOO_LONG, ERR_NOMEM, ERR_UNSUPPORTED,
 ERR_OVERFLOW) = range(10)

(STAGE_SHORT, STAGE_SUBFILTER, STAGE_KFILTER, STAGE_LOCUS, STAGE_QC, STAGE_BAIT, STAGE_ASGN, STAGE_COUNTED,
 STAGE_EXTRACT, STAGE_THREADING) = range(10)

(C_NREADS, C_SUBFILTERED, C_KMERFILTERED, C_BAITFILTERED, C_QUALFILTERED, C_LOCUSFILTERED, C_QCFILTERED,
 C_THREADING, C_FEASIBLE, C_ASGN, C_NSHORT, C_NHASH0, C_NHASH1, C_ALGO_PROBES, C_ALGO_VV, C_ALGO_CLS, C_ALGO_INC,
 C_SURVIVORS, C_BASES) = range(19)
C_COUNT = 24

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
u16p = C.POINTER(C.c_uint16)
u8p = C.POINTER(C.c_uint8)


class Params(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in
                ("ksize", "n_filter", "nm_filter", "cthreshold", "nm_tr", "max_nt", "qth", "okam", "qc", "bait",
                 "bubbles", "extract", "trace", "threading", "simmode", "thread_cth", "maxncorrection", "correction", "aln", "trackbait", "diag")]


class RpggArrays(C.Structure):
    _fields_ = [
        ("ksize", C.c_uint32), ("nloci", C.c_uint64),
        ("nkeys", C.c_uint64), ("keys", u64p), ("vals", u32p),
        ("nvv", C.c_uint64), ("vv", u32p),
        ("fl_cnt", u64p), ("fl_ks", u64p),
        ("tre_cnt", u64p), ("tre_ks", u64p),
        ("tr_cnt", u64p), ("tr_ks", u64p),
        ("qc", u8p),
        ("bt_cnt", u64p), ("bt_ks", u64p), ("bt_vs", u16p),
        ("gr_cnt", u64p), ("gr_ks", u64p), ("gr_ms", u8p),
    ]


class MateRec(C.Structure):
    _fields_ = [(n, C.c_int16) for n in ("si", "ei", "si_", "ei_", "nt", "bs", "ti")] + \
               [(n, C.c_uint8) for n in ("kf", "hf", "bf", "qf", "af", "rm")] + \
               [("nk", C.c_uint16), ("as2", C.c_uint8 * (MAX_READ_LEN // 4))]

    def annot(self):
        """The `as` vector (0 '*', 1 '.', 2 '=')."""
        return [(self.as2[i >> 2] >> (2 * (i & 3))) & 3 for i in range(self.nk)]


class PairRec(C.Structure):
    _fields_ = [("pair", C.c_uint32), ("stage", C.c_uint32), ("dst", C.c_uint32), ("dst0", C.c_uint32),
                ("nm1", C.c_int32), ("nm2", C.c_int32), ("r1", MateRec), ("r2", MateRec)]


class ThreadRec(C.Structure):
    """What isThreadFeasible leaves behind for one read (include/dbtk.h: dbtk_thread_rec_t)."""
    _fields_ = [("ret", C.c_int32), ("ni", C.c_int32), ("nkm", C.c_uint32), ("nes", C.c_uint32), ("ntr", C.c_uint32),
                ("flags", C.c_uint32),
                ("es_t", C.c_uint8 * THREAD_CAP), ("es_r", C.c_uint8 * THREAD_CAP), ("es_g", C.c_uint8 * THREAD_CAP),
                ("tr", C.c_uint8 * THREAD_CAP), ("kmers", C.c_uint64 * THREAD_CAP)]


class WalkRes(C.Structure):
    _fields_ = [("pair", C.c_uint32), ("dst", C.c_uint32), ("ret1", C.c_int8), ("ret2", C.c_int8), ("pad", C.c_uint8 * 2)]


class AlnHdr(C.Structure):
    _fields_ = [("pair", C.c_uint32), ("dst", C.c_uint32), ("ret1", C.c_int8), ("ret2", C.c_int8), ("pad", C.c_uint8 * 2),
                ("nes1", C.c_uint16), ("ntr1", C.c_uint16), ("nes2", C.c_uint16), ("ntr2", C.c_uint16), ("pad2", C.c_uint32)]


LOAD_INDEX_ONLY, LOAD_GRAPH = 1, 2


def default_params(**kw) -> Params:
    """Defaults of the reference: src/aQueryFasta_thread.cpp:26-34, 2336-2339."""
    p = Params(ksize=21, n_filter=4, nm_filter=1, cthreshold=10, nm_tr=40, max_nt=2, qth=20, okam=1, thread_cth=100,
               maxncorrection=4)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class IngestInfo(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("npairs", C.c_uint32), ("nkept", C.c_uint32), ("max_read_len", C.c_uint32),
                ("first_byte", C.c_uint64), ("cut_byte", C.c_uint64), ("seq_bytes", C.c_uint64)]


class IngestSpan(C.Structure):
    _fields_ = [("title", C.c_uint32), ("title_len", C.c_uint32), ("seq", C.c_uint32 * 2), ("seq_len", C.c_uint32 * 2),
                ("qual", C.c_uint32 * 2), ("qual_len", C.c_uint32 * 2)]


class SimFacts(C.Structure):
    """include/dbtk_sim.h: dbtk_sim_facts_t"""
    _fields_ = [(n, C.c_uint64) for n in ("ncontigs", "nskipped", "nfrags", "arena_bytes", "nbreaks")] + \
               [(n, C.c_uint32) for n in ("flen", "rlen", "shft", "ngroups")]


class EvalSums(C.Structure):
    """include/dbtk_eval.h: dbtk_eval_sums_t"""
    _fields_ = [(n, C.c_uint64) for n in ("nk", "windows", "n1", "Sx", "Sy", "Sy1", "Sxy", "Sxx", "Syy", "Syy1")]


class EvalCols(C.Structure):
    """include/dbtk_eval.h: dbtk_eval_cols_t"""
    _fields_ = [(n, C.c_double) for n in ("slope", "pred", "r2", "pred_present", "r2_present")]


class AssocBest(C.Structure):
    """include/dbtk_assoc.h: dbtk_assoc_best_t"""
    _fields_ = [("n_tests", C.c_uint64), ("skipped", C.c_uint64), ("row", C.c_uint32), ("locus", C.c_uint32)] + \
               [(n, C.c_double) for n in ("r", "se", "t", "p", "p_bonf", "q")]


class AssocPermResult(C.Structure):
    """include/dbtk_assoc_perm.h: dbtk_assoc_perm_result_t"""
    _fields_ = [("n_perm", C.c_uint64), ("n_ge", C.c_uint64), ("row", C.c_uint32), ("pad", C.c_uint32)] + \
               [(n, C.c_double) for n in ("r2", "p_perm", "q_perm")]


class AssocHit(C.Structure):
    """include/dbtk_assoc.h: dbtk_assoc_hit_t"""
    _fields_ = [(n, C.c_uint32) for n in ("pheno", "locus", "row", "pad")] + [(n, C.c_double) for n in ("r", "t", "p")]
