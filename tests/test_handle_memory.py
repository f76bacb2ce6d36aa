"""What the side modules' handles (pred, windowed pred, dosage, kcp, kcp_fps, sim, eval, assoc) hold of the HBM goes back when they are
closed: free memory by hipMemGetInfo over create / use / close cycles, as test_contexts_share_device_tables does it for the contexts.

Per handle type: two cycles first (what the HIP runtime keeps for itself at a kernel's first launches, code objects and scratch, is not
the library's to give back), then the footprint F = the drop of free memory from before the handle's creation to after its use, then six
more cycles.  Six cycles must cost less than F / 2: a buffer of a twelfth of the footprint leaked once per cycle would cost that much,
and any of the main buffers six times its size.  The HBM of these machines is shared, hence a margin and no equality to the byte; the
shapes are chosen so that F is tens of MB (asserted) and the allocator's granularity cannot decide the outcome."""
import ctypes as C

import numpy as np
import pytest

import bind

pkg, abi = bind.pkg, bind.abi
pytestmark = pytest.mark.gpu

MIN_FOOTPRINT = 20e6
CYCLES = 6


@pytest.fixture(scope="module")
def lib():
    return pkg.Dbtk()


class Hip:
    def __init__(self):
        h = self.h = C.CDLL("libamdhip64.so")
        h.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipFree.argtypes = [C.c_void_p]

    def free_bytes(self):
        f, t = C.c_size_t(0), C.c_size_t(0)
        assert self.h.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value

    def put(self, arr):
        d = C.c_void_p()
        assert self.h.hipMalloc(C.byref(d), max(arr.nbytes, 8)) == 0
        assert self.h.hipMemcpy(d, arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1) == 0
        return d

    def free(self, d):
        self.h.hipFree(d)


@pytest.fixture(scope="module")
def hip():
    return Hip()


def check_cycles(hip, name, cycle):
    """cycle(probe): creates the handle, uses it, calls probe() while everything it allocates is alive, and closes it."""
    for _ in range(2):
        cycle(lambda: None)
    seen = []
    m0 = hip.free_bytes()
    cycle(lambda: seen.append(hip.free_bytes()))
    foot = m0 - seen[0]
    m1 = hip.free_bytes()
    for _ in range(CYCLES):
        cycle(lambda: None)
    m2 = hip.free_bytes()
    print(f"{name}: footprint {foot} bytes; free HBM {m0} before it, {m1} after its close, {m2} after {CYCLES} more cycles (cost {m1 - m2})")
    assert foot >= MIN_FOOTPRINT, (name, foot)
    assert m1 - m2 < foot / 2, (name, foot, m0, m1, m2)
    return foot


# ---- the genotype matrix, its windowed form and the dosage tables: no invariant k-mers (every locus uncorrected), loci of equal size
def meta_of(nk, ntr):
    return np.arange(1, ntr + 1, dtype=np.uint32) * np.uint32(nk // ntr), np.zeros(ntr, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint8)


def test_pred_gives_back_its_matrix_and_both_stagings(lib, hip):
    """G 32 MB, the staging of load_samples 16 MB (2 samples), the depths of load_device (2 samples: the tile kernel's buffer)."""
    ns, nk, ntr = 8, 1 << 20, 64
    rng = np.random.default_rng(1)
    counts = rng.integers(0, 50, (2, nk)).astype(np.uint64)
    d_counts = hip.put(counts)

    def cycle(probe):
        P = pkg.Pred(lib, ns, *meta_of(nk, ntr), nk=nk)
        P.load(0, counts, [30.0, 31.0])
        P.load_device(2, 2, d_counts.value, [32.0, 33.0])
        probe()
        P.close()
    try:
        check_cycles(hip, "pred", cycle)
    finally:
        hip.free(d_counts)


def test_windowed_pred_gives_back_its_window_buffers(lib, hip):
    """max_rows = nk / 4: 24 * max_rows * ns bytes of window buffers beside G's 4; one window loaded, run through the fused pass, read."""
    ns, nk, ntr = 8, 1 << 20, 64
    rows = nk // 4
    rng = np.random.default_rng(2)
    counts = rng.integers(0, 50, (2, rows)).astype(np.uint64)

    def cycle(probe):
        W = pkg.PredWindowed(lib, ns, *meta_of(nk, ntr), rows, nk=nk)
        assert W.rows == rows
        W.load(0, counts, [30.0, 31.0])
        W.submit()
        W.outputs()
        probe()
        W.close()
    check_cycles(hip, "windowed pred", cycle)


def test_dosage_gives_back_its_tables_and_its_staging(lib, hip):
    """The staging of load_samples is 16 samples' counts whatever is loaded: 32 MB at nk = 2^18; one sample goes through it."""
    ns, nk, ntr = 8, 1 << 18, 64
    counts = np.random.default_rng(3).integers(0, 50, (1, nk)).astype(np.uint64)

    def cycle(probe):
        D = pkg.Dosage(lib, ns, *meta_of(nk, ntr), nk=nk)
        D.load(0, counts, [30.0])
        D.finish()
        probe()
        D.close()
    check_cycles(hip, "dosage", cycle)


# ---- the bait profile table and the candidates of the FP filter
def random_pairs(npairs, seed, rlen=150):
    seq = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, npairs * 2 * rlen)]
    return seq, np.arange(2 * npairs + 1, dtype=np.uint64) * np.uint64(rlen)


def test_kcp_gives_back_its_table_after_a_growth(lib, hip, monkeypatch):
    """DBTK_KCP_SLOTS = 64 and 2500 pairs of 260 k-mer positions: one growth, to 2^21 slots of 40 bytes, the old table freed behind it."""
    monkeypatch.setenv("DBTK_KCP_SLOTS", "64")
    npairs, nloci = 2500, 50
    seq, off = random_pairs(npairs, 4)
    dst = np.arange(npairs, dtype=np.uint32) % nloci
    src = np.where(np.arange(npairs) % 3 == 0, (dst + 1) % nloci, dst).astype(np.uint32)

    def cycle(probe):
        K = pkg.Kcp(lib, 21, nloci)
        assert K.stats()[1] == 64
        K.add(seq, off, src, dst)
        assert K.stats()[1] == 1 << 21 and K.count(0) + K.count(1) == K.stats()[2] > 600000
        probe()
        K.close()
    check_cycles(hip, "kcp", cycle)


def test_kcp_fps_gives_back_its_candidates(lib, hip):
    """6000 false-positive pairs: 1.5 million candidates of 20 bytes, begun from one table and applied to another (both outlive the cycles)."""
    npairs, nloci = 6000, 50
    seq, off = random_pairs(npairs, 5)
    dst = np.arange(npairs, dtype=np.uint32) % nloci
    K = pkg.Kcp(lib, 21, nloci)
    K.add(seq, off, (dst + 1) % nloci, dst)
    T = pkg.Kcp(lib, 21, nloci, tp_only=True)
    T.add(seq[:300 * 200], off[:401], dst[:200], dst[:200])

    def cycle(probe):
        F = pkg.KcpFps(K)
        n, alive = F.count()
        assert n == alive == K.count(1) > 1500000
        F.apply(T)
        assert 0 < F.count()[1] < n
        probe()
        F.close()
    try:
        check_cycles(hip, "kcp_fps", cycle)
    finally:
        T.close()
        K.close()


# ---- the simulated read source
def test_sim_gives_back_its_arena_and_both_batch_sets(lib, hip, tmp_path):
    """Two contigs of 8 MB in one group: a 16 MB arena; one batch of 40000 pairs: 12 MB of reads, their offsets and sources."""
    rng = np.random.default_rng(6)
    fa, bed = str(tmp_path / "asm.fa"), str(tmp_path / "asm.bed")
    with open(fa, "wb") as f:
        for c in range(2):
            f.write(b">ctg%d\n" % c + np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 8 << 20)].tobytes() + b"\n")
    with open(bed, "w") as f:
        f.write("ctg0\t1000\t3000\t0\nctg1\t5000\t9000\t1\n")

    def cycle(probe):
        S = pkg.Sim(lib, fa, bed, 2, ml=1)
        assert S.info().ncontigs == 2
        S.attach(0)
        assert S.info().ngroups == 1
        S.batch(400000, 40000)   # (across the two contigs: the first has 419406 fragments)
        S.wait()
        probe()
        S.close()
    check_cycles(hip, "sim", cycle)


# ---- the genotype score
def test_eval_gives_back_its_tables(lib, hip):
    """A Synth of 400 loci: the class table (the evaluator's own share of it: no context exists), the table of the k-mers in both sets,
    truth, windows, sums and the count vector of score_host."""
    syn = pkg.Synth(nloci=400)
    arrs = syn.arrays()
    h = C.c_void_p()
    lib._chk(lib.L.dbtk_rpgg_from_arrays(C.byref(arrs), C.byref(h)))
    g = pkg.Rpgg(lib, h)
    rng = np.random.default_rng(7)
    truth = rng.integers(0, 40, g.ntrkmers).astype(np.uint64)
    counts = rng.integers(0, 40, g.ntrkmers).astype(np.uint64)

    def cycle(probe):
        E = pkg.Eval(lib, g)
        E.truth_set(truth)
        sums = E.score_host(counts)
        assert len(sums) == g.nloci and sum(s["Sx"] for s in sums) == int(truth.sum())
        probe()
        E.close()
    try:
        check_cycles(hip, "eval", cycle)
    finally:
        g.close()
        syn.close()


# ---- the association scan
class AssocCase:
    """n = 70 of 70 samples (more than a wave's 64), 3 loci of 10000 rows, 4000 phenotypes listed at every locus, 2 covariates: the hit
    buffer's 16 MB, 11.5 MB of candidates (120 work items x 4000), the phenotypes and their projections."""
    ns, ntr, rows, P, q = 70, 3, 10000, 4000, 2

    def __init__(self, hip):
        rng = np.random.default_rng(8)
        self.G = rng.normal(size=(self.ntr * self.rows, self.ns)).astype(np.float32)
        self.pheno = rng.normal(size=(self.P, self.ns))
        self.covar = rng.normal(size=(self.q, self.ns))
        self.nk_cum = np.arange(1, self.ntr + 1, dtype=np.uint32) * np.uint32(self.rows)
        self.off = np.arange(self.ntr + 1, dtype=np.uint64) * np.uint64(self.P)
        self.idx = np.tile(np.arange(self.P, dtype=np.uint32), self.ntr)
        self.d_G = hip.put(self.G)

    def create(self, lib):
        A = pkg.Assoc(lib, self.ns, np.arange(self.ns), self.pheno)
        A.set_pairs(self.off, self.idx)
        A.set_covariates(self.covar)
        return A

    def scan(self, A):
        A.scan_device(self.d_G, len(self.G), self.nk_cum, p_threshold=1e-5)   # (some thousand hits of 120 million tests)
        return A.best(), A.hits()


@pytest.fixture(scope="module")
def assoc_case(hip):
    c = AssocCase(hip)
    yield c
    hip.free(c.d_G)


def test_assoc_gives_back_its_tables(lib, hip, assoc_case):
    def cycle(probe):
        A = assoc_case.create(lib)
        best, hits = assoc_case.scan(A)
        assert all(b["n_tests"] == assoc_case.ntr * assoc_case.rows for b in best) and 0 < len(hits) < 1 << 20
        probe()
        A.close()
    check_cycles(hip, "assoc", cycle)


def test_assoc_refused_covariates_cost_nothing_and_change_nothing(lib, hip, assoc_case):
    """dbtk_assoc_covar_set with a covariate equal to a phenotype: DBTK_ERR_ARG once the new tables are in HBM and the kernel has run on
    them.  Six refusals cost less than half a footprint, and the handle scans on with the covariates it had: the result it gave before."""
    A = assoc_case.create(lib)
    bad = np.vstack([assoc_case.covar[0], assoc_case.pheno[5]])

    def refuse():
        with pytest.raises(pkg.DbtkError) as e:
            A.set_covariates(bad)
        assert e.value.status == abi.ERR_ARG and "is explained by the covariates" in str(e.value)
    try:
        m0 = hip.free_bytes()
        B = assoc_case.create(lib)
        assoc_case.scan(B)
        foot = m0 - hip.free_bytes()
        B.close()
        before = assoc_case.scan(A)
        for _ in range(2):
            refuse()
        m1 = hip.free_bytes()
        for _ in range(CYCLES):
            refuse()
        m2 = hip.free_bytes()
        print(f"assoc, refused covariates: footprint {foot} bytes; {CYCLES} refusals cost {m1 - m2}")
        assert foot >= MIN_FOOTPRINT and m1 - m2 < foot / 2, (foot, m1, m2)
        assert A.covariates() == (assoc_case.q, assoc_case.ns - 2 - assoc_case.q)
        assert assoc_case.scan(A) == before
    finally:
        A.close()
