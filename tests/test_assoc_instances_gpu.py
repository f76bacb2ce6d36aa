"""The association kernels (csrc/dbtk_assoc.hip: k_assoc_scan; csrc/dbtk_assoc_perm_dev.h: k_assoc_perm) where tests/test_assoc_gpu.py,
tests/test_assoc_covar_gpu.py and tests/test_assoc_perm_gpu.py do not reach, read against the launchers' dispatch:

A. tables over EVERY sample (n == ns, the instances IDENT == true that read G[base + j] without the index list), with sample_of a
   permutation of 0 .. ns - 1: the host reorders the phenotypes, the covariates and nothing else;
B. 2 AS_GRID + 5 work items, so that a workgroup takes a second and a third item: the LDS and the registers of the item before are used
   again, and many workgroups fold into one T[p][b];
C. sizes that fill a unit exactly: loci of AS_ROWS, 2 AS_ROWS, AS_ITEM_ROWS and 2 AS_ITEM_ROWS rows, AS_CHUNK and 2 AS_CHUNK phenotypes,
   q and B + 1 whole numbers of chunks, and DBTK_ASSOC_ALL_PAIRS_MAX phenotypes without a pair list.

The reference is the numpy float64 model (tests/assoc_model.py, tests/assoc_covar_model.py, tests/assoc_perm_model.py) fed the same
float32 matrix and, with covariates, the handle's own basis; the tolerance is the derived one of tests/test_assoc_gpu.py and
tests/test_assoc_covar_gpu.py, unchanged; n_tests, skipped, rows, loci, the hit set and n_ge compare exactly, behind the margins that
test_the_inputs_keep_their_margins_without_a_gpu asserts of every case on the model alone.  dispatch() mirrors the two launchers, and
test_the_cases_reach_every_instance holds the case lists to it.  Every GPU test prints the largest |device - model| / bound it met."""
import functools
import math
import os
import re

import numpy as np
import pytest

import assoc_covar_model as cm
import assoc_model
import assoc_perm_model as pm
import bind
from test_assoc_covar_gpu import ROW_NEAR, ROW_SPAN, share_margins
from test_assoc_gpu import LOCUS_PHENOS, LOCUS_ROWS, NPHENO, P_THRESHOLD, TRAILING, assert_margins, compare, mask_of, put
from test_assoc_perm_gpu import bound_of, check, with_noise
from test_pred_device import _Hip

abi, pkg = bind.abi, bind.pkg


def kernel_constants():
    src = open(os.path.join(bind.ROOT, "danbing-tk_amd", "csrc", "dbtk_assoc.hip")).read()
    env = {}
    for name, expr in re.findall(r"constexpr\s+uint(?:32|64)_t\s+(AS_\w+)\s*=\s*([^;]+);", src):
        env[name] = eval(re.sub(r"(\d+)ull\b", r"\1", expr), {}, dict(env))
    return env


K = kernel_constants()
AS_GRID, AS_ITEM_ROWS, AS_ROWS, AS_CHUNK, AS_SEG = K["AS_GRID"], K["AS_ITEM_ROWS"], K["AS_ROWS"], K["AS_CHUNK"], K["AS_SEG"]

# ---- A: n == ns
A_PLAIN = [3, 65, 512, 513, 1100]
A_COVAR = [(12, 9), (512, 17), (513, 128)]                 # (n, q)
A_PERM = [(65, 9), (513, 9)]                               # (n, B)
A_PERM_COVAR = [(65, 8, 7), (513, 9, 3)]                   # (n, q, B)
A_SEED = {}                                                # (kind, n): seeds other than 1, chosen on the model alone
# ---- B: 2 AS_GRID + 5 non-empty items behind a pair list
B_ITEMS = 2 * AS_GRID + 5
B_SHAPES = [(65, 70), (65, 65), (513, 513)]                # (n, ns)
B_Q, B_B, B_P, B_TRAILING = 9, 9, 16, 3
# covariates plus permutations: (65, 70) is the one the work asked for; the two all-sample shapes stand beside it because without them no
# k_assoc_perm<true, true, .> would make a second trip (test_the_cases_reach_every_instance)
B_PERM_COVAR_SHAPES = [(65, 70), (65, 65), (513, 513)]
B_SEED = {}
# ---- C: whole units
C_ROWS = [AS_ROWS, 2 * AS_ROWS, AS_ITEM_ROWS, 2 * AS_ITEM_ROWS, AS_ROWS - 1]
C_PHENOS = [AS_CHUNK, 2 * AS_CHUNK, AS_CHUNK, 1, AS_CHUNK - 1]
C_P, C_TRAILING = 2 * AS_CHUNK, 2
C_SHAPES = [(64, 70), (64, 64), (513, 520)]
C_QS = [AS_CHUNK, 2 * AS_CHUNK]
C_BS = [AS_CHUNK - 1, 2 * AS_CHUNK - 1]
# (n, ns, q, B): no case above is masked, not resident, with covariates AND permuted: k_assoc_perm<false, true, false>
C_PERM_COVAR = [(513, 520, AS_CHUNK, AS_CHUNK - 1)]
C_SEED = {}
# DBTK_ASSOC_ALL_PAIRS_MAX phenotypes against 40 rows without a pair list
WIDE_SHAPES = [(65, 70), (65, 65)]
WIDE_ROWS, WIDE_B = 40, AS_CHUNK - 1
WIDE_SEED = {}


def dispatch(n, ns, q, perm):
    """(kernel, IDENT, COVAR, RES) as assoc_scan_impl and assoc_perm_pass_impl choose it (RES is None for the scan)"""
    ident, covar = n == ns, q > 0
    return ("k_assoc_perm", ident, covar, n <= AS_SEG) if perm else ("k_assoc_scan", ident, covar, None)


ALL_INSTANCES = {("k_assoc_scan", i, c, None) for i in (False, True) for c in (False, True)} | \
                {("k_assoc_perm", i, c, r) for i in (False, True) for c in (False, True) for r in (False, True)}


def reached(n, ns, q, B):
    """a permutation scan makes the ordinary scan first"""
    return {dispatch(n, ns, q, False)} | ({dispatch(n, ns, q, True)} if B else set())


def case_lists():
    """group -> [(n, ns, q, B)] of every GPU case of this module"""
    a = [(n, n, 0, 0) for n in A_PLAIN] + [(n, n, q, 0) for n, q in A_COVAR] + [(n, n, 0, B) for n, B in A_PERM] + [(n, n, q, B) for n, q, B in A_PERM_COVAR]
    b = [(n, ns, q, B) for n, ns in B_SHAPES for q, B in ((0, 0), (B_Q, 0), (0, B_B))] + [(n, ns, B_Q, B_B) for n, ns in B_PERM_COVAR_SHAPES]
    c = [(n, ns, q, 0) for n, ns in C_SHAPES for q in [0] + C_QS] + [(n, ns, 0, B) for n, ns in C_SHAPES for B in C_BS] + list(C_PERM_COVAR)
    c += [(n, ns, 0, B) for n, ns in WIDE_SHAPES for B in (0, WIDE_B)]
    return dict(A=a, B=b, C=c)


@pytest.fixture(scope="module")
def dbtk():
    return lib()


@pytest.fixture(scope="module")
def hip():
    return _Hip()


@functools.lru_cache(maxsize=None)
def lib():
    return pkg.Dbtk()


# ---------------------------------------------------------------------------------------------------------------------- the builders
def all_samples(n, seed):
    """test_assoc_gpu.hand_made over every sample: ns = n, sample_of a seeded permutation of 0 .. ns - 1 that is not the identity.  No
    column is masked, so nothing is written "outside the mask"; the special rows stand in the locus of 40 rows as there."""
    rng = np.random.default_rng(seed)
    ns = n
    nk_cum = np.cumsum(LOCUS_ROWS).astype(np.uint32)
    nrows = int(nk_cum[-1]) + TRAILING
    sample_of = rng.permutation(ns).astype(np.int64)
    while (sample_of == np.arange(ns)).all():
        sample_of = rng.permutation(ns).astype(np.int64)
    G = rng.gamma(2.0, 1.5, (nrows, ns)).astype(np.float32)
    pheno = rng.normal(0, 1, (NPHENO, n))
    for p in range(NPHENO):
        pheno[p] += 0.8 * G[(37 * p + 11) % nrows, sample_of] / 1.5
    off, idx = [0], []
    for k in LOCUS_PHENOS:
        idx += sorted(int(v) for v in rng.choice(NPHENO, k, replace=False))
        off.append(len(idx))
    r40 = int(nk_cum[4])
    G[r40 + 2, :] = 2.5                                                    # constant
    G[r40 + 3, sample_of[n // 2]] = np.inf                                  # one inf
    G[r40 + 4, :] = 1.0
    G[r40 + 4, sample_of[1]] = 3.0                                          # a single sample differs
    p_one = idx[off[5]]
    pheno[p_one] = rng.gamma(2.0, 1.5, n).astype(np.float32).astype(np.float64)
    G[r40 + 7, sample_of] = pheno[p_one].astype(np.float32)                 # a row that equals a phenotype: r = 1, p = 0
    p_tie = idx[off[5] + 1]
    G[r40 + 20] = G[r40 + 9]                                                # duplicate rows: a tie in r^2, the lower row wins
    pheno[p_tie] = rng.normal(0, 1, n) + (2.0 if n > 3 else 0.5) * G[r40 + 9, sample_of]
    return dict(G=G, ns=ns, sample_of=sample_of, pheno=pheno, nk_cum=nk_cum, pairs=(off, idx), r40=r40, p_one=p_one, p_tie=p_tie)


def add_covariates(c, q, seed, special=True):
    """what test_assoc_covar_gpu.covar_case adds to its matrix: small integer covariates (all but the first two with noise), phenotypes
    that lean on them (not the one that a row equals), and with `special` a row that is an exact combination of the integer covariates
    and that row plus noise"""
    rng = np.random.default_rng(77 + seed)
    n, so = len(c["sample_of"]), c["sample_of"]
    covar = rng.integers(0, 4, (q, n)).astype(np.float64)
    covar[2:] += rng.normal(0, 0.25, (max(q - 2, 0), n))
    for p in range(c["pheno"].shape[0]):
        if p != c.get("p_one"):
            c["pheno"][p] += covar.T @ rng.normal(0, 0.5, q)
    if special:
        r40 = c["r40"]
        combo = 1.0 + 2.0 * covar[0] + (3.0 * covar[1] if q > 1 else 0.0)
        c["G"][r40 + ROW_SPAN, so] = combo.astype(np.float32)
        assert (c["G"][r40 + ROW_SPAN, so].astype(np.float64) == combo).all()
        c["G"][r40 + ROW_NEAR, so] = (combo + rng.normal(0, 1.4, n)).astype(np.float32)
    c.update(covar=covar, q=q)
    return c


def samples_of(n, ns, rng):
    return mask_of(n, ns, rng) if n < ns else rng.permutation(ns).astype(np.int64)


def decorate(G, sample_of, ns):
    """outside the mask anything may stand (as in test_assoc_gpu.hand_made)"""
    masked = np.setdiff1d(np.arange(ns), sample_of)
    if len(masked):
        G[::3, masked[0]] = np.nan
        G[1::5, masked[-1]] = np.inf


def items_of(rows, nph):
    """the work items as assoc_scan_impl cuts them behind a pair list: (locus, first row of the item within the locus)"""
    return [(l, r) for l in range(len(rows)) if nph[l] for r in range(0, int(rows[l]), AS_ITEM_ROWS)]


@functools.lru_cache(maxsize=None)
def many_items(n, ns, seed):
    """B_ITEMS non-empty work items: loci of 1 row, one of AS_ROWS + 1 and one of AS_ITEM_ROWS + 1 rows (two items), three of no row
    and three without a phenotype (neither makes an item); 1, 2, AS_CHUNK, AS_CHUNK + 1 phenotypes per locus in turn; B_P phenotypes,
    each leaning on one of its rows: of the first, the second and the third trip in turn."""
    rng = np.random.default_rng(seed)
    nloci = B_ITEMS - 1 + 6
    rows = np.ones(nloci, np.int64)
    empty, bare = (7, AS_GRID + 2, nloci - 6), (11, AS_GRID + 3, nloci - 1)
    rows[list(empty)] = 0
    rows[1000], rows[3000] = AS_ROWS + 1, AS_ITEM_ROWS + 1
    cyc, k, nph = (1, 2, AS_CHUNK, AS_CHUNK + 1), 0, np.zeros(nloci, np.int64)
    for l in range(nloci):
        if l not in bare:
            nph[l] = cyc[k % 4]
            k += 1
    nph[1000], nph[3000] = AS_CHUNK + 1, AS_CHUNK
    items = items_of(rows, nph)
    assert len(items) == B_ITEMS and (B_ITEMS - 1) // AS_GRID == 2                # a third trip for the first blocks
    nk_cum = np.cumsum(rows).astype(np.uint32)
    nrows = int(nk_cum[-1]) + B_TRAILING
    sample_of = samples_of(n, ns, rng)
    G = rng.gamma(2.0, 1.5, (nrows, ns)).astype(np.float32)
    decorate(G, sample_of, ns)
    off, idx = [0], []
    for l in range(nloci):
        idx += sorted(int(v) for v in rng.choice(B_P, int(nph[l]), replace=False))
        off.append(len(idx))
    pheno = rng.normal(0, 1, (B_P, n))
    first = np.concatenate([[0], nk_cum[:-1]]).astype(np.int64)
    lean = []
    for p in range(B_P):
        for t in (p % 3, 1):             # (the five items of the third trip do not carry every phenotype)
            mine = [first[l] + r for l, r in items[t * AS_GRID:(t + 1) * AS_GRID] if p in idx[off[l]:off[l + 1]]]
            if mine:
                break
        row = int(mine[(7 * p + 1) % len(mine)])
        lean.append(row)
        pheno[p] += 0.8 * G[row, sample_of] / 1.5
    trip = np.full(nrows, -1, np.int64)                                            # the trip that scans a row
    for i, (l, r) in enumerate(items):
        trip[first[l] + r:first[l] + min(r + AS_ITEM_ROWS, rows[l])] = i // AS_GRID
    return dict(G=G, ns=ns, sample_of=sample_of, pheno=pheno, nk_cum=nk_cum, pairs=(off, idx), nitems=len(items), lean=lean, trip=trip)


@functools.lru_cache(maxsize=None)
def whole_units(n, ns, seed):
    """loci of exactly AS_ROWS, 2 AS_ROWS, AS_ITEM_ROWS and 2 AS_ITEM_ROWS rows with exactly AS_CHUNK, 2 AS_CHUNK, AS_CHUNK and 1
    phenotypes, and beside them one of AS_ROWS - 1 rows with AS_CHUNK - 1"""
    rng = np.random.default_rng(seed)
    nk_cum = np.cumsum(C_ROWS).astype(np.uint32)
    nrows = int(nk_cum[-1]) + C_TRAILING
    sample_of = samples_of(n, ns, rng)
    G = rng.gamma(2.0, 1.5, (nrows, ns)).astype(np.float32)
    decorate(G, sample_of, ns)
    off, idx = [0], []
    for k in C_PHENOS:
        idx += sorted(int(v) for v in rng.choice(C_P, k, replace=False))
        off.append(len(idx))
    pheno = rng.normal(0, 1, (C_P, n))
    for p in range(C_P):                 # (a row of the locus that carries every phenotype: the last rows of its two passes among them)
        pheno[p] += 0.8 * G[C_ROWS[0] + (4 * p + 3) % C_ROWS[1], sample_of] / 1.5
    return dict(G=G, ns=ns, sample_of=sample_of, pheno=pheno, nk_cum=nk_cum, pairs=(off, idx))


@functools.lru_cache(maxsize=None)
def wide(n, ns, seed):
    """DBTK_ASSOC_ALL_PAIRS_MAX phenotypes and WIDE_ROWS rows, one of them constant: scanned without a pair list, 8 full chunks"""
    rng = np.random.default_rng(seed)
    P = abi.ASSOC_ALL_PAIRS_MAX
    sample_of = samples_of(n, ns, rng)
    G = rng.gamma(2.0, 1.5, (WIDE_ROWS, ns)).astype(np.float32)
    decorate(G, sample_of, ns)
    G[17, :] = 0.5
    pheno = rng.normal(0, 1, (P, n))
    for p in range(P):
        row = (11 * p + 5) % WIDE_ROWS
        pheno[p] += 0.8 * G[row + (row == 17), sample_of] / 1.5          # (not on the constant row)
    return dict(G=G, ns=ns, sample_of=sample_of, pheno=pheno, nk_cum=np.array([WIDE_ROWS], np.uint32), pairs=None)


def with_pheno(c, **more):
    """a case of its own phenotypes over a shared matrix"""
    d = dict(c)
    d["pheno"] = c["pheno"].copy()
    d.update(more)
    return d


# ------------------------------------------------------------------------------------------------------------------------ the models
def basis_of(c):
    order = np.argsort(c["sample_of"], kind="stable")
    return pkg.assoc_covar_basis(lib(), c["covar"][:, order])


def scan_model(c, pairs):
    """the model's scan with hits, its tolerance, and every margin that the exact comparisons need"""
    n, q = len(c["sample_of"]), c.get("q", 0)
    if q:
        m = cm.scan(c["G"], c["sample_of"], c["pheno"], c["covar"], Q=c["Q"], nk_cum=c["nk_cum"], pairs=pairs, p_threshold=P_THRESHOLD)
        tol = cm.tolerance(c["G"], c["sample_of"], c["pheno"], q, m["share_x"], m["share_y"])
        assert tol[m["tested"]].max() < 1e-7
        share_margins(m)
    else:
        m = assoc_model.scan(c["G"], c["sample_of"], c["pheno"], nk_cum=c["nk_cum"], pairs=pairs, p_threshold=P_THRESHOLD)
        tol = assoc_model.tolerance(c["G"], c["sample_of"], c["pheno"])
        assert tol.max() < 1e-9
    assert_margins(m, c["G"], c["sample_of"], tol, pkg.assoc_r2_threshold(lib(), P_THRESHOLD, n - q))
    assert len(m["hits"]) < 2 ** 20
    return m, tol


def perm_model(c, pairs, m, tol, B, seed):
    """the maxima of the model over the scan's tested pairs, their bound, and the margins of n_ge"""
    n = len(c["sample_of"])
    perms = pm.generate(n, B, seed)
    T, n_tests, y = pm.maxima(c["G"], c["sample_of"], c["pheno"], perms, nk_cum=c["nk_cum"], pairs=pairs, covar=c.get("covar"), Q=c.get("Q"))
    use = m["paired"] & m["tested"][:, None]
    assert (use.sum(axis=0) == n_tests).all()
    bound = bound_of(tol, use)
    assert bound.max() < 1e-6
    pm.assert_margins(T, y, perms, bound)
    return dict(perms=perms, T=T, n_tests=n_tests, bound=bound)


def modelled(c, B, seed, pair_modes):
    """c with its basis and, per pair mode (True: the pair list, False: every phenotype against every row), the models"""
    if c.get("q"):
        c["Q"] = basis_of(c)
    c["model"] = {}
    for on in pair_modes:
        pairs = c["pairs"] if on else None
        m, tol = scan_model(c, pairs)
        c["model"][on] = dict(m=m, tol=tol, perm=perm_model(c, pairs, m, tol, B, seed) if B else None)
    return c


@functools.lru_cache(maxsize=None)
def case_a(n, q, B):
    kind = ("perm_" if B else "") + ("covar" if q else "plain")
    seed = A_SEED.get((kind, n), 1)
    c = all_samples(n, 5000 + 1000 * seed + n + (300 if B else 0))
    if q:
        add_covariates(c, q, seed)
    if B:
        with_noise(c, seed, n)
    c = modelled(c, B, seed, (False, True))
    r40, m = c["r40"], c["model"][False]["m"]
    assert m["tested"][r40 + 4] and not m["tested"][r40 + 2] and not m["tested"][r40 + 3]
    if q:
        assert not m["tested"][r40 + ROW_SPAN] and m["tested"][r40 + ROW_NEAR] and 1e-3 < m["share_x"][r40 + ROW_NEAR] < 0.5
    for on in (False, True):
        w = c["model"][on]["m"]["best"]
        assert w[c["p_one"]]["row"] == r40 + 7 and w[c["p_one"]]["r"] == 1.0
        assert w[c["p_tie"]]["row"] != r40 + 20 and (w[c["p_tie"]]["row"] == r40 + 9 or n == 3 or q)
    c["seed"] = seed
    return c


@functools.lru_cache(maxsize=None)
def case_b(n, ns, q, B):
    seed = B_SEED.get((n, ns), 1)
    c = with_pheno(many_items(n, ns, 7000 + 10 * seed + n + ns))
    if q:
        add_covariates(c, q, seed, special=False)
    c = modelled(c, B, seed, (True,))
    mm = c["model"][True]
    best_trips = {int(c["trip"][b["row"]]) for b in mm["m"]["best"]}
    assert best_trips == {0, 1, 2}, best_trips                 # a scan that stops after a trip loses best rows; so do the maxima
    assert {int(c["trip"][h[2]]) for h in mm["m"]["hits"]} == {0, 1, 2} and len(mm["m"]["hits"]) > 300
    assert all(b["n_tests"] > 1000 for b in mm["m"]["best"])
    c["seed"] = seed
    return c


@functools.lru_cache(maxsize=None)
def case_c(n, ns, q, B):
    seed = C_SEED.get((n, ns), 1)
    c = with_pheno(whole_units(n, ns, 8000 + 10 * seed + n + ns))
    if q:
        add_covariates(c, q, seed, special=False)
    c = modelled(c, B, seed, (True,))
    c["seed"] = seed
    return c


@functools.lru_cache(maxsize=None)
def case_wide(n, ns, B):
    seed = WIDE_SEED.get((n, ns), 1)
    c = modelled(with_pheno(wide(n, ns, 9000 + 10 * seed + n + ns)), B, seed, (False,))
    c["seed"] = seed
    return c


# -------------------------------------------------------------------------------------------------------- the tests without a device
def test_the_cases_reach_every_instance():
    """The union of this module's cases runs all 12 instances of the two kernels, and every one of the 6 with IDENT == true both on the
    hand-made matrix of A and behind the many work items of B."""
    lists = case_lists()
    union = set().union(*(reached(*c) for cases in lists.values() for c in cases))
    assert union == ALL_INSTANCES and len(ALL_INSTANCES) == 12, ALL_INSTANCES - union
    ident = {i for i in ALL_INSTANCES if i[1]}
    assert len(ident) == 6
    for group in ("A", "B"):
        got = set().union(*(reached(*c) for c in lists[group]))
        assert ident <= got, (group, ident - got)
    assert all(n == ns for n, ns, _, _ in lists["A"])
    # the launchers are read as they stand: the flag, the two ladders and the resident limit
    src = open(os.path.join(bind.ROOT, "danbing-tk_amd", "csrc", "dbtk_assoc.hip")).read()
    dev = open(os.path.join(bind.ROOT, "danbing-tk_amd", "csrc", "dbtk_assoc_perm_dev.h")).read()
    assert "h->ident = n == ns;" in src and "const bool res = n <= AS_SEG;" in dev
    assert len(re.findall(r"k_assoc_scan<(?:true|false), (?:true|false)>\)", src)) == 4
    assert len(set(re.findall(r"k_assoc_perm<(?:true|false), (?:true|false), (?:true|false)>", dev))) == 8
    # the sizes of B and C are the kernel's own
    assert (AS_GRID, AS_ITEM_ROWS, AS_ROWS, AS_CHUNK, AS_SEG) == (2048, 256, 32, 8, 512) and B_ITEMS == 4101
    assert abi.ASSOC_ALL_PAIRS_MAX == 8 * AS_CHUNK and (B_B + 1) % AS_CHUNK and B_B + 1 > AS_CHUNK
    assert all((B + 1) % AS_CHUNK == 0 for B in C_BS + [WIDE_B]) and all(q % AS_CHUNK == 0 for q in C_QS)


def test_the_inputs_keep_their_margins_without_a_gpu():
    """What the GPU tests below assert of their inputs before they compare, on the model alone and on every case of A, B and C
    (test_assoc_gpu.assert_margins, test_assoc_covar_gpu.share_margins, assoc_perm_model.assert_margins, the caps on the bounds: inside
    scan_model and perm_model): the seeds are good wherever the suite runs."""
    for n, ns, q, B in case_lists()["A"]:
        case_a(n, q, B)
    for n, ns, q, B in case_lists()["B"]:
        c = case_b(n, ns, q, B)
        assert c["nitems"] == B_ITEMS
    for n, ns, q, B in case_lists()["C"]:
        if (n, ns) in WIDE_SHAPES:
            c = case_wide(n, ns, B)
            assert all(b["n_tests"] == WIDE_ROWS - 1 and b["skipped"] == 1 for b in c["model"][False]["m"]["best"])
        else:
            case_c(n, ns, q, B)


# ------------------------------------------------------------------------------------------------------------- the tests on the GPU
def scan_ratio(best, hits, mm):
    m, tol = mm["m"], mm["tol"]
    r = [abs(g["r"] - w["r"]) / tol[w["row"]] for g, w in zip(best, m["best"]) if w["n_tests"] and tol[w["row"]] > 0]
    r += [abs(g[3] - w[3]) / tol[w[2]] for g, w in zip(hits, m["hits"])]
    return max(r, default=0.0)


def run(A, d, c, on, label, B=0, perms=None):
    """one pair mode of one case: the scan (with permutations: the permutation scan) against the model, then again for the same bytes"""
    mm = c["model"][on]
    n, q, nrows = len(c["sample_of"]), c.get("q", 0), c["G"].shape[0]
    A.set_pairs(*(c["pairs"] if on else ([], [])))
    go = A.perm_scan_device if B else A.scan_device
    go(d, nrows, nk_cum=c["nk_cum"], p_threshold=P_THRESHOLD)
    best, hits = A.best(), A.hits()
    print(f"{label} pairs={on}: scan max |r - model| / bound {scan_ratio(best, hits, mm):.4f} hits {len(hits)}")
    compare(best, hits, mm["m"], n - q, mm["tol"])
    got = None
    if B:
        pmm = mm["perm"]
        assert (A.permutations() == pmm["perms"]).all()
        got = check(A, pmm["T"], pmm["n_tests"], pmm["bound"], mm["m"], B)
        have = pmm["n_tests"] > 0
        print(f"{label} pairs={on}: perm max |T - model| / bound {(np.abs(got - pmm['T'])[have] / pmm['bound'][have, None]).max():.4f}")
    go(d, nrows, nk_cum=c["nk_cum"], p_threshold=P_THRESHOLD)
    assert A.best() == best and A.hits() == hits
    if B:
        assert np.array([A.perm_stats(p) for p in range(A.P)]).tobytes() == got.tobytes()
    return best, hits, got


def handle_of(dbtk, c, B):
    A = pkg.Assoc(dbtk, c["ns"], c["sample_of"], c["pheno"])
    if c.get("q"):
        A.set_covariates(c["covar"])
        assert A.covariates() == (c["q"], len(c["sample_of"]) - 2 - c["q"])
    if B:
        A.set_permutations(B, seed=c["seed"])
    return A


def all_sample_case(dbtk, hip, n, q, B, twin=False):
    c = case_a(n, q, B)
    r40, nrows = c["r40"], c["G"].shape[0]
    assert c["ns"] == n and sorted(c["sample_of"]) == list(range(n)) and (c["sample_of"] != np.arange(n)).any()
    A = handle_of(dbtk, c, B)
    d = put(hip, c["G"])
    try:
        for on in (False, True):
            best, hits, got = run(A, d, c, on, f"A n={n} q={q} B={B}", B)
            w = c["model"][on]["m"]["best"]
            one = best[c["p_one"]]
            assert one["row"] == r40 + 7 and one["r"] == 1.0 and one["p"] == 0.0 and one["t"] == math.inf and one["se"] == 0.0 and one["locus"] == 5
            assert best[c["p_tie"]]["row"] == w[c["p_tie"]]["row"] != r40 + 20            # duplicate rows: never the upper one,
            assert best[c["p_tie"]]["row"] == r40 + 9 or n == 3 or q
            dup = {h[0]: h[3] for h in hits if h[2] == r40 + 9}
            assert all(h[0] in dup and h[3] == dup[h[0]] for h in hits if h[2] == r40 + 20)  # and they tie bit for bit
            if not on:
                skipped = 3 if q else 2                                                   # constant, not finite, explained by the covariates
                assert all(b["n_tests"] == nrows - skipped and b["skipped"] == skipped for b in best)
            else:
                assert all(h[2] < int(c["nk_cum"][-1]) for h in hits)
            if twin:
                # the same table with the samples listed in ascending order: the order of sample_of reaches nothing but the host's reordering
                order = np.argsort(c["sample_of"], kind="stable")
                t = dict(c, sample_of=np.arange(n), pheno=np.ascontiguousarray(c["pheno"][:, order]))
                if q:
                    t["covar"] = np.ascontiguousarray(c["covar"][:, order])
                S = handle_of(dbtk, t, B)
                try:
                    S.set_pairs(*(c["pairs"] if on else ([], [])))
                    (S.perm_scan_device if B else S.scan_device)(d, nrows, nk_cum=c["nk_cum"], p_threshold=P_THRESHOLD)
                    assert S.best() == best and S.hits() == hits
                    if B:
                        assert np.array([S.perm_stats(p) for p in range(S.P)]).tobytes() == got.tobytes() and S.perm_results() == A.perm_results()
                finally:
                    S.close()
        if B:
            assert any(r["n_ge"] > 0 for r in A.perm_results()[NPHENO:])
    finally:
        hip.free(d)
        A.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", A_PLAIN)
def test_every_sample_plain(dbtk, hip, n):
    all_sample_case(dbtk, hip, n, 0, 0, twin=n == 65)


@pytest.mark.gpu
@pytest.mark.parametrize("n,q", A_COVAR)
def test_every_sample_with_covariates(dbtk, hip, n, q):
    all_sample_case(dbtk, hip, n, q, 0, twin=n == 12)


@pytest.mark.gpu
@pytest.mark.parametrize("n,B", A_PERM)
def test_every_sample_permuted(dbtk, hip, n, B):
    all_sample_case(dbtk, hip, n, 0, B, twin=n == 65)


@pytest.mark.gpu
@pytest.mark.parametrize("n,q,B", A_PERM_COVAR)
def test_every_sample_permuted_with_covariates(dbtk, hip, n, q, B):
    all_sample_case(dbtk, hip, n, q, B, twin=n == 65)


def listed_case(dbtk, hip, c, label, B):
    A = handle_of(dbtk, c, B)
    d = put(hip, c["G"])
    try:
        on = c["pairs"] is not None
        best, hits, _ = run(A, d, c, on, label, B)
        if on:
            assert all(h[2] < int(c["nk_cum"][-1]) for h in hits)                        # no trailing row is tested
        return best
    finally:
        hip.free(d)
        A.close()


B_PASSES = [(n, ns, q, B) for n, ns, q, B in case_lists()["B"]]


@pytest.mark.gpu
@pytest.mark.parametrize("n,ns,q,B", B_PASSES)
def test_many_work_items(dbtk, hip, n, ns, q, B):
    """2 AS_GRID + 5 items on AS_GRID workgroups: the first five take three items, the others two"""
    c = case_b(n, ns, q, B)
    assert c["nitems"] == B_ITEMS > 2 * AS_GRID
    listed_case(dbtk, hip, c, f"B n={n} ns={ns} q={q} B={B}", B)


C_PASSES = [c for c in case_lists()["C"] if (c[0], c[1]) not in WIDE_SHAPES]


@pytest.mark.gpu
@pytest.mark.parametrize("n,ns,q,B", C_PASSES)
def test_whole_units(dbtk, hip, n, ns, q, B):
    """loci that end with a full pass and a full item, phenotype lists, covariates and columns that end with a full chunk"""
    c = case_c(n, ns, q, B)
    best = listed_case(dbtk, hip, c, f"C n={n} ns={ns} q={q} B={B}", B)
    off, idx = c["pairs"]
    want = [sum(C_ROWS[l] for l in range(len(C_ROWS)) if p in idx[off[l]:off[l + 1]]) for p in range(C_P)]
    assert [b["n_tests"] for b in best] == want and all(b["skipped"] == 0 for b in best) and all(w >= C_ROWS[1] for w in want)


@pytest.mark.gpu
@pytest.mark.parametrize("n,ns", WIDE_SHAPES)
@pytest.mark.parametrize("B", [0, WIDE_B])
def test_all_pairs_at_the_limit(dbtk, hip, n, ns, B):
    """DBTK_ASSOC_ALL_PAIRS_MAX phenotypes without a pair list: scanned, not refused; 8 full chunks (with B + 1 = 8: 64 full chunks)"""
    c = case_wide(n, ns, B)
    assert c["pheno"].shape[0] == abi.ASSOC_ALL_PAIRS_MAX == 64
    best = listed_case(dbtk, hip, c, f"C wide n={n} ns={ns} B={B}", B)
    assert all(b["n_tests"] == WIDE_ROWS - 1 and b["skipped"] == 1 for b in best)
