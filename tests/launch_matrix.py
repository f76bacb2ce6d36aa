#!/usr/bin/env python3
"""Which instance of the hot path's kernel templates runs, and whether it is right: small batches, each built to select named entries of
the launcher's nine tables (dbtk_hip.hip: K_PROBE, K_PROBE_LOCUS, K_PAIR_USUAL, K_PAIR, K_PAIR_BUB, K_WALK_FAST_LOCUS, K_WALK_FAST,
K_PROBE_GENERAL, K_WALK_PAIRS_LOCUS), each checked against the oracle bit for bit.  tests/test_launch_matrix.py starts
    python tests/launch_matrix.py SET
once per environment set (the launcher reads its switches once per process) with that set's switches and DBTK_TRACE_LAUNCHES=1: the
library then announces every launch on stderr, this driver prints "[scenario] NAME begin / end" around each scenario's batch on the same
stream, and one "RESULT {json}" line per scenario on stdout.

The instances a scenario must launch are computed here (declared), by a restatement of launch_batch's selection rules from k, the longest
read, the parameters, the hint words and the switches — never read from the output."""
import functools
import json
import os
import re
import sys
import tempfile
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import bind  # noqa: E402
import probe_unsorted as pu  # noqa: E402
import synth  # noqa: E402

abi = bind.abi
HIP_SRC = os.path.join(ROOT, "danbing-tk_amd", "csrc", "dbtk_hip.hip")

# ------------------------------------------------------------------ the tables --
CLASSES = ("XS", "S", "L")


def table_dims(src=HIP_SRC):
    """{table: its declared dimensions} from the launcher's source."""
    text = open(src).read()
    return {m.group(1): [int(x) for x in re.findall(r"\[(\d+)\]", m.group(2))]
            for m in re.finditer(r"const Kern<[^>]*> (K_[A-Z_]+)((?:\[\d+\])+) =", text)}


def table_families(src=HIP_SRC):
    """The kernel templates the tables hold instances of: what stands in KERN(...) and in the LOC_CLASSES macros."""
    text = open(src).read()
    return set(re.findall(r"KERN\((k_[a-z_]+)<", text)) | set(re.findall(r"LOC_CLASSES(?:_FUSED)?\((k_[a-z_]+),", text))


def library_names(lib=None):
    """The names KERN(...) stored in the built library: string constants of the form (k_xxx<...>), of the tables' templates (the
    image builder launches three kernels under names of the same form: they stand in no table)."""
    data = open(lib or bind.pkg.LIB_PATH, "rb").read()
    fam = table_families()
    names = {m.group(1).decode() for m in re.finditer(rb"(\(k_[a-z_0-9]+<[A-Za-z0-9_, -]+>\))\x00", data)}
    return sorted(n for n in names if n[1:n.index("<")] in fam)


# ------------------------------------------------------------------ the launcher's rules, restated --
def mz_m_for_k(k):
    return k - 6 if 19 <= k <= 22 else k - 10 if 23 <= k <= 26 else 0


def walkfast_npl(maxlen, k, grmz):
    if k + 4 > 32:
        return 0
    ext = (mz_m_for_k(k) if grmz else k) - 1
    if maxlen <= 32 * 3 + ext and k + 2 <= 32:
        return 3
    return 5 if maxlen <= 32 * 5 + ext else 0


def _b(v):
    return "true" if v else "false"


ENV_SETS = {
    "default": {},
    "locus_always": {"DBTK_LOCUS_ALWAYS": "1"},
    "locus_off": {"DBTK_LOCUS": "0"},
    "fuse1": {"DBTK_FUSE": "1"},
    "fuse0": {"DBTK_FUSE": "0"},
    "walk_ec": {"DBTK_WALK_LOCUS_EC": "1", "DBTK_LOCUS_ALWAYS": "1"},
}
# the scenario lists of the two large sets run in two children each (the lean k classes apart), so that no child takes long
PARTS = ["default", "default:k", "locus_always", "locus_always:k", "locus_off", "fuse1", "fuse0", "walk_ec"]


def declared(sc, env):
    """(instances launch_batch launches for the scenario's batch, whether it launches the sort): launch_batch, line by line.
    The RPGGs here are consistent (T.consistent) and are loaded without bait."""
    k, maxlen, p = sc.k, sc.maxlen, sc.params
    trace, okam, bubbles = p.get("trace", 0), p.get("okam", 1), p.get("bubbles", 0)
    walking, aln = p.get("threading", 0) == 2, p.get("aln", 0)
    nkmax = maxlen - k + 1 if maxlen >= k else 1
    ns = (nkmax + 63) // 64
    nsi = 0 if ns <= 2 else 1 if ns == 3 else 2
    NS = nsi + 2
    recs = bool(trace or okam)
    usual = not trace and not bubbles
    fuse_on = int(env.get("DBTK_FUSE", 3))
    fuse = usual and not recs and bool(fuse_on & 1)
    fuse_lean = usual and not recs and bool(fuse_on & 2)
    images = env.get("DBTK_LOCUS", "1") != "0" and max(5, 2 * k - 40) <= 11   # T.ldir / T.gldir: build_locus_images, build_graph_images
    hints = "DBTK_LOCUS_ALWAYS" not in env                                        # the pinned hint words exist
    # a fresh context's words say "many survivors, sorted"; after a primer without survivors and reset() they say "none, not sorted"
    sort_hint = locus_hint = not (hints and sc.primer)
    m = mz_m_for_k(k)
    wn = k - m + 1 if m else 0
    npl = 0 if (not m or bubbles or wn not in (7, 11)) else 3 if maxlen <= 96 + m - 1 else 5 if maxlen <= 160 + m - 1 else 0
    out, sel = set(), False
    if npl and images and locus_hint:
        out |= {f"(k_probe_locus<{npl}, LOC_NW_{c}, LOC_IMGB_{c}{', true' if fuse else ''}>)" for c in CLASSES}
        sel = True
    lean_fused = fuse_lean and npl != 0 and (not sel or fuse)
    if npl:
        out.add(f"(k_probe<{npl}, {wn}, {_b(sel)}, {_b(lean_fused)}, {_b(sel or sort_hint)}>)")
    else:
        out.add(f"(k_probe_general<{NS}>)")
    if usual and not lean_fused:
        out.add(f"(k_pair_usual<{NS}, true>)" if recs else f"(k_pair_usual<{NS}, false, true>)" if fuse and sel else f"(k_pair_usual<{NS}, false>)")
    out.add(f"(k_pair{'_bub' if bubbles == abi.BUBBLES_TABLE else ''}<{NS}, {_b(recs)}>)")
    if walking:
        walk_txt = bool(aln & 3) and bool(aln & abi.ALN_TEXT)
        walk_aln = bool(aln & 3) and not walk_txt
        wnpl = 0 if (walk_aln or trace) else walkfast_npl(maxlen, k, m != 0)
        if wnpl:
            if images and locus_hint:
                out |= {f"(k_walk_fast_locus<{wnpl}, LOC_NW_{c}, LOC_IMGB_{c}>)" for c in CLASSES}
                if env.get("DBTK_WALK_LOCUS_EC", "0") != "0":
                    out |= {f"(k_walk_pairs_locus<LOC_IMGB_{c}>)" for c in CLASSES}
            out.add(f"(k_walk_fast<{wnpl}, {11 if (m and k - m + 1 == 11) else 7}>)")
    return out, sort_hint


# An entry no batch can select, with the derivation from launch_batch.  (A cap, not a convenience: at most 3 of the 73.)
UNREACHABLE = {
    "(k_pair_usual<4, false, true>)":
        "K_PAIR_USUAL[USUAL_SEL][2] needs a.sel != nullptr and nsi == 2.  a.sel is set only inside `if (npl && a.T.ldir && locus_hint)`, and "
        "npl != 0 needs max_read_len <= 32 * 5 + mz_m - 1 with mz_m = mz_m_for_k(k) <= 16 and k >= mz_m + 6: at most 160 + mz_m - 1 - k + 1 "
        "<= 160 - 6 = 154 k-mer positions, ns = ceil(154 / 64) = 3 slots, nsi <= 1.  nsi == 2 needs more than 192 positions.",
}


# ------------------------------------------------------------------ loci and reads --
def merge_loci(*groups):
    g0 = groups[0]
    assert all(g.flank == g0.flank and g.nhap == g0.nhap for g in groups)
    return synth.Loci(flank=g0.flank, haps=[sum((g.haps[h] for g in groups), []) for h in range(g0.nhap)], nloci=sum(g.nloci for g in groups), nhap=g0.nhap)


N_PER_CLASS = 3


@functools.lru_cache(maxsize=None)
def loci_classes():
    """Three groups of loci whose index image at k = 21 takes 2^9, 2^10 and 2^11 buckets (loc_lgnb_for: 16 << lg >= 5 * keys; at most 1 638,
    1 639 .. 3 276 and 3 277 .. 6 553 keys): 600 flank k-mers and the k-mers of the TR — two copies of a motif of 400 bases for the
    small class, of 1 500 for the middle one, of 4 000 for the large one (a repeat of a short motif has few distinct k-mers however long it is: 120 single-base variants of
    a 40-base motif give at most 2 500).  test_launch_matrix.py asserts the classes on the CPU."""
    kw = dict(nloci=N_PER_CLASS, nhap=2, flank=300, variation=1.0)
    return merge_loci(synth.make_loci(seed=301, tr_min=800, tr_max=850, motif_min=400, motif_max=400, **kw),
                      synth.make_loci(seed=302, tr_min=3000, tr_max=3100, motif_min=1500, motif_max=1500, **kw),
                      synth.make_loci(seed=303, tr_min=8000, tr_max=8100, motif_min=4000, motif_max=4000, **kw))


def _palindrome(k, seed):
    half = synth.BASES[np.random.default_rng(seed).integers(0, 4, k // 2)]
    return np.concatenate([half, synth.revcomp(half)])


@functools.lru_cache(maxsize=None)
def loci_plain(k=21):
    """Eight ordinary loci; at an even k locus 0 carries a self-complementary k-mer in the middle of every haplotype's TR (such k-mers
    exist at even k only: the canonical form of both strands is the k-mer itself)."""
    L = synth.make_loci(nloci=8, nhap=3, flank=500, seed=5 + k, tr_min=120, tr_max=700)
    if k % 2 == 0:
        pal = _palindrome(k, 900 + k)
        for h in range(L.nhap):
            s = L.haps[h][0]
            mid = L.flank + (len(s) - 2 * L.flank) // 2
            L.haps[h][0] = np.concatenate([s[:mid], pal, s[mid:]])
    return L


@functools.lru_cache(maxsize=None)
def loci_shared():
    return synth.make_loci(nloci=16, nhap=2, flank=500, seed=7, shared_frac=0.8)


LOCI = {"classes": loci_classes, "shared": loci_shared}


def get_loci(key, k):
    return loci_plain(k) if key == "plain" else LOCI[key]()


def tail_pairs(loci, L, k):
    """One pair per locus whose two mates END inside the TR, at full length L: mate 1 ends on the TR's last base, mate 2 (reverse strand) on
    its first — the locus k-mers of a read's last positions are the ones a kernel with too few positions per lane would lose."""
    out = synth.Reads()
    for l in range(loci.nloci):
        s = loci.haps[0][l]
        e = len(s) - loci.flank
        if e - L < 0 or loci.flank + L > len(s):
            continue
        out.seqs += [s[e - L:e].tobytes(), synth.revcomp(s[loci.flank:loci.flank + L]).tobytes()]
        out.titles.append(f"tail{l}")
    return out


def pal_pairs(loci, k, L):
    """Pairs across the self-complementary k-mer of locus 0 (even k): it stands in the first mate, read forward, and in the second, read from
    the other strand — and the same two mates in the other order."""
    out = synth.Reads()
    pal = _palindrome(k, 900 + k).tobytes()
    for h in range(loci.nhap):
        s = loci.haps[h][0]
        i = s.tobytes().index(pal)
        a, b = s[i - 5:i - 5 + L].tobytes(), synth.revcomp(s[i + k + 5 - L:i + k + 5]).tobytes()
        assert len(a) == L and len(b) == L
        out.seqs += [a, b, b, a]
        out.titles += [f"pal{h}", f"pal{h}r"]
    return out


FEW = 6


def batch(key, k, L, per_locus, seed, sub=0.004, **kw):
    """per_locus pairs of every locus at read length L (so the list in locus order has items of that many pairs), the tail pairs, and a few
    pairs of k, k + 1 and 60 bases (one position, two, a short read)."""
    loci = get_loci(key, k)
    frag = (max(300, L + 40), max(520, L + 200))
    # (the last locus has 6 pairs only, fewer than LOC_MIN_PAIRS: no item of the locus-resident kernels — its pairs are the rest list's)
    parts = [pu.from_locus(loci, l, per_locus if l + 1 < loci.nloci else FEW, seed=seed * 100 + l, rlen=L, sub=sub, frag=frag, **kw) for l in range(loci.nloci)]
    parts.append(tail_pairs(loci, L, k))
    if key == "plain" and k % 2 == 0:
        parts.append(pal_pairs(loci, k, L))
    parts += [synth.sim_reads(loci, npairs=4, rlen=r, seed=seed * 100 + 90 + i, frag=(300, 500)) for i, r in enumerate((k, k + 1, 60))]
    return pu.join(*parts)


WALK = dict(threading=2, thread_cth=85, correction=1, maxncorrection=3, okam=0)  # -gc 85 3


@dataclass
class Scn:
    name: str
    part: str
    k: int
    L: int                      # the longest read
    params: dict
    loci: str = "plain"
    per_locus: int = 24
    primer: bool = False
    reads_kw: dict = field(default_factory=dict)
    classes: tuple = ()         # image classes whose locus-resident instances the scenario claims (the others are launched without an item)
    why: str = ""               # for an instance without a path statistic: why the reads must reach it
    min_passed: int = 0         # pairs the usual-pair kernel must pass on to k_pair (shared flanks, chimeric and spliced pairs)

    @property
    def env(self):
        return ENV_SETS[self.part.split(":")[0]]

    @functools.cached_property
    def reads(self):
        return batch(self.loci, self.k, self.L, self.per_locus, seed=sum(map(ord, self.name)) % 997, **self.reads_kw)

    @functools.cached_property
    def maxlen(self):
        return max(len(s) for s in self.reads.seqs)

    @property
    def walking(self):
        return self.params.get("threading", 0) == 2

    def cth(self):
        return 20 if self.k >= 24 else 45


def lean_limits(k):
    m = mz_m_for_k(k)
    return 96 + m - 1, 160 + m - 1


MODES = {"okam0": dict(okam=0), "okam1": dict(okam=1), "trace": dict(okam=1, trace=1), "walk": WALK}
K_CLASSES = (19, 20, 22, 23, 24, 26)


@functools.lru_cache(maxsize=None)
def scenarios():
    S = []

    def add(name, part, k, L, mode, **kw):
        params = dict(MODES[mode]) if isinstance(mode, str) else dict(mode)
        S.append(Scn(f"{part}/{name}", part, k, L, params, **kw))

    cls_of = lambda k: () if 2 * k - 40 > 11 else CLASSES if k < 23 else CLASSES[max(0, 2 * k - 40 - 9):]
    for part in ("default", "locus_always"):
        # vi x fused x class at k = 21 over the three classes of image, sorted and locus-resident: K_PROBE_LOCUS[*][*][*], K_PROBE[0|2][SEL][*],
        # and the walk's K_WALK_FAST_LOCUS[*][*] + K_WALK_FAST[*][0]
        for L in lean_limits(21):
            for mode in MODES:
                add(f"classes_k21_L{L}_{mode}", part, 21, L, mode, loci="classes", classes=CLASSES,
                    reads_kw=dict(sub=0.02, indel=0.004) if mode == "walk" else {})
        # k = 25 (windows of 11: vi = 1 | 3; images of 2^10 buckets and more): K_PROBE[1|3][SEL][*], K_WALK_FAST[*][1]
        for L in lean_limits(25):
            for mode in MODES:
                add(f"k25_L{L}_{mode}", part, 25, L, mode, classes=("S",))
        add("k21_L175_okam0", part, 21, 175, "okam0", why="first length past the last lean form: every survivor goes through k_probe_general")
    for k in (21, 25):
        for L in lean_limits(k):
            for mode in ("okam0", "okam1"):
                # a list that was not sorted: K_PROBE[vi][P2_UNSORTED][*]
                add(f"unsorted_k{k}_L{L}_{mode}", "default", k, L, mode, primer=True, why="no locus path, no sort: every survivor in the lean kernel's ranges")
                # no images: K_PROBE[vi][P2_WHOLE][*]
                add(f"whole_k{k}_L{L}_{mode}", "locus_off", k, L, mode, why="no images: the lean kernel takes the whole sorted list")
            add(f"whole_k{k}_L{L}_walk", "locus_off", k, L, "walk", why="no graph images: k_walk_fast takes the whole list")
    # nsi: 2, 3 and 4 slots of 64 positions through the general probe kernel, with and without records (K_PROBE_GENERAL, K_PAIR, K_PAIR_USUAL)
    for k, L in ((17, 100), (21, 175), (21, 250)):
        for mode in ("okam0", "okam1", "trace"):
            add(f"nsi_k{k}_L{L}_{mode}", "default", k, L, mode, why="k or length outside the lean forms: the general probe kernel takes every survivor")
    # ... and with the table of novel edges (K_PAIR_BUB): -bu keeps the edges of every position, the lean form does not apply
    for L in (100, 150, 250):
        for okam in (0, 1):
            add(f"bub_L{L}_okam{okam}", "default", 21, L, dict(okam=okam, bubbles=abi.BUBBLES_TABLE, cthreshold=30), reads_kw=dict(sub=0.01, indel=0.002),
                why="bubbles: general probe kernel, every assigned pair's novel edges go through k_pair_bub")
    # work k_pair must do: shared flanks, chimeric and spliced pairs — the usual-pair kernel passes them on (K_PAIR[*][0 | 1 | 2])
    for L in (100, 150, 250):
        for mode in ("okam0", "okam1"):
            add(f"shared_L{L}_{mode}", "default", 21, L, mode, loci="shared", per_locus=12, reads_kw=dict(chimeric=0.5, splice=0.3), min_passed=1,
                why="" if L < 175 else "four slots: general probe kernel")
    # DBTK_FUSE=1: fused locus-resident kernel, unfused lean kernel, K_PAIR_USUAL[USUAL_SEL][0 | 1]; DBTK_FUSE=0: two kernels throughout
    for part in ("fuse1", "fuse0"):
        for L in lean_limits(21):
            add(f"classes_k21_L{L}_okam0", part, 21, L, "okam0", loci="classes", classes=CLASSES)
        add(f"k25_L174_okam0", part, 25, 174, "okam0", classes=("S",))
        add(f"shared_okam0", part, 21, 150, "okam0", loci="shared", per_locus=20, reads_kw=dict(chimeric=0.5, splice=0.3), min_passed=1)
        add(f"k21_L250_okam0", part, 21, 250, "okam0", why="four slots: no lean form, hence no rest list: USUAL_PLAIN")
    # DBTK_WALK_LOCUS_EC=1: K_WALK_PAIRS_LOCUS[*]
    for L in lean_limits(21):
        add(f"classes_k21_L{L}_walk", "walk_ec", 21, L, "walk", loci="classes", classes=CLASSES, reads_kw=dict(sub=0.02, indel=0.004))
    add("k25_L174_walk", "walk_ec", 25, 174, "walk", classes=("S",), reads_kw=dict(sub=0.02, indel=0.004))
    # the lean k classes: both limits and one base beyond, counting with and without records, trace, walk — sorted + locus-resident
    # (fresh context / DBTK_LOCUS_ALWAYS) and, for counting, not sorted
    for part in ("default:k", "locus_always:k"):
        for k in K_CLASSES:
            l3, l5 = lean_limits(k)
            for L in (l3, l5, l5 + 1):
                for mode in MODES:
                    add(f"k{k}_L{L}_{mode}", part, k, L, mode, classes=cls_of(k)[:1] if L <= l5 else (),
                        why="one base past the last lean form: general probe kernel" if L > l5 else
                        "k = 26 has no images (loc_lg_min = 12): the lean kernel takes the whole sorted list" if k == 26 else "")
                if part == "default:k" and L <= l5:
                    add(f"unsorted_k{k}_L{L}_okam0", part, k, L, "okam0", primer=True, why="not sorted: every survivor in the lean kernel's ranges")
        for k in (18, 27):
            add(f"k{k}_L150_okam0", part, k, 150, "okam0", why="k outside 19 .. 26: no minimizer-grouped table, general probe kernel")
    names = [s.name for s in S]
    assert len(set(names)) == len(names)
    return S


def by_part(part):
    return [s for s in scenarios() if s.part == part]


# ------------------------------------------------------------------ what a scenario claims --
def _class_of(name):
    return next((i for i, c in enumerate(CLASSES) if f"LOC_IMGB_{c}" in name), None)


def claimed(sc):
    """The declared instances the scenario CLAIMS to give work.  Launched is not claimed: the locus-resident kernels are launched for all
    three classes of image whether or not a class has an item, and k_pair runs behind the usual-pair kernel whether or not that passed
    a pair on — it is claimed where every survivor is its own (trace, -bu: no usual-pair kernel) or the loci share flank k-mers."""
    out = set()
    for n in declared(sc, sc.env)[0]:
        c = _class_of(n)
        if c is not None and CLASSES[c] not in sc.classes:
            continue
        if n.startswith("(k_pair<") and not (sc.params.get("trace") or sc.min_passed):
            continue
        out.add(n)
    return out


def assigned(sc, ctr):
    """Pairs that were assigned a locus (a walking batch counts its reads at C_THREADING and leaves C_ASGN to the walk's outcome)."""
    return int(ctr[abi.C_THREADING]) // 2 if sc.walking else int(ctr[abi.C_ASGN])


def evidence(sc, n, ps, ctr):
    """Did instance n of the scenario's batch do something?  ps: the path statistics, ctr: the counters of the batch."""
    names = declared(sc, sc.env)[0]
    surv, asgn, thr = int(ctr[abi.C_SURVIVORS]), assigned(sc, ctr), int(ctr[abi.C_THREADING])
    c = _class_of(n)
    if n.startswith("(k_probe_locus"):
        ev = ps["probe_items"][c] > 0 and ps["probe_pairs"][c] >= 16 * ps["probe_items"][c]
        return ev and (ps["fused_done"] > 0 or not n.endswith(", true>)"))
    if n.startswith("(k_walk_fast_locus"):
        return ps["walk_items"][c] > 0 and ps["walk_pairs"][c] > 0
    if n.startswith("(k_walk_pairs_locus"):
        return ps["walk_items"][c] > 0 and ps["walk_locus_ec"] > 0
    if n.startswith("(k_probe<"):
        _, _, sel, fused, _ = n[len("(k_probe<"):-2].split(", ")
        # (not fused, no rest list: no statistic — every survivor is in the ranges of its waves, sc.why)
        return surv > 0 and (sel != "true" or ps["probe_rest"] > 0) and (fused != "true" or ps["lean_done"] > 0) and (sel == "true" or fused == "true" or bool(sc.why))
    if n.startswith("(k_pair_usual"):
        # the pairs no fused kernel resolved are this kernel's; over the rest list (USUAL_SEL) those are the list's
        return asgn > 0 and surv - ps["fused_done"] - ps["lean_done"] > 0 and (not n.endswith(", false, true>)") or ps["probe_rest"] > 0)
    if n.startswith("(k_pair_bub"):
        return surv > 0 and thr > 0   # (-bu: no usual-pair kernel, every survivor is k_pair_bub's)
    if n.startswith("(k_pair<"):
        # trace: every survivor; otherwise the pairs the usual-pair kernel cannot finish — pairs with k-mers of several loci, whose vv
        # words only body_pair reads (DBTK_PS_PAIR_VV)
        return thr > 0 and asgn > 0 and (bool(sc.params.get("trace")) or ps["pair_vv"] > 0)
    if n.startswith("(k_walk_fast<"):
        # (behind the locus-resident form: the pairs of the locus with fewer than LOC_MIN_PAIRS pairs are left to it)
        return thr > 0 and (ps["walk_rest"] > 0 or not any("k_walk_fast_locus" in x for x in names))
    assert n.startswith("(k_probe_general"), n
    return surv > 0 and bool(sc.why)   # no statistic: every survivor is its (sc.why)


# ------------------------------------------------------------------ the driver --
def make_prefix(tmp, key, k):
    d = os.path.join(tmp, f"{key}_k{k}")
    pref = os.path.join(d, "pan")
    if not os.path.isdir(d):
        os.makedirs(d)
        loci = get_loci(key, k)
        synth.write_rpgg_files(synth.build_rpgg_arrays(loci, k), pref)
        synth.write_graph_file(synth.build_graph_arrays(loci, k), pref)
    return pref


def oracle_run(O, go, sc):
    """The oracle's results for the scenario's batch (the graph is loaded into go when the scenario walks)."""
    p = abi.default_params(ksize=sc.k, cthreshold=sc.params.get("cthreshold", sc.cth()), **{k_: v for k_, v in sc.params.items() if k_ != "cthreshold"})
    seq, off = sc.reads.packed()
    if sc.walking:
        return p, O.align_walk(go, p, seq, off, trace=bool(p.trace))
    if p.bubbles:
        q = abi.Params.from_buffer_copy(p)
        q.bubbles = 1
        return p, O.align_ex(go, q, seq, off, trace=False)
    return p, O.align(go, p, seq, off, trace=bool(p.trace))


def nontrivial(sc, o):
    c = o["counters"]
    return int(c[abi.C_SURVIVORS]) > 0 and assigned(sc, c) > 0 and int(o["counts_file"].sum()) > 0


def compare(sc, g, order, o, r, recs, walk=None, nloci=0):
    """Every comparison exact; returns a string naming the first difference, or ""."""
    co = np.zeros(g.ntrkmers, np.uint64)
    np.add.at(co, order, o["counts_file"])
    if not (co == r["counts"]).all():
        return f"{int((co != r['counts']).sum())} k-mer counts differ"
    if not ((o["kmc"] == r["kmc"]).all() and (o["nmapread"] == r["nmapread"]).all()):
        return "kmc / nmapread differ"
    if not (o["counters"] == r["counters"]).all():
        return f"counters differ: {o['counters'].tolist()} {r['counters'].tolist()}"
    if sc.params.get("trace") and not sc.walking:
        d = bind.recs_equal(o["recs"], recs, sc.reads.npairs)
        if d >= 0:
            return f"record {d}: {bind.rec_str(o['recs'][d])} | {bind.rec_str(recs[d])}"
    if walk is not None:
        res, nres = walk
        if nres != o["nres"] or bind.walk_res_equal(res, o["res"], nres, nloci, every_mate=False) < 0:
            return f"walk results differ ({nres} against {o['nres']})"
    return ""


def bub_table(ctx):
    loci, edges, counts = ctx.bubbles(0)
    return dict(zip(zip(loci.tolist(), edges.tolist()), counts.tolist()))


def bub_want(ev):
    want = {}
    for l, e in zip(ev["locus"], ev["edge"]):
        want[(int(l), int(e))] = want.get((int(l), int(e)), 0) + 1
    return want


def run_part(part, out=sys.stdout, err=sys.stderr):
    dbtk, O = bind.pkg.Dbtk(), bind.Oracle()
    handles = {}
    nbad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for sc in by_part(part):
            hk = (sc.loci, sc.k)
            if hk not in handles:
                pref = make_prefix(tmp, sc.loci, sc.k)
                go = O.load(pref, sc.k)
                O.load_graph(go, pref + ".graph.kmers")
                g = dbtk.load(pref, sc.k, flags=abi.LOAD_GRAPH)
                handles[hk] = (g, go, g.output_order().astype(np.int64))
            g, go, order = handles[hk]
            p, o = oracle_run(O, go, sc)
            seq, off = sc.reads.packed()
            ctx = dbtk.context(g, p)
            if sc.primer:
                ctx.align(*pu.primer().packed())
                assert int(ctx.counts()["counters"][abi.C_SURVIVORS]) == 0
                ctx.reset()
            print(f"[scenario] {sc.name} begin", file=err, flush=True)
            recs, _ = ctx.align(seq, off)
            r = ctx.counts()
            print(f"[scenario] {sc.name} end", file=err, flush=True)
            walk = None
            if sc.walking:
                res, _, nres = ctx.walk_results(sc.reads.npairs)
                walk = (res, nres)
            diff = compare(sc, g, order, o, r, recs, walk, g.nloci)
            if not diff and p.bubbles and bub_table(ctx) != bub_want(o["events"]):
                diff = "table of novel edges differs"
            ps = ctx.path_stats()
            ctx.close()
            nbad += bool(diff)
            print("RESULT " + json.dumps(dict(name=sc.name, exact=not diff, diff=diff, ps=ps, ctr=[int(x) for x in r["counters"]])), file=out, flush=True)
        # -ae text where the lean walk kernels write the records themselves: one scenario per walking part, as dense_slice_checks does
        for sc in [s for s in by_part(part) if s.walking and s.L <= lean_limits(s.k)[1]][:1]:
            g, go, order = handles[(sc.loci, sc.k)]
            seq, off = sc.reads.packed()
            po = abi.default_params(ksize=sc.k, cthreshold=sc.cth(), aln=2, **sc.params)
            pd = abi.default_params(ksize=sc.k, cthreshold=sc.cth(), aln=2 | abi.ALN_TEXT, **sc.params)
            oa = O.align_walk(go, po, seq, off)
            exp = []
            for i in range(oa["nres"]):
                w = oa["res"][i]
                if w.dst != g.nloci:
                    c1, a1 = O.cigar_annot(oa["trecs"][2 * i])
                    c2, a2 = O.cigar_annot(oa["trecs"][2 * i + 1])
                    exp.append((w.pair, w.dst, f"{c2}\t{a2}\t{c1}\t{a1}"))
            ctx = dbtk.context(g, pd)
            ctx.align(seq, off)
            ok = ctx.aln_text(sc.reads.npairs) == exp and len(exp) > 0
            ctx.close()
            nbad += not ok
            print("RESULT " + json.dumps(dict(name=sc.name + "+ae", exact=ok, diff="" if ok else "-ae text differs", ps=None, ctr=None)), file=out, flush=True)
        for g, go, _ in handles.values():
            O.free(go)
            g.close()
    return nbad


def main():
    part = sys.argv[1] if len(sys.argv) > 1 else "default"
    nbad = run_part(part)
    n = len(by_part(part))
    print(f"{n - nbad if nbad <= n else 0}/{n} scenarios bit-exact")
    return 1 if nbad else 0


if __name__ == "__main__":
    sys.exit(main())
