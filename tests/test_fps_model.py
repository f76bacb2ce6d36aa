"""The Python model of the FP-specific filter (tests/fps_model.py) against `ktools fps`, byte for byte: on the golden profiles the
reference's baitBuilder wrote (tests/golden/kcp) and on random profile text with entries of all three fates, a locus whose candidates
all die (its header stays) and means that sit exactly on mean +- 2 sd."""
import os
import subprocess

import numpy as np

import bind
import fps_model

KTOOLS = os.path.join(bind.ROOT, "danbing-tk_amd", "bin", "ktools")
GOLD = os.path.join(bind.ROOT, "tests", "golden", "kcp")


def ktools_fps(tmp_path, nloci, fp_text, tp_texts):
    fp = tmp_path / "m.FP_pf.txt"
    fp.write_text(fp_text)
    tps = []
    for i, t in enumerate(tp_texts):
        p = tmp_path / f"m{i}.TP_pf.txt"
        p.write_text(t)
        tps.append(str(p))
    out = tmp_path / "fps.txt"
    r = subprocess.run([KTOOLS, "fps", str(nloci), "21", str(out), str(fp)] + tps, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return out.read_bytes()


def test_model_equals_ktools_fps_on_the_golden_profiles(tmp_path):
    fp, tp0, tp1 = (open(os.path.join(GOLD, n)).read() for n in ("ref.FP_pf.txt", "ref.TP_pf.txt", "tp.TP_pf.txt"))
    fp_stats = fps_model.stats_of_text(fp)
    for tps in ([tp0], [tp0, tp1], [tp1, tp0]):
        kept, loci = fps_model.fps(fp_stats, [fps_model.stats_of_text(t) for t in tps])
        assert fps_model.fps_text(kept, loci).encode() == ktools_fps(tmp_path, 3, fp, tps)
    dropped, plain, widened = fps_model.fates(fp_stats, kept)
    assert dropped > 0 and plain > 0 and widened > 0, (dropped, plain, widened)


def random_tables(seed):
    """One FP+TP table and two TP-only tables over 6 loci and a pool of 60 k-mers, counts 1 .. 4 or 6 .. 9 over 1 .. 6 reads: small moments, so
    equal means, sd 0 and means exactly on the bounds all occur.  Locus 4: every FP entry is the TP entry (dropped: a header alone).
    Locus 5: no TP table holds any of its k-mers."""
    rng = np.random.default_rng(seed)
    pool = [int(x) for x in rng.choice(1 << 42, size=60, replace=False)]

    def counts():
        lo = 1 if rng.random() < 0.6 else 6  # (two ranges: a low FP mean against high TP counts lies outside, and widens)
        return [int(c) for c in rng.integers(lo, lo + 4, int(rng.integers(1, 7)))]
    first, others = [], [[], []]
    for l in range(4):
        for km in pool:
            if rng.random() < 0.5:
                first.append((1, l, km, counts()))
            if rng.random() < 0.5:
                first.append((0, l, km, counts()))
            for o in others:
                if rng.random() < 0.4:
                    o.append((0, l, km, counts()))
    for km in pool[:9]:
        cs = counts()
        first += [(1, 4, km, cs), (0, 4, km, cs)]
        first.append((1, 5, km, counts()))
    # on the bounds: TP counts 1, 3 (mean 2, sd 1) against FP means 0 + 2 * ... = 4 and 0: FP counts [4] sits on mean + 2 sd
    first += [(0, 0, 7, [1, 3]), (1, 0, 7, [4]), (0, 1, 7, [2, 4, 2, 4]), (1, 1, 7, [1]), (0, 2, 7, [2, 2]), (1, 2, 7, [2]), (0, 3, 7, [2, 2]), (1, 3, 7, [3])]
    return fps_model.table_of_counts(first), [fps_model.table_of_counts(o) for o in others]


def test_model_equals_ktools_fps_on_random_profile_text(tmp_path):
    for seed in (1, 2, 3):
        first, others = random_tables(seed)
        fp_stats = fps_model.stats_of(first, 1)
        tabs = [first] + others
        kept, loci = fps_model.fps(fp_stats, [fps_model.stats_of(t, 0) for t in tabs])
        text = fps_model.fps_text(kept, loci)
        assert text.encode() == ktools_fps(tmp_path, 6, fps_model.profile_text(first, 1), [fps_model.profile_text(t, 0) for t in tabs])
        # ... and from the text of the same profiles, and in another order of the TP profiles
        kept2, loci2 = fps_model.fps(fps_model.stats_of_text(fps_model.profile_text(first, 1)), [fps_model.stats_of_text(fps_model.profile_text(t, 0)) for t in reversed(tabs)])
        assert (kept2, loci2) == (kept, loci)
        dropped, plain, widened = fps_model.fates(fp_stats, kept)
        assert dropped >= 20 and plain >= 9 and widened >= 20, (dropped, plain, widened)
        assert ">4\n>5\n" in text and all((5, km) in kept for (l, km) in fp_stats if l == 5), "a header-only locus, and one no TP profile holds"
        assert (0, 7) not in kept and (1, 7) not in kept and (2, 7) not in kept and kept[(3, 7)] == (2, 2)


def test_text_floats_on_ties_and_the_inside_test_at_both_equalities():
    f = fps_model.f32
    assert f(1 / 32) == np.float32("0.0312") and f(3 / 32) == np.float32("0.0938") and f(33 / 32) == np.float32("1.0312")
    assert fps_model.text_floats(32, 33, 35)[0] == np.float32("1.0312")
    assert fps_model.text_floats(4, 10, 30) == (np.float32(2.5), np.float32("1.1180"))
    m, sd = np.float32(1.5), np.float32(0.25)
    assert fps_model.inside(np.float32(1.0), m, sd) and fps_model.inside(np.float32(2.0), m, sd)
    assert not fps_model.inside(np.nextafter(np.float32(1.0), np.float32(0)), m, sd) and not fps_model.inside(np.nextafter(np.float32(2.0), np.float32(3)), m, sd)
