"""`ktools fps` against what the reference's `baitBuilder v2` made of the golden profiles (tests/golden/kcp, per locus as sets), and
`ktools serialize-bt`: the reference's bytes where its ktools is built, and always a file that dbtk_rpgg_load takes and
dbtk_rpgg_view hands back entry by entry."""
import os
import subprocess

import numpy as np

import bind
import kcp_model
import synth

KTOOLS = os.path.join(bind.ROOT, "danbing-tk_amd", "bin", "ktools")
GOLD = os.path.join(bind.ROOT, "tests", "golden", "kcp")


def ktools(*args):
    return subprocess.run([KTOOLS, *map(str, args)], capture_output=True, text=True, timeout=60)


def test_usage_names_both_commands():
    r = ktools()
    assert r.returncode == 0 and "fps" in r.stderr and "serialize-bt" in r.stderr
    assert ktools("fps").returncode == 0 and "FP_pf" in ktools("fps").stderr
    assert ktools("serialize-bt").returncode == 0 and "outPref" in ktools("serialize-bt").stderr
    assert ktools("fps", 3, 21, "out").returncode == 1


def test_fps_equals_the_reference_on_the_golden_profiles(tmp_path):
    out = tmp_path / "fps.txt"
    r = ktools("fps", 3, 21, out, os.path.join(GOLD, "ref.FP_pf.txt"), os.path.join(GOLD, "ref.TP_pf.txt"), os.path.join(GOLD, "tp.TP_pf.txt"))
    assert r.returncode == 0, r.stderr
    got, order = kcp_model.parse_profile(out.read_text())
    want, want_order = kcp_model.parse_profile(open(os.path.join(GOLD, "ref.fps.txt")).read())
    assert order == want_order == sorted(want)
    kept = widened = 0
    for l in want:
        assert len(got[l]) == len(set(got[l])) and set(got[l]) == set(want[l]), (l, sorted(set(got[l]) ^ set(want[l]))[:6])
        assert [int(x.split("\t")[0]) for x in got[l]] == sorted(int(x.split("\t")[0]) for x in got[l]), "ascending by k-mer inside a locus"
        kept += len(want[l])
        widened += sum(1 for x in want[l] if not x.endswith("\t255\t0"))
    nfp = sum(len(v) for v in kcp_model.parse_profile(open(os.path.join(GOLD, "ref.FP_pf.txt")).read())[0].values())
    assert 0 < widened < kept < nfp, "the golden set holds k-mers of all three fates: dropped, kept as 255/0, kept with a TP profile's min/max"


def test_fps_with_a_tp_profile_that_lacks_loci_and_an_fp_locus_that_is_dropped_whole(tmp_path):
    fp = tmp_path / "x.FP_pf.txt"
    tp = tmp_path / "x.TP_pf.txt"
    fp.write_text(">1\n10\t1\t1\t1.0000\t0.0000\n11\t2\t2\t2.0000\t0.0000\n>3\n10\t1\t1\t1.0000\t0.0000\n>5\n12\t4\t4\t4.0000\t0.0000\n")
    tp.write_text(">0\n10\t1\t9\t5.0000\t1.0000\n>3\n10\t1\t3\t1.5000\t0.5000\n>4\n12\t1\t1\t1.0000\t0.0000\n>5\n12\t1\t3\t1.5000\t0.5000\n")
    out = tmp_path / "o.txt"
    assert ktools("fps", 6, 21, out, fp, tp).returncode == 0
    # locus 1: the TP profile has none; locus 3: 1.0 lies inside 1.5 +- 1.0, dropped (the header stays); locus 5: 4.0 outside, widened to 1 / 3
    assert out.read_text() == ">1\n10\t255\t0\n11\t255\t0\n>3\n>5\n12\t1\t3\n"
    assert ktools("fps", 6, 21, out, tmp_path / "none", tp).returncode == 134


def bait_text(rng, nloci, per_locus):
    lines = []
    for l in range(nloci):
        if l % 3 == 2:
            continue  # a locus without baits
        lines.append(f">{l}")
        for km in rng.choice(1 << 40, size=per_locus + l, replace=False):
            mi, ma = [(255, 0), (2, 9), (0, 1), (1, 1)][int(rng.integers(0, 4))]
            lines.append(f"{int(km)}\t{mi}\t{ma}")
    return "\n".join(lines) + "\n"


def parse_kmdb(fn):
    a = np.fromfile(fn, np.uint8)
    nl = int(a[:8].view(np.uint64)[0])
    idx = a[8:8 + 8 * nl].view(np.uint64)
    nk, szv = (int(x) for x in a[8 + 8 * nl:24 + 8 * nl].view(np.uint64))
    ks = a[24 + 8 * nl:24 + 8 * nl + 8 * nk].view(np.uint64)
    vs = a[24 + 8 * nl + 8 * nk:].view(np.uint16)
    assert szv == 2 and len(vs) == nk and int(idx.sum()) == nk
    return nl, idx, ks, vs


def test_serialize_bt_bytes_and_the_file_loads(tmp_path):
    rng = np.random.default_rng(31)
    nloci, k = 7, 21
    txt = tmp_path / "bait.txt"
    txt.write_text(bait_text(rng, nloci, 40))
    r = ktools("serialize-bt", txt, nloci, tmp_path / "mine")
    assert r.returncode == 0, r.stderr
    mine = (tmp_path / "mine.bt.kmdb").read_bytes()
    if synth.have_ref():
        subprocess.run([synth.ref_tool("ktools"), "serialize-bt", str(txt), str(nloci), str(tmp_path / "ref")], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        assert mine == (tmp_path / "ref.bt.kmdb").read_bytes()
    # what the text says, locus by locus
    nl, idx, ks, vs = parse_kmdb(tmp_path / "mine.bt.kmdb")
    want, _ = kcp_model.parse_profile(txt.read_text())
    assert nl == nloci
    at = 0
    for l in range(nloci):
        got = {(int(ks[i]), int(vs[i])) for i in range(at, at + int(idx[l]))}
        assert got == {(int(x.split("\t")[0]), (int(x.split("\t")[1]) << 8) + int(x.split("\t")[2])) for x in want.get(l, [])}
        at += int(idx[l])
    # ... and through the loader: dbtk_rpgg_load with the file as its bait DB, dbtk_rpgg_view
    pref = str(tmp_path / "pan")
    synth.write_rpgg_files(synth.build_rpgg_arrays(synth.make_loci(nloci=nloci, nhap=1, flank=100, seed=3), k), pref)
    g = bind.pkg.Dbtk().load(pref, k, bait_file=str(tmp_path / "mine.bt.kmdb"))
    v = g.view()
    assert (np.ctypeslib.as_array(v.bt_cnt, (nloci,)) == idx).all()
    assert (np.ctypeslib.as_array(v.bt_ks, (len(ks),)) == ks).all() and (np.ctypeslib.as_array(v.bt_vs, (len(ks),)) == vs).all()
    assert ktools("serialize-bt", txt, 2, tmp_path / "few").returncode == 1  # a locus beyond nloci
