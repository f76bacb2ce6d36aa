"""The model of tests/eval_model.py against the compiled reference: `fa2kmers -tr -k K -fsi F -fso 0` over the per-locus records
ctg[START - F, END + F) counts, per record, exactly the windows the model counts per BED line (F = k; the record is padded with N
where it would leave the contig).  No device."""
import os
import subprocess

import pytest

import eval_cases
import eval_model
import sim_model
import synth


def fa2kmers_counts(case, d, k):
    """Per locus {k-mer: count} by the reference: one record per BED line of either assembly (the same records, in the same order,
    in both haplotype files; a line of the other assembly is a record of N), summed over the lines of a locus."""
    exe = os.path.join(synth.REFDIR, "fa2kmers")
    if not synth.have_ref() or not os.path.exists(exe):
        pytest.skip("oracle/_ref/fa2kmers is not built")
    F = k
    lines = [(a, i) for a in range(2) for i in range(len(case.beds[a]))]
    fas = []
    for a in range(2):
        seqs = {sim_model.name_of(h): s.upper() for h, s in case.contigs[a]}
        fn = os.path.join(d, f"h{a}.fa")
        with open(fn, "w") as f:
            for n, (la, i) in enumerate(lines):
                rec = "N" * (2 * F + 1)
                if la == a:
                    name, st, en, _ = case.beds[a][i]
                    s = seqs[name]
                    en = min(en, len(s))
                    rec = "".join(s[p] if 0 <= p < len(s) else "N" for p in range(st - F, en + F))
                f.write(f">{n}\n{rec}\n")
        fas.append(fn)
    subprocess.run([exe, "-tr", "-k", str(k), "-fsi", str(F), "-fso", "0", "-on", "T", "-fa", "2", *fas], check=True, cwd=d, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    per_line = []
    for line in open(os.path.join(d, "T.tr.kmers")):
        if line[0] == ">":
            per_line.append({})
        else:
            km, n = line.split()
            per_line[-1][int(km)] = int(n)
    assert len(per_line) == len(lines)
    out = [dict() for _ in range(eval_cases.NLOCI)]
    for (a, i), dct in zip(lines, per_line):
        l = case.beds[a][i][3]
        for km, n in dct.items():
            out[l][km] = out[l].get(km, 0) + n
    return out


@pytest.mark.parametrize("k", [21, 20])
def test_the_models_windows_are_what_fa2kmers_counts(tmp_path, k):
    case = eval_cases.TruthCase(k)
    want = fa2kmers_counts(case, str(tmp_path), k)
    got = case.window_counts()
    assert got == want
    # the case holds what it says: no window, one window, clipped, N inside, a locus in both assemblies, a self-complementary k-mer at even k
    assert got[1] == {} and sum(got[2].values()) == 1 and sum(got[11].values()) > 5000 and max(got[11].values()) > 700
    palin = eval_model.canon("ACGT" * 5, 20)
    assert (palin in got[12]) == (k == 20)
    name, st, en, l = case.beds[0][[b[3] for b in case.beds[0]].index(14)]
    assert en == len(dict((sim_model.name_of(h), s) for h, s in case.contigs[0])[name]) + 37 and sum(got[14].values()) == en - 37 - st - k + 1


def test_truth_takes_the_tr_kmers_of_the_locus_only():
    counts = [{5: 2, 6: 1, 9: 4}, {5: 3}]
    slots = [{5: 0, 6: 1}, {7: 2}]
    assert eval_model.truth(counts, slots, 3) == ([2, 1, 0], [7, 3])


def test_sums_and_text():
    x, y, beg = [0, 2, 3, 0, 0], [5, 4, 6, 0, 9], [0, 3, 3, 5]
    s = eval_model.sums(x, y, beg, windows=[11, 0, 2])
    assert s[0] == dict(nk=3, n1=2, Sx=5, Sy=15, Sy1=10, Sxy=26, Sxx=13, Syy=77, Syy1=52, windows=11)
    assert s[1] == dict(nk=0, n1=0, Sx=0, Sy=0, Sy1=0, Sxy=0, Sxx=0, Syy=0, Syy1=0, windows=0)
    assert eval_model.columns(s[0]) == (2.0, 7.5, 676 / (13 * 77), 5.0, 1.0) and eval_model.columns(s[2]) == (0.0,) * 5
    assert eval_model.tsv_text(s) == eval_model.TSV_HEADER + "0\t3\t2\t11\t5\t15\t10\t26\t13\t77\t52\t2.00\t7.5\t0.6753\t5.0\t1.0000\n" + \
        "1\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0.00\t0.0\t0.0000\t0.0\t0.0000\n2\t2\t0\t2\t0\t9\t0\t0\t0\t81\t0\t0.00\t0.0\t0.0000\t0.0\t0.0000\n"
    assert eval_model.pred_text(s) == eval_model.PRED_HEADER + "11\t5.0\t2.00\t1.0000\n0\t0.0\t0.00\t0.0000\n2\t0.0\t0.00\t0.0000\n"
    assert eval_model.sums(x, y, beg)[0]["windows"] == 5
