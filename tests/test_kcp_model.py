"""The Python model of the bait k-mer count profiles (tests/kcp_model.py) against files the reference's baitBuilder wrote from
tests/golden/kcp/in.kam (tests/golden/make_golden_kcp.py): every locus' lines as a set, all five printed fields.  The library is
compared with this model (tests/test_kcp_gpu.py, tests/test_kcp_cli.py)."""
import os

import pytest

import kcp_model

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kcp")
K, NLOCI = 21, 3


def gold(name):
    return open(os.path.join(GOLD, name)).read()


@pytest.fixture(scope="module")
def kam():
    return gold("in.kam").split("\n")


def same_per_locus(text, want_text):
    got, order = kcp_model.parse_profile(text)
    want, _ = kcp_model.parse_profile(want_text)
    assert order == sorted(want), "every locus with an entry, ascending"
    for l in want:
        assert len(got[l]) == len(set(got[l])) == len(want[l])
        assert set(got[l]) == set(want[l]), (l, sorted(set(got[l]) ^ set(want[l]))[:6])


def test_the_golden_input_is_what_the_issue_asks_for(kam):
    rows = [l.split() for l in kam if l]
    assert 0 < len(rows) <= 300
    lens = {len(r[11]) for r in rows} | {len(r[13]) for r in rows}
    assert lens == {20, 21, 100, 150, 256}
    off = sum(1 for r in rows if r[0] != r[1] or int(r[1]) == NLOCI)
    assert 3 * off >= len(rows) and any(int(r[1]) == NLOCI for r in rows)
    text = "".join(r[11] + r[13] for r in rows)
    assert "N" in text and any(c in text for c in "acgt")


def test_model_reproduces_the_reference_profiles(kam):
    tab = kcp_model.from_kam(kam, K, NLOCI)
    same_per_locus(kcp_model.profile_text(tab, 0), gold("ref.TP_pf.txt"))
    same_per_locus(kcp_model.profile_text(tab, 1), gold("ref.FP_pf.txt"))
    assert len(gold("ref.FP_pf.txt")) > 1000 and len(gold("ref.TP_pf.txt")) > 1000


def test_model_tp_only_reproduces_the_reference_tp_run(kam):
    tab = kcp_model.from_kam(kam, K, NLOCI, tp_only=True)
    same_per_locus(kcp_model.profile_text(tab, 0), gold("tp.TP_pf.txt"))
    assert kcp_model.profile_text(tab, 1) == ""


def test_a_kmer_in_both_mates_is_two_observations():
    tab = {}
    read = "ACGTTGCAGGATCCATAGCAAGT"
    rc = read[::-1].translate(str.maketrans("ACGT", "TGCA"))
    kcp_model.add_pair(tab, (read, rc), 21, 2, 1, 1)
    assert len(tab) == 3 and all(v == [2, 2, 2, 1, 1] for v in tab.values())
