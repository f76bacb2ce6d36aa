"""The bytes danbing-tk-pred's kernels make, pinned: SHA-256 digests of the raw matrix, the corrected matrix and Bias of a whole-matrix
and of a windowed dbtk_pred_t, and of the three dosage tables, over two small seeded cohorts (tests/golden/pred_pinned.json).  The other
pred tests compare the paths with each other and with the oracle to a tolerance; this one says that a change which must not alter a
bit has not, and on every path.  The digests were recorded from the library as it was before the kernels' tile body, locus-span line
and handle set-up were each written once (measure() below, run against that build on an MI355X)."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import bind
from test_pred import make_cohort
from test_pred_device import _Hip

pkg = bind.pkg
GOLDEN = os.path.join(bind.ROOT, "tests", "golden", "pred_pinned.json")
# ns -> seed of make_cohort(ntr = 12, max_k = 3000).  ns = 1: one sample, every tile ragged; ns = 70: a second, ragged block of 64
# samples for the bias kernels, three tiles of 32 (the last ragged) for the load kernels
COHORTS = {1: 40, 70: 43}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def cohort(ns):
    meta, counts, depths = make_cohort(COHORTS[ns], ns=ns, ntr=12, max_k=3000)
    counts.setflags(write=False)
    return meta, counts, depths


def locus_sizes(meta):
    nks = np.diff(np.concatenate([[0], meta["nk_cum"].astype(np.int64)]))
    niks = np.diff(np.concatenate([[0], meta["nik_cum"].astype(np.int64)]))
    return nks, niks


@pytest.mark.parametrize("ns", sorted(COHORTS))
def test_the_cohorts_are_what_they_claim(ns):
    meta, counts, depths = cohort(ns)
    nks, niks = locus_sizes(meta)
    assert len(nks) == 12 and counts.shape == (ns, meta["nk"])
    assert (nks == 0).any()                                       # a locus without k-mers
    assert ((nks > 0) & (niks == 0)).any()                        # a locus without invariant k-mers
    assert (nks > 2048).any()                                     # two work items of the dosage pass
    assert ((nks > 0) & (nks < 64)).any() and meta["nk"] % 64     # less than a tile; a ragged last tile along the k-mers
    assert (niks > 64).any()                                      # more invariant k-mers than one turn of the window's bias kernel


def measure(lib, ns):
    """{path: {table: digest}} of the cohort's outputs through `lib`, and the digest of the inputs they were made from."""
    meta, counts, depths = cohort(ns)
    args = (meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"])
    out = {"inputs": sha(np.concatenate([a.view(np.uint8).ravel() for a in (counts, depths) + args]))}

    def whole(load):
        P = pkg.Pred(lib, ns, *args, nk=meta["nk"])
        load(P)
        d = {"raw": sha(P.matrix())}
        P.correct()
        d.update(bias=sha(P.bias()), corrected=sha(P.matrix()))
        P.close()
        return d

    def host_loads(P):
        for s0 in range(0, ns, 23):                               # ragged transfers
            P.load(s0, counts[s0:s0 + 23], depths[s0:s0 + 23])

    def device_loads(P):                                          # n = 1: the column kernel; n > 1: the tile kernel
        hip = _Hip()
        d = hip.put(np.ascontiguousarray(counts))
        P.load_device(0, 1, d.value, depths[:1])
        if ns > 1:
            P.load_device(1, ns - 1, d.value + 8 * meta["nk"], depths[1:])
        hip.free(d)

    out["whole"] = whole(host_loads)
    out["whole_device"] = whole(device_loads)

    nks, _ = locus_sizes(meta)
    W = pkg.PredWindowed(lib, ns, *args, int(nks.max()), nk=meta["nk"])
    raw, cor, first = [], [], 0
    while first < meta["ntr"]:
        end, row0, rows = W.window(first)
        for s0 in range(0, ns, 23):
            W.load(s0, counts[s0:s0 + 23, row0:row0 + rows], depths[s0:s0 + 23])
        r, c = W.outputs()
        raw.append(r); cor.append(c)
        first = end
    assert len(raw) > 1
    out["windowed"] = {"raw": sha(np.concatenate(raw)), "bias": sha(W.bias()), "corrected": sha(np.concatenate(cor))}
    W.close()

    D = pkg.Dosage(lib, ns, *args, nk=meta["nk"])
    for s0 in range(0, ns, 23):
        D.load(s0, counts[s0:s0 + 23], depths[s0:s0 + 23])
    D.finish()
    out["dosage"] = {"kms": sha(D.kms()), "bias": sha(D.bias()), "values": sha(D.values())}
    D.close()
    return out


def agree(m):
    """What the other pred tests say the paths share, bit for bit (checked on the measurement before it was recorded, too)."""
    return m["whole_device"] == m["whole"] and m["windowed"] == m["whole"] and m["dosage"]["bias"] == m["whole"]["bias"]


@pytest.mark.gpu
@pytest.mark.parametrize("ns", sorted(COHORTS))
def test_pinned_bytes(ns):
    want = json.load(open(GOLDEN))[str(ns)]
    got = measure(pkg.Dbtk(), ns)
    assert got["inputs"] == want["inputs"], "make_cohort no longer makes the cohort the digests were recorded from"
    for path, pinned in (("whole", "whole"), ("whole_device", "whole"), ("windowed", "windowed"), ("dosage", "dosage")):
        assert got[path] == want[pinned], path
    assert agree(got)
