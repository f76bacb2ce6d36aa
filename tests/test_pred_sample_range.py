"""The sample range of a load, first_sample + n, where the sum wraps past 2^64 (include/dbtk_pred.h: DBTK_ERR_ARG for a range outside the
cohort).  The cohort is test_pred_window.py's."""
import ctypes as C

import numpy as np
import pytest

import bind
from test_pred_window import cohort, whole

pkg, abi = bind.pkg, bind.abi


@pytest.mark.gpu
def test_a_sample_range_that_wraps_is_refused():
    """first_sample + n past 2^64 is refused like any range outside the cohort, whichever of the two is the huge one: on the matrix
    handle of dbtk_pred_create (whose matrix keeps its bytes) and on the dosage tables alike."""
    ns = 3
    meta, counts, depths = cohort(ns)
    dbtk = pkg.Dbtk()
    args = (meta["nk_cum"], meta["nik_cum"], meta["iki"], meta["ikmc"])
    P = pkg.Pred(dbtk, ns, *args, nk=meta["nk"])
    D = pkg.Dosage(dbtk, ns, *args, nk=meta["nk"])
    P.load(0, counts, depths)
    D.load(0, counts, depths)
    before, kms = P.matrix(), D.kms()
    assert before.tobytes() == whole(ns)[0].tobytes()
    two, one = np.full((2, meta["nk"]), 7, np.uint64), np.ones(2, np.float32)
    for h, raw_load in ((P, dbtk.L.dbtk_pred_load_samples), (D, dbtk.L.dbtk_dosage_load_samples)):
        with pytest.raises(pkg.DbtkError) as e:
            h.load(2 ** 64 - 1, two, one)
        assert e.value.status == abi.ERR_ARG
        assert raw_load(h.h, 2, 2 ** 64 - 1, two.ctypes.data_as(abi.u64p), one.ctypes.data_as(C.POINTER(C.c_float))) == abi.ERR_ARG
    assert P.matrix().tobytes() == before.tobytes() and (D.kms() == kms).all()
    P.close()
    D.close()
