"""GPU: gamma_hip_opq_train against tests/golden/opq_train.npz (written by tests/gen_golden_opq.py from the compiled
library's OPQMatrix::train).  The library's training is not bit-reproducible (its own source says so), so what is held
against it is QUALITY: the PQ error of our rotation under the fixed CPU evaluation of tests/opq_ref.py lies within the
reference's worst run plus the spread of its five runs from different starting points -- the reference's own variability,
recorded in the golden -- and below the identity's."""
import os

import numpy as np
import pytest

from gamma_amd import _lib, api
from tests import opq_ref as OR

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "opq_train.npz"))
_trained = {}


def _train(c):
    """(A, objective) of the full 50 alternations, trained once per case"""
    if c["name"] not in _trained:
        x = OR.anisotropic(c["n"], c["d"], c["seed"], c["decay"])
        g = api.GammaHip(0)
        try:
            _trained[c["name"]] = (x,) + g.opq_train(x, c["M"], 50)
        finally:
            g.close()
    return _trained[c["name"]]


@pytest.mark.parametrize("c", OR.OPQ_TRAIN_CASES, ids=lambda c: c["name"])
def test_quality_and_orthonormality(c):
    x, A, obj = _train(c)
    ref_err = GOLDEN[c["name"] + "_err"]
    ident = float(GOLDEN[c["name"] + "_err_identity"])
    err = OR.pq_error(A, x, c["M"])
    defect = OR.orthonormality_defect(A)
    print("%s: our error %.6g (device objective %.6g), reference runs %s, identity %.6g; defect %.3g, reference %s"
          % (c["name"], err, obj, ref_err, ident, defect, GOLDEN[c["name"] + "_defect"]))
    assert err <= ref_err.max() + (ref_err.max() - ref_err.min())
    assert err < ident
    # 4 u: a matrix orthonormalised in double and rounded once to fp32 (2 u from the rounding of two rows' entries in a
    # dot product of unit vectors, doubled for the solver's residual)
    assert defect <= max(float(GOLDEN[c["name"] + "_defect"].max()), 4 * OR.U)


def test_same_input_same_bytes_one_alternation_and_too_few_points():
    c = OR.OPQ_TRAIN_CASES[0]
    x = OR.anisotropic(3000, c["d"], c["seed"], c["decay"])
    g = api.GammaHip(0)
    try:
        A1, o1 = g.opq_train(x, c["M"], 3)
        A2, o2 = g.opq_train(x, c["M"], 3)
        assert A1.tobytes() == A2.tobytes() and o1 == o2
        A3, _ = g.opq_train(x, c["M"], 1)                      # niter = 1 runs
        assert np.isfinite(A3).all() and OR.orthonormality_defect(A3) <= 4 * OR.U
        d = c["d"]
        out = np.empty((d, d), np.float32)
        rc = g.L.gamma_hip_opq_train(g.h, d, 255, x.ctypes.data_as(_lib.f32p), c["M"], 1, out.ctypes.data_as(_lib.f32p), None)
        assert rc == -1 and b"256" in g.L.gamma_hip_last_error(g.h)
        # the trained matrix goes onto a handle like any other
        g.ivfpq_init(d, 16, c["M"], 8, api.METRIC_L2)
        g.opq_set(A1)
        assert g.opq_get().tobytes() == A1.tobytes()
    finally:
        g.close()
