"""TEST INFRASTRUCTURE: writes tests/golden/opq_train.npz, the yardstick of gamma_hip_opq_train's QUALITY.

Run on a CPU where the oracle recipe has built oracle/_ref/libgamma_ref.so (it contains faiss's VectorTransform.cpp) and left
the unpacked faiss headers in its scratch directory:

    python -m tests.gen_golden_opq

It compiles tests/opq_ref_driver.cpp against those headers, trains the compiled OPQMatrix on every case of
tests/opq_ref.py OPQ_TRAIN_CASES from its default start and from four preset orthonormal starts, and stores for each of
the five matrices the orthonormality defect and the PQ error of the fixed CPU evaluation (opq_ref.pq_error), beside the
same evaluation of the identity.  The spread of the five runs is the reference's own variability between starting points:
the margin the GPU test grants.  Data only goes into the golden."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import opq_ref as OR   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "opq_train.npz")


def build_driver(tmp):
    scratch = os.environ.get("SCRATCH", "/tmp/gamma_ref_build")   # oracle/Makefile.ref's default
    inc = os.path.join(scratch, "faiss-1.7.1")
    ref = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(inc, "faiss", "VectorTransform.h")) or not os.path.exists(os.path.join(ref, "libgamma_ref.so")):
        raise SystemExit("needs the oracle recipe's outputs: make -f oracle/Makefile.ref")
    so = os.path.join(tmp, "libopq_ref_driver.so")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-fopenmp", "-w", "-DFINTEGER=int", "-I" + inc,
                           os.path.join(ROOT, "tests", "opq_ref_driver.cpp"), "-o", so, "-L" + ref, "-lgamma_ref",
                           "-Wl,-rpath," + ref])
    L = C.CDLL(so)
    f32p = C.POINTER(C.c_float)
    L.opq_train_ref.restype = C.c_int
    L.opq_train_ref.argtypes = [C.c_int, C.c_int, C.c_long, f32p, f32p, f32p]
    return L


def main():
    out = {}
    f32p = C.POINTER(C.c_float)
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        for c in OR.OPQ_TRAIN_CASES:
            d, M = c["d"], c["M"]
            x = OR.anisotropic(c["n"], d, c["seed"], c["decay"])
            mats = []
            for start in range(5):
                A0 = None if start == 0 else OR.random_rotation(d, 1000 * c["seed"] + start)
                A = np.empty((d, d), np.float32)
                rc = L.opq_train_ref(d, M, len(x), x.ctypes.data_as(f32p), None if A0 is None else A0.ctypes.data_as(f32p),
                                     A.ctypes.data_as(f32p))
                assert rc == 0
                mats.append(A)
            errs = np.array([OR.pq_error(A, x, M) for A in mats])
            defects = np.array([OR.orthonormality_defect(A) for A in mats])
            ident = OR.pq_error(np.eye(d, dtype=np.float32), x, M)
            print("%s: reference errors %s, identity %.6g, defects %s" % (c["name"], errs, ident, defects))
            # the condition that makes the test mean something: OPQ helps on this data
            assert errs.max() <= 0.8 * ident, "make the data more anisotropic"
            out[c["name"] + "_A"] = np.stack(mats)
            out[c["name"] + "_err"] = errs
            out[c["name"] + "_defect"] = defects
            out[c["name"] + "_err_identity"] = np.float64(ident)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
