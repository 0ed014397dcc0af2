// TEST INFRASTRUCTURE, CPU only: a thin extern "C" face of the compiled library's OPQMatrix::train for
// tests/gen_golden_opq.py, which builds it against the faiss headers the oracle recipe unpacks (oracle/Makefile.ref) and
// links it with oracle/_ref/libgamma_ref.so.  Nothing of the library is restated here.
#include <faiss/VectorTransform.h>

#include <cstring>

extern "C" int opq_train_ref(int d, int M, long n, const float* x, const float* A0, float* A_out) {
    try {
        faiss::OPQMatrix opq(d, M, d);   // as GammaIVFPQIndex::Init creates it (index/impl/gamma_index_ivfpq.cc:164)
        opq.verbose = false;
        if (A0) opq.A.assign(A0, A0 + (size_t)d * d);   // a preset orthonormal start (OPQMatrix::train keeps a non-empty A)
        opq.train(n, x);
        std::memcpy(A_out, opq.A.data(), sizeof(float) * (size_t)d * d);
        return 0;
    } catch (...) {
        return -1;
    }
}
