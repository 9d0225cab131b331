// tests/host_emul/spmv_emul.cpp -- TEST-ONLY: spmv_row + st (nova_amd/csrc/spmv_row.hpp), the row body of SpmvFn, SpmvSegFn, SpmvCrossFn and
// k_r1cs_sat, on the CPU over every row of a matrix, limb bounds asserted (NMX_DEBUG_BOUNDS).  The tagged indices and the internal-form
// coefficients come from the test (tests/test_spmv_edges.py), so registration (SpmvClassifyFn, the conversion) is not trusted here.
// NOT emulated: SpmvPairFn (its own copy of the row loop) and k_spmv_heavy -- those run in tests/test_gpu_spmv_edges.py only.
#include <stdint.h>

#include "../../nova_amd/csrc/spmv_row.hpp"

using namespace nmx;

template <int FID>
static void run(const uint32_t* indptr, const uint32_t* indices, const uint32_t* data, const uint32_t* z, uint32_t colmask, uint32_t rows,
                uint32_t* out) {
  for (uint32_t row = 0; row < rows; row++) st<FID>(out, row, spmv_row<FID>(indptr, indices, data, z, colmask, row));
}

// indices carry the class in the top four bits when colmask = 2^28 - 1; data in the internal form; z and out 8 words per element
extern "C" int emul_spmv(int fid, const uint32_t* indptr, const uint32_t* indices, const uint32_t* data, const uint32_t* z, uint32_t colmask,
                         uint32_t rows, uint32_t* out) {
  switch (fid) {
    case 0: run<0>(indptr, indices, data, z, colmask, rows, out); break;
    case 1: run<1>(indptr, indices, data, z, colmask, rows, out); break;
    case 2: run<2>(indptr, indices, data, z, colmask, rows, out); break;
    case 3: run<3>(indptr, indices, data, z, colmask, rows, out); break;
    default: return -1;
  }
  return 0;
}

extern "C" uint32_t emul_spmv_index_mask(uint64_t extent) { return spmv_index_mask((size_t)extent); }
