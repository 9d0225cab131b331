// tests/host_emul/r1cs_eval_emul.cpp -- TEST-ONLY: the lane body of k_r1cs_eval (nova_amd/csrc/r1cs_eval.hpp) on the CPU, one fiber per
// thread (simt.hpp), limb bounds asserted (NMX_DEBUG_BOUNDS).  The tables, the tagged indices and the internal-form coefficients come
// from the test (tests/test_r1cs_evaluate_abi.py), so the host half of the call is not trusted here.  Every lane's canonical sum is
// handed back; the test adds them up.  NOT emulated: the wave / block reduction (r1cs_eval_block_sum: shuffles), k_r1cs_eval_finish
// and the host half (the folding of the upper variables, the split of T_x) -- those run in tests/test_gpu_r1cs_evaluate.py only.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/msm_pipeline.hpp"
#include "../../nova_amd/csrc/r1cs_eval.hpp"

using namespace nmx;

template <int FID> static void run(const R1csEvalArgs& a, uint32_t k, uint8_t* lane_sums) {
  simt::launch(k * a.bpm, 256, [&] {
    const uint32_t m = simt::bid() / a.bpm, blk = simt::bid() - m * a.bpm;
    const Fp<FID> acc = r1cs_eval_lane<FID>(a, m, blk);
    acc.to_words((uint32_t*)lane_sums + 8 * ((size_t)simt::bid() * 256 + simt::tid()));
  });
}

// indptr / indices / data: k pointers each (u32 arrays; indices carry the class in the top four bits; data in the internal form)
extern "C" int emul_r1cs_eval(int fid, uint32_t k, const uint32_t* const* indptr, const uint32_t* const* indices, const uint32_t* const* data,
                              const uint32_t* rows, const uint32_t* xL, const uint32_t* xR, uint32_t sx, const uint32_t* ty, uint32_t bpm,
                              uint8_t* lane_sums) {
  if (k < 1 || k > kR1csEvalMaxMats) return -1;
  R1csEvalArgs a{};
  uint32_t max_rows = 0;
  for (uint32_t j = 0; j < k; j++) {
    a.indptr[j] = indptr[j], a.indices[j] = indices[j], a.data[j] = data[j], a.rows[j] = rows[j];
    a.colmask[j] = (1u << kSpmvColBits) - 1u;
    max_rows = rows[j] > max_rows ? rows[j] : max_rows;
  }
  a.xL = xL, a.xR = xR, a.sx = sx, a.ty = ty;
  a.bpm = bpm ? bpm : r1cs_eval_blocks(max_rows);
  switch (fid) {
    case 0: run<0>(a, k, lane_sums); break;
    case 1: run<1>(a, k, lane_sums); break;
    case 2: run<2>(a, k, lane_sums); break;
    case 3: run<3>(a, k, lane_sums); break;
    default: return -1;
  }
  return (int)a.bpm;
}
