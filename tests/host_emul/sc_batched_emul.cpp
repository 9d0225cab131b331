// tests/host_emul/sc_batched_emul.cpp -- TEST-ONLY: the lane bodies of the batched cubic sum-check's kernels (k_sc_sums over ScBatchedSums
// and ScBatchedBindSums, k_scb_bind_only: nova_amd/csrc/sumcheck_batched.hpp, sumcheck_inplace.hpp) on the CPU, one fiber per thread (simt.hpp), limb bounds asserted
// (NMX_DEBUG_BOUNDS).  Tables, eq tables, the alphas and the challenge in the device's internal form come from the test
// (tests/test_sumcheck_batched_abi.py), so the host half of the call is not trusted here.  Every lane's pair of canonical sums is
// handed back; the test adds them up.  NOT emulated: the block reduction (block_sum_waves: shuffles), k_sum_partials_mail and the host
// half (eq heaps, mailbox, round algebra) -- those run in tests/test_gpu_sumcheck_batched.py only.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/msm_pipeline.hpp"
#include "../../nova_amd/csrc/sumcheck_batched.hpp"

using namespace nmx;

namespace {
struct In {
  uint32_t k;
  uint32_t* const* A;
  uint32_t* const* B;
  uint32_t* const* C;
  const uint32_t *alpha, *nk, *r, *eqL, *eqR;  // alpha: k x 8 words (alpha R' mod p); nk, r: 8 words
  uint32_t* stage;
  uint32_t shift, n, with_inf, bind, grid;
};
template <int FID> ScBatchedArgs<FID> args(const In& in) {
  ScBatchedArgs<FID> a{};
  for (uint32_t i = 0; i < in.k; i++) {
    a.A[i] = in.A[i], a.B[i] = in.B[i], a.C[i] = in.C[i];
    a.alpha[i] = Fp<FID>::from_words(in.alpha + 8 * i);
  }
  a.nk = Fp<FID>::from_words(in.nk);
  a.r = in.r ? Fp<FID>::from_words(in.r) : Fp<FID>::zero();
  a.eqL = in.eqL, a.eqR = in.eqR, a.stage = in.stage;
  a.shift = in.shift, a.mask = in.shift >= 32 ? 0xffffffffu : ((1u << in.shift) - 1u);
  a.k = in.k, a.n = in.n, a.with_inf = in.with_inf, a.bind = in.bind;
  return a;
}
// which: 0 sums, 1 bind + sums, 2 bind only
template <int FID> void run(const In& in, int which, uint32_t* lane_sums) {
  const ScBatchedArgs<FID> a = args<FID>(in);
  simt::launch(in.grid, 256, [&] {
    const uint32_t first = simt::bid() * 256u + simt::tid(), stride = in.grid * 256u;
    if (which == 2) {
      sc_batched_bind_only_lane<FID>(a, first, stride);
      return;
    }
    Fp<FID> s0 = Fp<FID>::zero(), s1 = Fp<FID>::zero();
    if (which == 0) sc_batched_sums_lane<FID>(a, first, stride, s0, s1);
    else sc_batched_bind_lane<FID>(a, first, stride, s0, s1);
    s0.to_words(lane_sums + 16 * (size_t)first);
    s1.to_words(lane_sums + 16 * (size_t)first + 8);
  });
}
}  // namespace

// lane_sums: grid x 256 x 2 elements (which = 2: unused); returns 0
extern "C" int emul_sc_batched(int fid, int which, uint32_t k, uint32_t* const* A, uint32_t* const* B, uint32_t* const* C, const uint32_t* alpha,
                               const uint32_t* nk, const uint32_t* r, const uint32_t* eqL, const uint32_t* eqR, uint32_t shift, uint32_t n,
                               uint32_t with_inf, uint32_t bind, uint32_t* stage, uint32_t grid, uint32_t* lane_sums) {
  if (k < 1 || k > kScBatchedMaxK || which < 0 || which > 2 || grid < 1) return -1;
  const In in{k, A, B, C, alpha, nk, r, eqL, eqR, stage, shift, n, with_inf, bind, grid};
  switch (fid) {
    case 0: run<0>(in, which, lane_sums); break;
    case 1: run<1>(in, which, lane_sums); break;
    case 2: run<2>(in, which, lane_sums); break;
    case 3: run<3>(in, which, lane_sums); break;
    default: return -1;
  }
  return 0;
}
