// tests/host_emul/sc_ppsnark_emul.cpp -- TEST-ONLY: the lane bodies of the ppsnark sum-check's kernels (k_sc_sums over ScPpsMemSums / ..BindSums,
// ScPpsInnerSums / ..BindSums, ScPpsWitSums / ..BindSums; k_pps_bind_only: nova_amd/csrc/sumcheck_ppsnark.hpp, sumcheck_inplace.hpp) on the CPU, one fiber
// per thread (simt.hpp), limb bounds asserted (NMX_DEBUG_BOUNDS).  Tables, eq tables, the constants and the challenge in the device's
// internal form come from the test (tests/test_sumcheck_ppsnark_abi.py), so the host half of the call is not trusted here.  Every lane's
// canonical sums are handed back; the test adds them up.  NOT emulated: the block reductions (block_sum_waves: shuffles), the mailbox sum
// (k_sum_partials_mail) and the host half of the device rounds (eq heaps, mailbox, round algebra) -- those run in
// tests/test_gpu_sumcheck_ppsnark.py only.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/msm_pipeline.hpp"
#include "../../nova_amd/csrc/sumcheck_ppsnark.hpp"

using namespace nmx;

namespace {
struct In {
  uint32_t* const* X;                        // the group's tables in header order (5 / 4 / 2), or all 16 (bind only)
  const uint32_t *nk, *one, *r, *eqL, *eqR;  // nk, one, r: 8 words each (r may be null)
  uint32_t* stage;
  uint32_t shift, n, with_inf, bind, grid;
};
template <int FID, int J, class ACC> void put(const ACC& acc, uint32_t first, uint32_t* lane_sums) {
  for (int j = 0; j < J; j++) acc.s[j].to_words(lane_sums + 8 * (J * (size_t)first + j));
}
// which: 0 / 1 memory sums / bind + sums, 2 / 3 inner, 4 / 5 witness, 6 bind only
template <int FID> void run(const In& in, int which, uint32_t* lane_sums) {
  using F = Fp<FID>;
  const F r = in.r ? F::from_words(in.r) : F::zero();
  const uint32_t mask = in.shift >= 32 ? 0xffffffffu : ((1u << in.shift) - 1u);
  simt::launch(in.grid, 256, [&] {
    const uint32_t first = simt::bid() * 256u + simt::tid(), stride = in.grid * 256u;
    if (which <= 1) {
      const ScPpsMemArgs<FID> a{in.X[0], in.X[1], in.X[2], in.X[3], in.X[4], r, F::from_words(in.nk), F::from_words(in.one),
                                in.eqL, in.eqR, in.shift, mask, in.n, in.with_inf};
      ScPpsMemAcc<FID> acc;
      if (which == 0) sc_pps_mem_sums_lane<FID>(a, first, stride, acc);
      else sc_pps_mem_bind_lane<FID>(a, first, stride, acc);
      put<FID, 6>(acc, first, lane_sums);
    } else if (which <= 3) {
      const ScPpsInnerArgs<FID> a{in.X[0], in.X[1], in.X[2], in.X[3], r, in.eqL, in.eqR, in.shift, mask, in.n, in.with_inf};
      ScPpsInnerAcc<FID> acc;
      if (which == 2) sc_pps_inner_sums_lane<FID>(a, first, stride, acc);
      else sc_pps_inner_bind_lane<FID>(a, first, stride, acc);
      put<FID, 4>(acc, first, lane_sums);
    } else if (which <= 5) {
      const ScPpsWitArgs<FID> a{in.X[0], in.X[1], r, in.n};
      ScPpsWitAcc<FID> acc;
      if (which == 4) sc_pps_wit_sums_lane<FID>(a, first, stride, acc);
      else sc_pps_wit_bind_lane<FID>(a, first, stride, acc);
      put<FID, 2>(acc, first, lane_sums);
    } else {
      ScPpsBindArgs<FID> a;
      for (uint32_t t = 0; t < kScPpsTables; t++) a.X[t] = in.X[t];
      a.r = r, a.stage = in.stage, a.n = in.n, a.bind = in.bind;
      sc_pps_bind_only_lane<FID>(a, first, stride);
    }
  });
}
}  // namespace

// lane_sums: grid x 256 x J elements (J = 6 / 4 / 2 by group; which = 6: unused); returns 0
extern "C" int emul_sc_ppsnark(int fid, int which, uint32_t* const* X, const uint32_t* nk, const uint32_t* one, const uint32_t* r, const uint32_t* eqL,
                               const uint32_t* eqR, uint32_t shift, uint32_t n, uint32_t with_inf, uint32_t bind, uint32_t* stage, uint32_t grid,
                               uint32_t* lane_sums) {
  if (which < 0 || which > 6 || grid < 1) return -1;
  const In in{X, nk, one, r, eqL, eqR, stage, shift, n, with_inf, bind, grid};
  switch (fid) {
    case 0: run<0>(in, which, lane_sums); break;
    case 1: run<1>(in, which, lane_sums); break;
    case 2: run<2>(in, which, lane_sums); break;
    case 3: run<3>(in, which, lane_sums); break;
    default: return -1;
  }
  return 0;
}
