// tests/host_emul/ipa_verify_emul.cpp -- TEST-ONLY: the tile body of k_ipa_s (nova_amd/csrc/ipa_verify.hpp) on the CPU, one fiber per
// thread with real barriers (simt.hpp), limb bounds asserted (NMX_DEBUG_BOUNDS).  The kernel's constants come from the test
// (tests/ipa_verify_common.kernel_constants), so the host half of the call is not trusted here.  Built by tests/test_ipa_verify_abi.py.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/msm_pipeline.hpp"
#include "../../nova_amd/csrc/ipa_verify.hpp"

using namespace nmx;

template <int FID>
static void run(const uint8_t* t0, const uint8_t* hs0, const uint8_t* rsq, uint32_t ell, uint64_t lo, uint64_t cnt, uint32_t grid,
                const uint8_t* b, uint8_t* s_out, uint8_t* lane_sums) {
  IpaSArgs<FID> p{};
  p.t0 = Fp<FID>::from_words((const uint32_t*)t0);
  p.hs0 = Fp<FID>::from_words((const uint32_t*)hs0);
  for (uint32_t pos = 0; pos < ell; pos++) p.rsq[pos] = Fp<FID>::from_words((const uint32_t*)rsq + 8 * pos);
  p.ell = ell, p.lb = ell < kIpaSTileLog2 ? ell : kIpaSTileLog2;
  p.lo = lo, p.cnt = cnt;
  p.s = (uint32_t*)s_out, p.b = (const uint32_t*)b;
  static uint32_t tab[9 * kIpaSTile], hf[9 * kIpaSTiles];
  simt::launch(grid, 256, [&] {
    const Fp<FID> acc = b ? ipa_s_block<FID, true>(p, tab, hf) : ipa_s_block<FID, false>(p, tab, hf);
    acc.to_words((uint32_t*)lane_sums + 8 * ((size_t)simt::bid() * 256 + simt::tid()));
  });
}

extern "C" int emul_ipa_s(int fid, const uint8_t* t0, const uint8_t* hs0, const uint8_t* rsq, uint32_t ell, uint64_t lo, uint64_t cnt,
                          uint32_t grid, const uint8_t* b, uint8_t* s_out, uint8_t* lane_sums) {
  if (grid == 0) grid = ipa_s_blocks(lo, cnt, ell < kIpaSTileLog2 ? ell : kIpaSTileLog2);
  switch (fid) {
    case 0: run<0>(t0, hs0, rsq, ell, lo, cnt, grid, b, s_out, lane_sums); break;
    case 1: run<1>(t0, hs0, rsq, ell, lo, cnt, grid, b, s_out, lane_sums); break;
    case 2: run<2>(t0, hs0, rsq, ell, lo, cnt, grid, b, s_out, lane_sums); break;
    case 3: run<3>(t0, hs0, rsq, ell, lo, cnt, grid, b, s_out, lane_sums); break;
    default: return -1;
  }
  return (int)grid;
}
