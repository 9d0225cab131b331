// tests/host_emul/ppsnark_oracles_emul.cpp -- TEST-ONLY: the lane bodies of nova_amd/csrc/ppsnark_oracles.hpp on the CPU, one fiber per thread
// (simt.hpp), limb bounds asserted (NMX_DEBUG_BOUNDS): the gather, and both level-0 passes of the oracles with the kernels' own chunk ->
// (segment, local chunk) map.  The constants of the passes (gamma in the internal form, F R, Tn F, R^2 / F) come from the test
// (tests/test_ppsnark_oracles_abi.py) in big integers, so the host half of the call is not trusted here; between the two passes the TEST
// inverts the chunk products, which stands in for the levels above and the host top (they are nmx_field_batch_invert's).
// NOT emulated: the launches, the staging, the levels above level 0.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/msm_pipeline.hpp"
#include "../../nova_amd/csrc/ppsnark_oracles.hpp"

using namespace nmx;

template <int FID> static void run_gather(const uint32_t* mem, uint32_t n_mem, const uint32_t* addr, uint32_t n, uint32_t mont, uint32_t* out, uint32_t* err) {
  const GatherFn<FID> f{mem, addr, out, err, n_mem, mont};
  simt::launch((n + 255) / 256, 256, [&] {
    const uint32_t i = simt::bid() * 256u + simt::tid();
    if (i < n) f(i);
  });
}
extern "C" int emul_gather(int fid, const uint32_t* mem, uint32_t n_mem, const uint32_t* addr, uint32_t n, uint32_t mont, uint32_t* out, uint32_t* err) {
  switch (fid) {
    case 0: run_gather<0>(mem, n_mem, addr, n, mont, out, err); break;
    case 1: run_gather<1>(mem, n_mem, addr, n, mont, out, err); break;
    case 2: run_gather<2>(mem, n_mem, addr, n, mont, out, err); break;
    case 3: run_gather<3>(mem, n_mem, addr, n, mont, out, err); break;
    default: return -1;
  }
  return 0;
}

// consts: five elements of 8 words -- gamma R, r (the vectors' form), F R, Tn F, R^2 / F, all canonical; tab: 2 k x 4 addresses
// (ppsnark_oracles.hpp); chunk: 2 k Tn elements (backward == 0: the products are written; 1: the inverses are read)
template <int FID> static void run_level0(const uint64_t* tab, uint32_t k, uint32_t n, uint32_t K, const uint32_t* consts, uint32_t* chunk, int backward) {
  PpsOraArgs<FID> a;
  a.tab = tab, a.chunk = chunk;
  a.gamma = Fp<FID>::from_words(consts), a.r = Fp<FID>::from_words(consts + 8), a.form = Fp<FID>::from_words(consts + 16);
  a.step = Fp<FID>::from_words(consts + 24), a.tscale = Fp<FID>::from_words(consts + 32);
  a.n = n, a.K = K, a.Tn = (n + K - 1) / K;
  const uint32_t lanes = 2 * k * a.Tn;
  simt::launch((lanes + 255) / 256, 256, [&] {
    const uint32_t c = simt::bid() * 256u + simt::tid();
    if (c >= lanes) return;
    if (backward) PpsOraBwdFn<FID>{a}(c);
    else PpsOraFwdFn<FID>{a}(c);
  });
}
extern "C" int emul_pps_level0(int fid, const uint64_t* tab, uint32_t k, uint32_t n, uint32_t K, const uint32_t* consts, uint32_t* chunk, int backward) {
  if (!k || !n || !K) return -1;
  switch (fid) {
    case 0: run_level0<0>(tab, k, n, K, consts, chunk, backward); break;
    case 1: run_level0<1>(tab, k, n, K, consts, chunk, backward); break;
    case 2: run_level0<2>(tab, k, n, K, consts, chunk, backward); break;
    case 3: run_level0<3>(tab, k, n, K, consts, chunk, backward); break;
    default: return -1;
  }
  return 0;
}
