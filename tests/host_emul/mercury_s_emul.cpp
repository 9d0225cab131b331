// tests/host_emul/mercury_s_emul.cpp -- TEST-ONLY: the kernels of nmx_mercury_s_poly (nova_amd/csrc/mercury_s.hpp) on the CPU, one fiber per
// thread (simt.hpp: LDS staging and barriers included), limb bounds asserted (NMX_DEBUG_BOUNDS).  The launches are the library's own
// sequence -- the conversion of a1 and gamma a2, the tiled kernel with the plan's grid, the finish -- and the plan is the library's
// (mercury_s_plan); the internal-form gamma comes from the test (tests/test_mercury_prove_abi.py) in big integers.  The output and the
// workspace carry a guard element behind them, checked after the run.
// NOT emulated: the launches themselves, staging of host operands, the arena.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/msm_pipeline.hpp"
#include "../../nova_amd/csrc/mercury_s.hpp"

using namespace nmx;

static constexpr uint32_t kGuard = 0xA5A5A5A5u;

template <int FID>
static int run(const uint32_t* a1, const uint32_t* b1, const uint32_t* a2, const uint32_t* b2, uint32_t b, const uint32_t* gamma, uint32_t mont,
               uint32_t tile_opt, uint32_t* out, uint32_t* plan_out) {
  const MercurySPlan pl = mercury_s_plan(b, tile_opt);
  plan_out[0] = pl.tile, plan_out[1] = pl.ktiles, plan_out[2] = pl.chunks, plan_out[3] = pl.cpt;
  std::vector<uint32_t> t1(8 * (size_t)b), t2(8 * (size_t)b);
  const size_t parts = pl.chunks > 1 ? (size_t)pl.chunks * (b - 1) : 0;
  std::vector<uint32_t> part(8 * (parts + 1), 0xEEEEEEEEu);  // (a slot no live block wrote must not be read: it would not be canonical)
  for (int q = 0; q < 8; q++) part[8 * parts + q] = kGuard;
  const MercurySPrepFn<FID> prep{a1, a2, t1.data(), t2.data(), Fp<FID>::from_words(gamma), b, mont};
  for (uint32_t t = 0; t < 2 * b; t++) prep(t);
  MercurySArgs<FID> a;
  a.a1 = t1.data(), a.a2 = t2.data(), a.b1 = b1, a.b2 = b2, a.part = part.data(), a.out = out;
  a.b = b, a.tile = pl.tile, a.chunks = pl.chunks, a.cpt = pl.cpt;
  simt::launch(pl.ktiles * pl.chunks, 256, [&] { k_mercury_s<FID>(a); });
  if (pl.chunks > 1) {
    const MercurySFinishFn<FID> fin{part.data(), out, b, pl.tile, pl.chunks, pl.cpt};
    for (uint32_t k = 0; k + 1 < b; k++) fin(k);
  }
  for (int q = 0; q < 8; q++)
    if (part[8 * parts + q] != kGuard) return -3;
  return 0;
}

// a1, b1, a2, b2: b elements as stored; gamma: internal form, 8 words; out: b - 1 elements (the caller appends and checks its own guard);
// plan_out: tile, ktiles, chunks, cpt of the plan that ran
extern "C" int emul_mercury_s(int fid, const uint32_t* a1, const uint32_t* b1, const uint32_t* a2, const uint32_t* b2, uint32_t b, const uint32_t* gamma,
                              uint32_t mont, uint32_t tile_opt, uint32_t* out, uint32_t* plan_out) {
  if (b < 2 || (tile_opt != 0 && tile_opt != 16 && tile_opt != 32 && tile_opt != 64)) return -1;
  switch (fid) {
    case 0: return run<0>(a1, b1, a2, b2, b, gamma, mont, tile_opt, out, plan_out);
    case 1: return run<1>(a1, b1, a2, b2, b, gamma, mont, tile_opt, out, plan_out);
    case 2: return run<2>(a1, b1, a2, b2, b, gamma, mont, tile_opt, out, plan_out);
    case 3: return run<3>(a1, b1, a2, b2, b, gamma, mont, tile_opt, out, plan_out);
  }
  return -1;
}
