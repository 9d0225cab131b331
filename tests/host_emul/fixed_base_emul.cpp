// tests/host_emul/fixed_base_emul.cpp -- TEST-ONLY: the kernels of nova_amd/csrc/fixed_base.hpp on the CPU, one fiber per thread (simt.hpp),
// limb bounds asserted (NMX_DEBUG_BOUNDS): the table build and the multiplication pass, each with the block normalisation (LDS product tree,
// barriers, lane 0's inversion), with the kernels' own index maps, plus the two host helpers the library calls (window bases, squarings of
// tau).  Points come back as the kernels store them: x || y in the internal form (x * 2^261 mod p), all zero for the identity; the test
// (tests/test_fixed_base_abi.py) converts in big integers.
// NOT emulated: the launches, the staging of host scalars, the key's MSM window tables, the concurrency of the flag word's atomic.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/msm_pipeline.hpp"
#include "../../nova_amd/csrc/fixed_base.hpp"

using namespace nmx;

template <int CID> static int run_table(uint32_t c, const uint32_t* base16, uint32_t* table, uint32_t* flags) {
  using C = CurveT<CID>;
  constexpr int BF = C::BF;
  const uint32_t W = fb_windows(FpParams<C::SF>::BITS, c);
  Affine<BF> B;
  B.x = Fp<BF>::from_words(base16 ? base16 : C::GX).to_internal().canon();
  B.y = Fp<BF>::from_words(base16 ? base16 + 8 : C::GY).to_internal().canon();
  std::vector<AffineW> win(W);
  fb_window_bases<BF>(B, c, W, win.data());
  const uint32_t total = W * fb_entries(c);
  const FbTableArgs a{win.data(), (AffineW*)table, flags, c, W};
  simt::launch((total + kFbThreads - 1) / kFbThreads, kFbThreads, [&] { k_fb_table<BF>(a); });
  return 0;
}
// table: W (2^c - 1) x 16 words; base16: canonical x || y words, or null for the generator
extern "C" int emul_fb_table(int cid, uint32_t c, const uint32_t* base16, uint32_t* table, uint32_t* flags) {
  if (c < kFbMinC || c > kFbMaxC) return -1;
  switch (cid) {
    case 0: return run_table<0>(c, base16, table, flags);
    case 1: return run_table<1>(c, base16, table, flags);
    case 2: return run_table<2>(c, base16, table, flags);
    case 3: return run_table<3>(c, base16, table, flags);
  }
  return -1;
}

template <int CID>
static int run_mul(uint32_t c, const uint32_t* table, const uint32_t* scalars, uint32_t mont, const uint32_t* tau8, uint32_t begin, uint32_t n,
                   uint32_t* out, uint32_t* flags) {
  using C = CurveT<CID>;
  FbMulArgs<C::SF> m{};
  m.table = (const AffineW*)table, m.scalars = scalars, m.out = (AffineW*)out, m.flags = flags;
  m.n = n, m.c = c, m.W = fb_windows(FpParams<C::SF>::BITS, c), m.scalars_mont = mont, m.begin = begin;
  if (!scalars) fb_tau_squarings<C::SF>(tau8, mont != 0, m.sq);
  simt::launch((n + kFbThreads - 1) / kFbThreads, kFbThreads, [&] { k_fb_mul<C::BF, C::SF>(m); });
  return 0;
}
// scalars: n x 8 words (canonical, or Montgomery when `mont`), or null: tau mode, lane i takes tau^(begin + i) with tau8 in the form `mont` names
extern "C" int emul_fb_mul(int cid, uint32_t c, const uint32_t* table, const uint32_t* scalars, uint32_t mont, const uint32_t* tau8, uint32_t begin,
                           uint32_t n, uint32_t* out, uint32_t* flags) {
  if (c < kFbMinC || c > kFbMaxC || !n || (!scalars && !tau8)) return -1;
  switch (cid) {
    case 0: return run_mul<0>(c, table, scalars, mont, tau8, begin, n, out, flags);
    case 1: return run_mul<1>(c, table, scalars, mont, tau8, begin, n, out, flags);
    case 2: return run_mul<2>(c, table, scalars, mont, tau8, begin, n, out, flags);
    case 3: return run_mul<3>(c, table, scalars, mont, tau8, begin, n, out, flags);
  }
  return -1;
}

// windows and entries per window for (curve, c), and the bits of the flag word
extern "C" void emul_fb_geometry(int cid, uint32_t c, uint32_t* out4) {
  const uint32_t bits = cid < 2 ? 254u : 255u;
  out4[0] = fb_windows(bits, c), out4[1] = fb_entries(c), out4[2] = FB_ERR_SCALAR_RANGE, out4[3] = FB_ANY_IDENTITY;
}
