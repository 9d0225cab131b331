// tests/host_emul/key_ext_emul.cpp -- TEST-ONLY: k_key_lincomb of nova_amd/csrc/key_ext.hpp on the CPU, one fiber per thread (simt.hpp), limb
// bounds asserted (NMX_DEBUG_BOUNDS): the S / D rows and their two block normalisations, the ladder over the digit stream and the final
// block normalisation (LDS product tree, barriers, lane 0's inversion), with the kernel's own index map; plus the host recoding the library
// calls (ke_recode), which is plain C++.  Points go in and come back as the kernel holds them: x || y in the internal form (x * 2^261 mod p),
// all zero for the identity; the test (tests/test_key_ext_abi.py) converts in big integers.
// NOT emulated: the launch, build_key, the key's window tables, the concurrency of the flag word's atomic.
#include <stdint.h>
#include <string.h>

#include "simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/msm_pipeline.hpp"
#include "../../nova_amd/csrc/key_ext.hpp"

using namespace nmx;

// w1, w2: 8 canonical words each (w2 null: one weight); codes: 256 bytes, one position each; returns the length, or -1
extern "C" int emul_ke_recode(const uint32_t* w1, const uint32_t* w2, uint8_t* codes) {
  KeDigits d;
  if (!ke_recode(w1, w2, &d)) return -1;
  for (uint32_t j = 0; j < kKeMaxDigits; j++) codes[j] = (uint8_t)((d.w[j >> 3] >> (4 * (j & 7u))) & 15u);
  return (int)d.len;
}

template <int CID> static int run(const uint32_t* p0, const uint32_t* p1, uint32_t m, const KeDigits& dig, uint32_t* out, uint32_t* flags) {
  KeLincombArgs a{};
  a.p0 = (const AffineW*)p0, a.p1 = (const AffineW*)p1, a.out = (AffineW*)out, a.flags = flags;
  a.m = m, a.k = p1 ? 2u : 1u, a.dig = dig;
  simt::launch((m + kFbThreads - 1) / kFbThreads, kFbThreads, [&] { k_key_lincomb<CurveT<CID>::BF>(a); });
  return 0;
}
// p0, p1: m rows of 16 words (internal form, canonical; all zero = identity), p1 null for one weight; w1, w2: canonical words; out: m rows;
// flags: 2 words, zeroed here.  Returns 0, -1 for bad arguments
extern "C" int emul_key_lincomb(int cid, const uint32_t* p0, const uint32_t* p1, uint32_t m, const uint32_t* w1, const uint32_t* w2, uint32_t* out,
                                uint32_t* flags) {
  KeDigits dig;
  if (!m || !p0 || !w1 || (!p1) != (!w2) || !ke_recode(w1, w2, &dig)) return -1;
  flags[0] = flags[1] = 0;
  switch (cid) {
    case 0: return run<0>(p0, p1, m, dig, out, flags);
    case 1: return run<1>(p0, p1, m, dig, out, flags);
    case 2: return run<2>(p0, p1, m, dig, out, flags);
    case 3: return run<3>(p0, p1, m, dig, out, flags);
  }
  return -1;
}

// the codes of a position and the bit of the flag word
extern "C" void emul_ke_geometry(uint32_t* out8) {
  out8[0] = KE_P0, out8[1] = KE_P1, out8[2] = KE_SUM, out8[3] = KE_DIFF, out8[4] = KE_NEG, out8[5] = FB_ANY_IDENTITY, out8[6] = kKeMaxDigits;
  out8[7] = kFbThreads;
}
