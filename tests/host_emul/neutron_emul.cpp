// tests/host_emul/neutron_emul.cpp -- TEST-ONLY: the lane bodies of the NeutronNova kernels (nova_amd/csrc/neutron.hpp) on the CPU, thread by
// thread with the kernels' own thread -> (tile, lane) map, limb bounds asserted (NMX_DEBUG_BOUNDS).  The constants a launch carries (p - Fm,
// the internal-form challenge, the squarings) come from the test (tests/test_neutron_abi.py) in big integers, so the host half of the calls
// is not trusted here.  Of the two sums every thread's canonical totals are handed back and the test adds them up.
// NOT emulated: the block sum (shuffles), the one-block finish, the launches, the staging and the host half.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/msm_pipeline.hpp"
#include "../../nova_amd/csrc/neutron.hpp"

using namespace nmx;

// v: E1, Az1, Bz1, Cz1, E2, Az2, Bz2, Cz2 (the last four unused with POINTS = 1); totals: blocks * 256 * POINTS elements
template <int FID, int POINTS>
static void run_sums(const uint32_t* const* v, const uint32_t* nk, uint32_t left, uint32_t right, uint32_t blocks, uint32_t* totals) {
  NeutronSumArgs<FID> a;
  a.E1 = v[0], a.A1 = v[1], a.B1 = v[2], a.C1 = v[3], a.E2 = v[4], a.A2 = v[5], a.B2 = v[6], a.C2 = v[7];
  a.nk = Fp<FID>::from_words(nk);
  a.left = left, a.right = right;
  for (uint32_t b = 0; b < blocks; b++)      // (no barrier in the lane bodies: plain loops, as k_neutron_sums maps them)
    for (uint32_t t = 0; t < 256; t++) {
      Fp<FID> G[POINTS];
      neutron_sums_lane<FID, POINTS>(a, b * 4u + (t >> 6), blocks * 4u, t & 63u, 64u, G);
      for (int s = 0; s < POINTS; s++) G[s].to_words(totals + 8 * (((size_t)b * 256 + t) * POINTS + s));
    }
}
template <int FID> static int sums_by_points(int points, const uint32_t* const* v, const uint32_t* nk, uint32_t left, uint32_t right, uint32_t blocks,
                                             uint32_t* totals) {
  if (points == 5) run_sums<FID, 5>(v, nk, left, right, blocks, totals);
  else if (points == 1) run_sums<FID, 1>(v, nk, left, right, blocks, totals);
  else return -1;
  return 0;
}
extern "C" int emul_neutron_sums(int fid, int points, const uint32_t* const* v, const uint32_t* nk, uint32_t left, uint32_t right, uint32_t blocks,
                                 uint32_t* totals) {
  if (!left || !right || !blocks) return -1;
  switch (fid) {
    case 0: return sums_by_points<0>(points, v, nk, left, right, blocks, totals);
    case 1: return sums_by_points<1>(points, v, nk, left, right, blocks, totals);
    case 2: return sums_by_points<2>(points, v, nk, left, right, blocks, totals);
    case 3: return sums_by_points<3>(points, v, nk, left, right, blocks, totals);
  }
  return -1;
}
extern "C" uint32_t emul_neutron_blocks(uint64_t left, uint64_t right, uint32_t opt) { return neutron_blocks((size_t)left, (size_t)right, opt); }

template <int FID>
static void run_fold(const uint32_t* w1, const uint32_t* w2, uint32_t n_w, const uint32_t* e1, const uint32_t* e2, uint32_t n_e, const uint32_t* r,
                     uint32_t* w, uint32_t* e) {
  NeutronFoldFn<FID> f;
  f.w1 = w1, f.w2 = w2, f.e1 = e1, f.e2 = e2, f.w = w, f.e = e, f.n_w = n_w, f.r = Fp<FID>::from_words(r);
  for (uint32_t i = 0; i < n_w + n_e; i++) f(i);
}
// r: the internal form of r_b (r_b 2^261 mod p), 8 words
extern "C" int emul_neutron_fold(int fid, const uint32_t* w1, const uint32_t* w2, uint32_t n_w, const uint32_t* e1, const uint32_t* e2, uint32_t n_e,
                                 const uint32_t* r, uint32_t* w, uint32_t* e) {
  switch (fid) {
    case 0: run_fold<0>(w1, w2, n_w, e1, e2, n_e, r, w, e); break;
    case 1: run_fold<1>(w1, w2, n_w, e1, e2, n_e, r, w, e); break;
    case 2: run_fold<2>(w1, w2, n_w, e1, e2, n_e, r, w, e); break;
    case 3: run_fold<3>(w1, w2, n_w, e1, e2, n_e, r, w, e); break;
    default: return -1;
  }
  return 0;
}

template <int FID> static void run_pow(const uint32_t* sq_e, const uint32_t* sq_f, const uint32_t* unit, uint32_t left, uint32_t n, uint32_t* out) {
  NeutronPowFn<FID> f;
  for (int b = 0; b < kNeutronPowBits; b++) f.sq_e[b] = Fp<FID>::from_words(sq_e + 8 * b), f.sq_f[b] = Fp<FID>::from_words(sq_f + 8 * b);
  f.unit = Fp<FID>::from_words(unit), f.left = left, f.out = out;
  for (uint32_t i = 0; i < n; i++) f(i);
}
// sq_e / sq_f: 31 elements each, tau^(2^b) and (tau^left)^(2^b) in the internal form; unit: the stored form of 1
extern "C" int emul_neutron_pow(int fid, const uint32_t* sq_e, const uint32_t* sq_f, const uint32_t* unit, uint32_t left, uint32_t n, uint32_t* out) {
  switch (fid) {
    case 0: run_pow<0>(sq_e, sq_f, unit, left, n, out); break;
    case 1: run_pow<1>(sq_e, sq_f, unit, left, n, out); break;
    case 2: run_pow<2>(sq_e, sq_f, unit, left, n, out); break;
    case 3: run_pow<3>(sq_e, sq_f, unit, left, n, out); break;
    default: return -1;
  }
  return 0;
}
