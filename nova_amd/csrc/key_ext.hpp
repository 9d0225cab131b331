// key_ext.hpp -- out[i] = w1 * L[i] + w2 * R[i] (nmx_bases_fold) and out[i] = r * P[i] (nmx_bases_scale), in HBM: the N-sized methods of the
// reference's CommitmentKeyExtTrait (src/provider/pedersen.rs:430-529: fold :484-497, scale :500-512), which runs one two-point or one-point
// vartime_multiscalar_mul per output inside par_iter.  Included by runtime.hpp; the kernel is instantiated by curve_impl.hpp (the four curve
// TUs).  The device code uses lane-level and block-level primitives only (LDS, barriers, one atomic OR), so tests/host_emul/key_ext_emul.cpp
// runs the same body on the CPU (simt.hpp) with the limb bounds asserted (NMX_DEBUG_BOUNDS).
//
// Many bases, ONE shared scalar (or one shared pair): every output point follows the same digit stream, so the host recodes the weights once
// (ke_recode) and the kernel arguments carry the digits.  The lanes do no scalar handling: no scalar words in HBM, no range check, and every
// lane of every wave takes the same branch at every step of the ladder.
//   ke_recode       Solinas' joint sparse form of (w1, w2): digits u1, u2 in {-1, 0, 1}, at most BITS + 1 positions, joint density 1/2; with
//                   w2 = 0 it is the non-adjacent form of w1 (density 1/3).  Position j is a 4-bit code: 0 nothing, else one of P0, P1,
//                   S = P0 + P1, D = P0 - P1 with bit 3 for the sign.  256 positions = 32 words of kernel argument
//   k_key_lincomb   blocks of 256 lanes, one lane per output point.  k = 2: the lane forms S and D with one complete mixed addition each
//                   (P0 == P1: a doubling / the identity; P0 == -P1: the identity / a doubling; an identity row: the other row) and the
//                   block normalises both to affine rows in LDS with one shared inversion each (fb_block_affine, fixed_base.hpp), so EVERY
//                   addition of the ladder is the mixed XYZZ::add_affine.  Then from the top digit: dbl_in_place, at most one addition per
//                   position (P0 and P1 are re-read from the key, S and D from LDS; an all-zero row -- an identity source row, a cancelled
//                   S or D -- is skipped, as msm.rs:247-249 skips it), and fb_block_affine again for the AffineW row of the new key.  An
//                   output that is the identity is the all-zero row and raises FB_ANY_IDENTITY.
// Per output (len = digit positions <= BITS + 1, J = non-zero positions, about len / 2 for a pair and len / 3 for one weight): len - 1
// doublings that do work (the accumulator is the identity until the top digit is added), J mixed additions, no full addition; for a pair 2
// more mixed additions (S, D) and 3 block normalisations instead of 1 (3 tree products, 5 products and 1/256 inversion each).
//
// Bounds (multiples of p): operands of every addition are canonical rows (< 1: HBM rows, or rows fb_block_affine wrote after canon()); the
// accumulator keeps the XYZZ invariants of curve.hpp (x < 5.3, y < 3.5, zz, zzz < 1.2) since only dbl_in_place and add_affine touch it --
// asserted after every step under NMX_DEBUG_BOUNDS.  S and D enter fb_block_affine inside the same invariants (D's y after adding -P1 to the
// identity is 2p - y < 2 <= 3.5).
//
// Out of scope, on purpose: the GLV endomorphism (all four curves have j = 0; it would halve the doublings), wider per-lane windows, the
// layout of the S / D rows in LDS, any tuning.
#pragma once

#include "fixed_base.hpp"  // fb_block_affine, kFbThreads, FB_ANY_IDENTITY

namespace nmx {

static constexpr uint32_t kKeMaxDigits = 256;  // BITS + 1 <= 256 positions
enum : uint32_t { KE_P0 = 1u, KE_P1 = 2u, KE_SUM = 3u, KE_DIFF = 4u, KE_NEG = 8u };  // a position's code: 0, or one of the four | the sign

struct KeDigits {
  uint32_t w[kKeMaxDigits / 8];  // position j: bits [4 (j % 8), 4 (j % 8) + 4) of w[j / 8]; position 0 is the least significant
  uint32_t len;                  // positions used: the top one is non-zero (0: both weights are zero)
};

// Solinas' joint sparse form (Low-weight binary representations for pairs of integers, Alg. 2) of two 256-bit integers as canonical words;
// w2 == nullptr stands for 0, and the form is then the NAF of w1.  Plain C++, host.  False: more than 256 positions (an operand >= 2^255).
inline bool ke_recode(const uint32_t* w1, const uint32_t* w2, KeDigits* out) {
  uint32_t k[2][8], d[2] = {0u, 0u};
  for (int j = 0; j < 8; j++) k[0][j] = w1[j], k[1][j] = w2 ? w2[j] : 0u;
  for (uint32_t j = 0; j < kKeMaxDigits / 8; j++) out->w[j] = 0u;
  out->len = 0;
  auto nonzero = [&](int i) {
    uint32_t o = d[i];
    for (int j = 0; j < 8; j++) o |= k[i][j];
    return o != 0;
  };
  for (uint32_t pos = 0; nonzero(0) || nonzero(1); pos++) {
    if (pos >= kKeMaxDigits) return false;
    const uint32_t l[2] = {((k[0][0] & 7u) + d[0]) & 7u, ((k[1][0] & 7u) + d[1]) & 7u};  // (k_i + d_i) mod 8
    int u[2];
    for (int i = 0; i < 2; i++) {
      u[i] = (l[i] & 1u) ? 2 - (int)(l[i] & 3u) : 0;                           // l mods 4
      if ((l[i] == 3u || l[i] == 5u) && (l[1 - i] & 3u) == 2u) u[i] = -u[i];  // make the NEXT column zero in both rows
    }
    for (int i = 0; i < 2; i++) {
      if (2 * (int)d[i] == 1 + u[i]) d[i] = 1u - d[i];
      for (int j = 0; j < 7; j++) k[i][j] = (k[i][j] >> 1) | (k[i][j + 1] << 31);
      k[i][7] >>= 1;
    }
    uint32_t code = 0;
    if (u[0] && u[1]) code = (u[0] == u[1] ? KE_SUM : KE_DIFF) | (u[0] < 0 ? KE_NEG : 0u);
    else if (u[0]) code = KE_P0 | (u[0] < 0 ? KE_NEG : 0u);
    else if (u[1]) code = KE_P1 | (u[1] < 0 ? KE_NEG : 0u);
    out->w[pos >> 3] |= code << (4 * (pos & 7u));
    if (code) out->len = pos + 1;
  }
  return true;
}

struct KeLincombArgs {
  const AffineW* p0;  // m rows: P[i], or L[i]
  const AffineW* p1;  // m rows: R[i] (k == 2; never read when k == 1)
  AffineW* out;       // m rows
  uint32_t* flags;    // [0] the new key's flag word (FB_ANY_IDENTITY); [1] takes the same bit for an S or D that is the identity: not read
  uint32_t m, k;      // outputs; 1 (scale) or 2 (fold)
  KeDigits dig;       // codes KE_P1, KE_SUM, KE_DIFF only when k == 2
};
// grid = ceil(m / 256) blocks of 256 threads
template <int BF> NMX_KERNEL void NMX_LAUNCH_BOUNDS(256) k_key_lincomb(KeLincombArgs a) {
  NMX_LDS AffineW sd[2][kFbThreads];  // the lane's S and D rows, canonical, all zero for the identity (32 KiB)
  const uint32_t tid = NMX_TID, i = NMX_BID * kFbThreads + tid;  // i < m <= 2^31: every row read or written is row i of an m-row array
  const bool active = i < a.m;
  if (a.k == 2) {  // (uniform: a kernel argument)
    XYZZ<BF> s = XYZZ<BF>::identity(), d = XYZZ<BF>::identity();
    if (active) {
      const Affine<BF> P0 = Affine<BF>::load(a.p0[i]), P1 = Affine<BF>::load(a.p1[i]);
      s = XYZZ<BF>::from_affine(P0);
      s.add_affine(P1);
      d = XYZZ<BF>::from_affine(P0);
      d.add_affine(P1, true);
    }
    fb_block_affine<BF>(s, active, &sd[0][tid], a.flags + 1);
    fb_block_affine<BF>(d, active, &sd[1][tid], a.flags + 1);
  }
  XYZZ<BF> acc = XYZZ<BF>::identity();
  if (active) {
    for (int j = (int)a.dig.len - 1; j >= 0; j--) {  // len <= 256: inside dig.w
      acc.dbl_in_place();
      const uint32_t code = (a.dig.w[j >> 3] >> (4 * (j & 7))) & 15u, sel = code & 7u;
      if (!sel) continue;
      Affine<BF> q;  // (uniform branches: HBM and LDS loads stay apart)
      if (sel == KE_P0) q = Affine<BF>::load(a.p0[i]);
      else if (sel == KE_P1) q = Affine<BF>::load(a.p1[i]);
      else q = Affine<BF>::load(sd[sel == KE_SUM ? 0 : 1][tid]);
      acc.add_affine(q, (code & KE_NEG) != 0);
#ifdef NMX_BOUND_CHECKS
      acc.check();  // x < 5.3, y < 3.5, zz, zzz < 1.2
#endif
    }
  }
  fb_block_affine<BF>(acc, active, a.out + (active ? i : 0u), a.flags);
}

}  // namespace nmx
