// fixed_base.hpp -- key[i] = s_i * B for ONE base B, in HBM: nmx_bases_from_scalars (s_i from an array) and nmx_bases_setup_from_tau
// (s_i = tau^(begin + i): CommitmentKey::setup_from_rng -> setup_from_tau_direct / setup_from_tau_fixed_base_exp,
// /root/reference/src/provider/hyperkzg.rs:357-410, fixed_base_exp_comb_batch :443-).  Included by runtime.hpp; the kernels are instantiated by curve_impl.hpp (the four curve TUs).
// The kernels use block-level primitives only (LDS, barriers, one atomic OR), so tests/host_emul/fixed_base_emul.cpp runs the same bodies
// on the CPU (simt.hpp) with the limb bounds asserted (NMX_DEBUG_BOUNDS).
//
// Three steps, two launches:
//   window bases   P_w = 2^(c w) B, w < W = ceil(BITS / c): BITS doublings and W inversions on the HOST (fb_window_bases; ~0.2 ms), W x 64
//                  bytes up -- on the device they would be one lane's chain of 255 dependent doublings
//   k_fb_table     T[w][d - 1] = d P_w for d in [1, 2^c): one lane per entry, a c-bit double-and-add, then the block normalisation below.
//                  Affine, internal form, W (2^c - 1) x 64 bytes (c = 8: 510 KiB, inside one XCD's L2)
//   k_fb_mul       one lane per key point: the scalar as canonical words (from memory, or the product of the squarings tau^(2^j) that the
//                  bits of begin + i select, brought to canonical words), cut into W unsigned c-bit digits, one mixed addition per non-zero
//                  digit and NO doubling; then the block normalisation and one 64-byte store
// The block normalisation (fb_block_affine): one inversion per block of 256 lanes.  A product tree of the lanes' ZZZ through LDS (up-sweep),
// lane 0 inverts the root, the down-sweep hands every lane 1 / ZZZ_i:  y = Y / ZZZ, x = X / ZZ = X ZZ^2 / ZZZ^2 (ZZ^3 = ZZZ^2).  An identity
// lane (or one past the end) enters the product as 1 and writes the all-zero encoding.  Three tree products per lane and one inversion
// per block instead of one inversion per lane; no lane waits on another block.
//
// Digits are unsigned: d in [0, 2^c), the table holds every d > 0, so no carry runs between windows and a digit is c bits of the scalar.
// For a canonical scalar below r the partial sum never equals +- the entry added to it (both multiples stay below the prime order), but
// the additions are the complete XYZZ::add_affine_signed all the same.  Entries d 2^(c w) >= r of the top window are built (r is prime, so
// none is the identity) and never selected.
//
// Bounds (multiples of p): accumulators keep the XYZZ invariants of curve.hpp (x < 5.3, y < 3.5, zz, zzz < 1.2).  Tree nodes are products
// of operands < 1.2 or < 1.04: < 1 + 1.44 / 127 < 1.02; the root's inverse is < 2 (Fermat: a product; the host's Euclid: canonical); the
// down-sweep multiplies values < 2 by values < 1.02: < 1.02.  x = (X * ZZ^2) * iz^2: (5.3 * 1.02 -> 1.05) * 1.02 -> 1.01; y = Y * iz < 1.03;
// both then canon().  Scalars: a running product < 1.01 r times a canonical squaring.
#pragma once

#include "msm_partition.hpp"  // NMX_KERNEL / NMX_LDS / NMX_SYNC: the device / emulation spelling; funnel_shr

namespace nmx {

static constexpr uint32_t kFbThreads = 256;
static constexpr uint32_t kFbMinC = 4, kFbMaxC = 16, kFbDefaultC = 8;
static constexpr int kFbTauBits = 31;  // begin + i < 2^31
enum : uint32_t { FB_ERR_SCALAR_RANGE = 1u, FB_ANY_IDENTITY = 2u };  // bits of the flag word

NMX_HD uint32_t fb_windows(uint32_t bits, uint32_t c) { return (bits + c - 1) / c; }
NMX_HD uint32_t fb_entries(uint32_t c) { return (1u << c) - 1u; }  // per window

// P_w = 2^(c w) B for w < W, affine in the internal form (host; B internal, canonical, not the identity)
template <int BF> static inline void fb_window_bases(const Affine<BF>& B, uint32_t c, uint32_t W, AffineW* out) {
  XYZZ<BF> p = XYZZ<BF>::from_affine(B);
  for (uint32_t w = 0; w < W; w++) {
    p.to_affine().store(out[w]);  // (never the identity: 2^(c w) is not a multiple of the prime order)
    for (uint32_t b = 0; b < c && w + 1 < W; b++) p.dbl_in_place();
  }
}

// Every lane of the block calls this (lanes past the end with active = false).  Writes the affine form of acc to *slot: the all-zero
// encoding for the identity (and FB_ANY_IDENTITY into *flags), x || y canonical otherwise.
template <int BF> NMX_DEV void fb_block_affine(const XYZZ<BF>& acc, bool active, AffineW* slot, uint32_t* flags) {
  using F = Fp<BF>;
  NMX_LDS F t[2 * kFbThreads];  // node k = t[2 k] * t[2 k + 1]; leaves at [256, 512)
  const uint32_t tid = NMX_TID;
  const bool ident = !active || acc.is_identity();
  t[kFbThreads + tid] = ident ? F::one() : acc.zzz;
  NMX_SYNC();
  for (uint32_t half = kFbThreads / 2; half >= 1; half >>= 1) {  // up-sweep
    if (tid < half) {
      const uint32_t k = half + tid;
      t[k] = t[2 * k] * t[2 * k + 1];
    }
    NMX_SYNC();
  }
  if (tid == 0) t[1] = t[1].inv();
  NMX_SYNC();
  for (uint32_t half = 1; half < kFbThreads; half <<= 1) {  // down-sweep: node k holds the inverse of its product
    if (tid < half) {
      const uint32_t k = half + tid;
      const F i = t[k], a = t[2 * k], b = t[2 * k + 1];
      t[2 * k] = i * b;
      t[2 * k + 1] = i * a;
    }
    NMX_SYNC();
  }
  if (!active) return;
  if (ident) {
#pragma unroll
    for (int j = 0; j < 16; j++) slot->w[j] = 0u;
    nmx_atomic_or(flags, FB_ANY_IDENTITY);
    return;
  }
  const F iz = t[kFbThreads + tid];  // 1 / zzz
  iz.check_below(1.05, "fb_block_affine: 1 / zzz");
  Affine<BF> r;
  r.x = ((acc.x * acc.zz.sqr()) * iz.sqr()).canon();
  r.y = (acc.y * iz).canon();
  r.store(*slot);
}

// ---- the table ---------------------------------------------------------------------------------------------------------------------
struct FbTableArgs {
  const AffineW* win;  // W window bases
  AffineW* table;      // W x (2^c - 1)
  uint32_t* flags;
  uint32_t c, W;
};
// grid = ceil(W (2^c - 1) / 256) blocks of 256 threads
template <int BF> NMX_KERNEL void NMX_LAUNCH_BOUNDS(256) k_fb_table(FbTableArgs a) {
  const uint32_t M = fb_entries(a.c), total = a.W * M;  // <= 64 x 65535
  const uint32_t idx = NMX_BID * kFbThreads + NMX_TID;
  const bool active = idx < total;
  XYZZ<BF> acc = XYZZ<BF>::identity();
  if (active) {
    const uint32_t w = idx / M, d = idx % M + 1u;
    const Affine<BF> P = Affine<BF>::load(a.win[w]);
    for (int b = (int)a.c - 1; b >= 0; b--) {
      acc.dbl_in_place();
      if ((d >> b) & 1u) acc.add_affine_nonzero(P);
    }
  }
  fb_block_affine<BF>(acc, active, a.table + (active ? idx : 0u), a.flags);
}

// ---- the multiplication ----------------------------------------------------------------------------------------------------------------
template <int SF> struct FbMulArgs {
  const AffineW* table;
  const uint32_t* scalars;  // n x 8 words, or null: tau mode
  AffineW* out;             // n points
  uint32_t* flags;
  uint32_t n, c, W;
  uint32_t scalars_mont;
  uint32_t begin;               // tau mode: lane i computes tau^(begin + i)
  Fp<SF> sq[kFbTauBits];        // tau mode: tau^(2^j), internal form, canonical
};
// the squarings tau^(2^j), j < kFbTauBits, internal form and canonical (host); tau32: 32 bytes below r, Montgomery words when `mont`
template <int SF> static inline void fb_tau_squarings(const void* tau32, bool mont, Fp<SF>* sq) {
  using S = Fp<SF>;
  uint32_t tw[8];
  memcpy(tw, tau32, 32);
  S x = (mont ? S::from_words(tw).mont256_to_internal() : S::from_words(tw).to_internal()).canon();
  for (int j = 0; j < kFbTauBits; j++) {
    sq[j] = x;
    x = x.sqr().canon();
  }
}
// the lane's scalar as canonical words; false: not below r (the words are then zero)
template <int SF> NMX_DEV bool fb_scalar(const FbMulArgs<SF>& a, uint32_t i, uint32_t (&s)[8]) {
  using S = Fp<SF>;
  if (a.scalars) {
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] = a.scalars[8 * (size_t)i + j];
    if (!S::words_lt_p(s)) {
#pragma unroll
      for (int j = 0; j < 8; j++) s[j] = 0u;
      return false;
    }
    if (a.scalars_mont) S::from_words(s).mont256_to_canonical().to_words(s);
    return true;
  }
  const uint32_t e = a.begin + i;
  S acc = S::one();
  for (int j = 0; j < kFbTauBits; j++)
    if ((e >> j) & 1u) {
      acc = acc * a.sq[j];
      acc.check_below(1.02, "fb_scalar: running power of tau");
    }
  acc.to_canonical().to_words(s);
  return true;
}
// grid = ceil(n / 256) blocks of 256 threads
template <int BF, int SF> NMX_KERNEL void NMX_LAUNCH_BOUNDS(256) k_fb_mul(FbMulArgs<SF> a) {
  const uint32_t i = NMX_BID * kFbThreads + NMX_TID;
  const bool active = i < a.n;
  XYZZ<BF> acc = XYZZ<BF>::identity();
  if (active) {
    uint32_t s[8];
    if (!fb_scalar<SF>(a, i, s)) nmx_atomic_or(a.flags, FB_ERR_SCALAR_RANGE);
    const uint32_t c = a.c, mask = (1u << c) - 1u, M = mask;
    // the digit of window w is the low c bits of s >> (c w): the scalar is shifted down by c every window (seven funnel shifts with
    // constant register indices), never indexed by a run-time word number.  The next window's entry is loaded before this window's addition.
    auto take = [&]() {
      const uint32_t d = s[0] & mask;
#pragma unroll
      for (int j = 0; j < 7; j++) s[j] = funnel_shr(s[j + 1], s[j], c);
      s[7] >>= c;
      return d;
    };
    Affine<BF> cur, nxt;
    cur.x = cur.y = nxt.x = nxt.y = Fp<BF>::zero();
    uint32_t d = take();  // d < 2^c and w < W: the row read is always inside the table
    if (d) cur = Affine<BF>::load(a.table[d - 1u]);
    for (uint32_t w = 0; w < a.W; w++) {
      uint32_t dn = 0;
      if (w + 1 < a.W) {
        dn = take();
        if (dn) nxt = Affine<BF>::load(a.table[(size_t)(w + 1) * M + dn - 1u]);
      }
      if (d) acc.add_affine_nonzero(cur);
      cur = nxt;
      d = dn;
    }
  }
  fb_block_affine<BF>(acc, active, a.out + (active ? i : 0u), a.flags);
}

}  // namespace nmx
