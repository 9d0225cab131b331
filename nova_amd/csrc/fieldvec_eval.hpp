// fieldvec_eval.hpp -- what every opening argument goes through: the functors of the eq tables (EqStepFn, EqDirectFn, EqDirect2Fn,
// EqSplit2Fn, EqProductFn), the two passes of batch_invert (BatchInvFwdFn, BatchInvBwdFn) and the lane body of k_eval_multi
// (eval_multi_lane).  Moved out of fieldvec.hip and sumcheck.hip unchanged, so that tests/host_emul/eval_emul.cpp runs them on the CPU
// with the limb bounds asserted (NMX_DEBUG_BOUNDS); fieldvec.hip and sumcheck.hip include this header.
//
// Operand rule: a 32-byte word w of an input VECTOR (batch_invert's v, the coefficients of an evaluated polynomial) is ANY 256-bit
// value and stands for w mod p (2^256 < 5.3 p for BN254, < 4 p for Pasta); every output word is canonical (< p).  The constants made
// from a challenge or a point (r 2^261, (1 - r) 2^261, u 2^261, the power tables) are canonical: the call refuses a challenge >= p.
#pragma once

#include <stdint.h>

#include "spmv_row.hpp"  // ld / st

namespace nmx {

// EqPolynomial::evals_from_points, one doubling step (/root/reference/src/spartan/polys/eq.rs:54-73):
//   y = x[i] * r;  x[i + size] = y;  x[i] -= y        for i < size
template <int FID> struct EqStepFn {
  uint32_t* buf;
  Fp<FID> r;  // r * 2^261
  uint32_t size;
  NMX_HD void operator()(uint32_t i) const {
    using F = Fp<FID>;
    F x = ld<FID>(buf, i);
    F y = r * x;                                   // < 1.01 p
    st<FID>(buf, (size_t)i + size, y);
    st<FID>(buf, i, F::sub2(x, y).norm());         // x - y + 2p
  }
};

// Small eq tables in ONE launch: out[x] = prod_i (x_i ? r_i : 1 - r_i), x_0 the most significant bit, ell <= 12
// (the sqrt-size tables of evaluate_with: ell doubling launches are ~10 us each, this is one).  ell modmuls per entry
// instead of one -- irrelevant at <= 4096 entries.
template <int FID> struct EqDirectFn {
  static constexpr uint32_t kMaxEll = 12;
  uint32_t* out;
  Fp<FID> r[kMaxEll], nr[kMaxEll];  // r_i * 2^261 and (1 - r_i) * 2^261, canonical
  Fp<FID> one;                      // ONE in the vectors' form (1 or 2^256 mod p), as a plain residue
  uint32_t ell;
  NMX_HD void operator()(uint32_t x) const {
    Fp<FID> acc = one;
    for (uint32_t i = 0; i < ell; i++) acc = acc * (((x >> (ell - 1 - i)) & 1u) ? r[i] : nr[i]);
    st<FID>(out, x, acc);
  }
};

// Both sqrt-size tables of an evaluation (multilinear.rs:141-147) in ONE launch: lanes [0, 2^ellL) build the left table, the rest
// the right one (a 2^20 evaluation was four launches -- two tables, the pass, the final sum -- for 28 us; now two).
template <int FID> struct EqDirect2Fn {
  uint32_t *outL, *outR;
  Fp<FID> r[2 * EqDirectFn<FID>::kMaxEll], nr[2 * EqDirectFn<FID>::kMaxEll];  // left challenges, then the right ones
  Fp<FID> one;
  uint32_t ellL, ellR;
  NMX_HD void operator()(uint32_t g) const {
    const bool right = g >= (1u << ellL);
    const uint32_t x = right ? g - (1u << ellL) : g, ell = right ? ellR : ellL, o = right ? ellL : 0u;
    Fp<FID> acc = one;
    for (uint32_t i = 0; i < ell; i++) acc = acc * (((x >> (ell - 1 - i)) & 1u) ? r[o + i] : nr[o + i]);
    st<FID>(right ? outR : outL, x, acc);
  }
};

// batch_invert (src/spartan/mod.rs:54-118: Montgomery's trick, chunked over threads there).  Here a lane owns the STRIDED chunk
// {c, c + T, c + 2T, ...} of K elements (T = number of chunks: consecutive lanes touch consecutive elements), a forward pass
// leaves every element's prefix product in `out` and the chunk products in a vector that is inverted the same way one level up
// (the last level, <= 128 products, on the host: one extended-Euclid inversion), and a backward pass per level turns prefix
// products into inverses.  All products are taken on the stored words as they are (canonical or Montgomery): the form factor is
// a scale the top level applies once, and every lower level inherits it through the chunk inverses.
// Cost: 3 products per element at level 0 (the trick's minimum) + 3/K of that above it -- VALU-bound for long vectors (2^24:
// 52 ps per element = 3.1 products at the multiplier's ~58 G/s; the 160 B per element of traffic would take 20 ps), and a chain
// of 3K DEPENDENT products per level for short ones, which is why K shrinks with the level's size (binv_chunk).
// The words of v are ANY 256-bit values (< 5.3 p): they enter products only, whose other factor is below 1.01 p.
static constexpr uint32_t kBinvHostBelow = 128;
static inline uint32_t binv_chunk(size_t n) { return n >= (1u << 23) ? 32 : n >= (1u << 21) ? 16 : 8; }
template <int FID> struct BatchInvFwdFn {
  const uint32_t* v;
  uint32_t *prefix, *chunk_prod;
  uint32_t n, T, K;
  NMX_HD void operator()(uint32_t c) const {
    Fp<FID> acc = Fp<FID>::one();
    for (uint32_t j = 0; j < K; j++) {
      const uint64_t i = (uint64_t)c + (uint64_t)j * T;
      if (i >= n) break;
      st<FID>(prefix, i, acc);
      acc = acc * ld<FID>(v, i);
    }
    st<FID>(chunk_prod, c, acc);
  }
};
template <int FID> struct BatchInvBwdFn {
  const uint32_t *v, *chunk_inv;
  uint32_t* prefix;  // in: prefix products; out: the inverses
  uint32_t n, T, K;
  NMX_HD void operator()(uint32_t c) const {
    Fp<FID> acc = ld<FID>(chunk_inv, c);
    uint32_t cnt = 0;
    while (cnt < K && (uint64_t)c + (uint64_t)cnt * T < n) cnt++;
    for (uint32_t j = cnt; j-- > 0;) {
      const uint64_t i = (uint64_t)c + (uint64_t)j * T;
      const Fp<FID> p = ld<FID>(prefix, i), w = ld<FID>(v, i);
      st<FID>(prefix, i, acc * p);
      acc = (acc * w).canon();
    }
  }
};

// Large eq tables (13 <= ell <= 24) in TWO launches instead of ell doubling steps (a 2^20 table was 20 dependent launches,
// ~130 us, for 32 MB of output: profiles/r05_spartan): the sqrt-size tables of the two halves of the point -- the left one in the
// INTERNAL form, so that one product per entry gives out[x] = L[x >> ellR] * R[x & mask] in the vectors' own form -- and the
// product pass.  compute_eval_table_sparse's operand (src/spartan/snark.rs:182) is such a table.
template <int FID> struct EqSplit2Fn {
  uint32_t *outL, *outR;
  Fp<FID> r[2 * EqDirectFn<FID>::kMaxEll], nr[2 * EqDirectFn<FID>::kMaxEll];
  Fp<FID> oneL, oneR;
  uint32_t ellL, ellR;
  NMX_HD void operator()(uint32_t g) const {
    const bool right = g >= (1u << ellL);
    const uint32_t x = right ? g - (1u << ellL) : g, ell = right ? ellR : ellL, o = right ? ellL : 0u;
    Fp<FID> acc = right ? oneR : oneL;
    for (uint32_t i = 0; i < ell; i++) acc = acc * (((x >> (ell - 1 - i)) & 1u) ? r[o + i] : nr[o + i]);
    st<FID>(right ? outR : outL, x, acc);
  }
};
template <int FID> struct EqProductFn {
  const uint32_t *L, *R;
  uint32_t* out;
  uint32_t shift, mask;
  NMX_HD void operator()(uint32_t x) const { st<FID>(out, x, ld<FID>(L, x >> shift) * ld<FID>(R, x & mask)); }
};

// One lane of k_eval_multi (sumcheck.hip): the coefficients f[lo, hi) -- a chunk of at most kEvalChunk -- evaluated by Horner at the
// m <= kEvalMaxPts points pts[j] (internal form), each result scaled by the lane's power pw16[j * 256 + t] = u_j^(16 t) of the block's
// table; h[j] canonical on return (j < m; the others are left as they came).
static constexpr uint32_t kEvalChunk = 16, kEvalMaxPts = 4;
template <int FID>
NMX_HD void eval_multi_lane(const uint32_t* f, uint32_t lo, uint32_t hi, uint32_t m, const uint32_t* pts, const uint32_t* pw16, uint32_t t,
                            Fp<FID> (&h)[kEvalMaxPts]) {
  using F = Fp<FID>;
  F u[kEvalMaxPts];
#pragma unroll
  for (uint32_t j = 0; j < kEvalMaxPts; j++) u[j] = j < m ? ld<FID>(pts, j) : F::zero();
  for (uint32_t i = hi; i-- > lo;) {
    const F c = ld<FID>(f, i);
#pragma unroll
    for (uint32_t j = 0; j < kEvalMaxPts; j++)
      if (j < m) h[j] = (c + u[j] * h[j]).norm();                    // c any word (< 5.3 p) + a product (< 1.1 p): < 6.4 p, normalized
  }
#pragma unroll
  for (uint32_t j = 0; j < kEvalMaxPts; j++)
    if (j < m) h[j] = (h[j] * ld<FID>(pw16, (size_t)j * 256 + t)).canon();
}

}  // namespace nmx
