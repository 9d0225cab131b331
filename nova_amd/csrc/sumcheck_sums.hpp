// sumcheck_sums.hpp -- the lane bodies of the three sum passes of sumcheck.hip: what ONE lane of k_eq_sums / k_eq_rows, k_bind_eq_sums
// and k_plain_sums adds up (and, for the bind pass, writes), given its first index, its stride and the grid geometry.  The __global__
// shells in sumcheck.hip call these and reduce over the block; tests/host_emul/fieldvec_emul.cpp calls them lane by lane on the CPU with
// the limb bounds asserted (NMX_DEBUG_BOUNDS).  sumcheck.hip includes this header first.
//
// Operand rule of the three calls built on these bodies (nmx_sumcheck_eq_sums, nmx_sumcheck_bind_eq_sums, nmx_sumcheck_plain_sums): a
// 32-byte word w of a table or an eq table is ANY 256-bit value and stands for w mod p (2^256 < 5.3 p); the sums and the bound
// tables come out canonical.  The table operands that enter a difference (x1 - x0, 2 x0 - x1) go through below_p; the eq factors,
// c0 and mode 1's a0 enter products only, whose bounds hold for words up to 5.3 p (stated at each formula).
#pragma once

#include <stdint.h>

#include "spmv_row.hpp"  // below_p

namespace nmx {

template <int FID> NMX_HD Fp<FID> ldw(const uint32_t* p, size_t i) {
  return Fp<FID>::from_words(p + 8 * i);
}

// The terms of one index: e0 = a0*b0 - c0 (at product scale) and q = (a1-a0)*(b1-b0), with the eq factor.
template <int FID, int MODE> struct EqTerm {
  Fp<FID> e0, q, fac;
};
template <int FID, int MODE>
NMX_HD EqTerm<FID, MODE> eq_term(const uint32_t* A, const uint32_t* B, const uint32_t* C,
                                 const uint32_t* eqL, const uint32_t* eqR, uint32_t shift,
                                 uint32_t mask, uint32_t h, const Fp<FID>& nk, uint32_t id,
                                 uint32_t eq_index = 0xffffffffu) {
  using F = Fp<FID>;
  EqTerm<FID, MODE> t;
  // eq_index given (k_eq_rows): the factor is eqR[eq_index] alone, eqL is applied once per row by the caller
  t.fac = ldw<FID>(eqR, eq_index != 0xffffffffu ? eq_index : (eqL ? (id & mask) : id));
  if (eqL) t.fac = ldw<FID>(eqL, id >> shift) * t.fac;
  if (MODE == 1) {
    t.e0 = ldw<FID>(A, id);  // any word, < 5.3 p: a term e0 * fac (two per reduction; four in k_eq_rows) stays below 127 p^2
    t.q = F::zero();
  } else {
    // below p: they enter the differences, and the bound of e0 below assumes it
    F x[4] = {ldw<FID>(A, id), ldw<FID>(A, (size_t)id + h), ldw<FID>(B, id), ldw<FID>(B, (size_t)id + h)};
    below_p<FID, 4>(x);
    const F a0 = x[0], a1 = x[1], b0 = x[2], b1 = x[3];
    // a0*b0 - c0*k in ONE reduction: nk = p - k (k brings c0 to the scale of a product; MODE 2: c0 = 1 folded into nk)
    t.e0 = MODE == 3 ? F::mul_add(a0, b0, ldw<FID>(C, id), nk) : (a0 * b0 + nk).norm();   // < 1.05 p (c0 < 5.3 p) / < 2.01 p
    t.q = F::sub2(a1, a0).norm() * F::sub2(b1, b0).norm();                                 // operands < 3 p
  }
  return t;
}

// one lane of k_eq_sums: indices first, first + stride, ... below h; s0, s1 canonical on return
template <int FID, int MODE>
NMX_HD void eq_sums_lane(const uint32_t* A, const uint32_t* B, const uint32_t* C, const uint32_t* eqL, const uint32_t* eqR,
                         uint32_t shift, uint32_t mask, uint32_t h, const Fp<FID>& nk, uint32_t first, uint32_t stride,
                         Fp<FID>& s0, Fp<FID>& s1) {
  using F = Fp<FID>;
  s0 = F::zero(), s1 = F::zero();
  uint32_t pending = 0;  // lazily added terms since the last canonicalisation (each < 1.1 p, limbs < 2^29)
  uint32_t id = first;
  // two indices per iteration: s += e_i * f_i + e_j * f_j is one reduction for two products
  for (; id + stride < h; id += 2 * stride) {
    const EqTerm<FID, MODE> x = eq_term<FID, MODE>(A, B, C, eqL, eqR, shift, mask, h, nk, id);
    const EqTerm<FID, MODE> y = eq_term<FID, MODE>(A, B, C, eqL, eqR, shift, mask, h, nk, id + stride);
    s0 = s0 + F::mul_add(x.e0, x.fac, y.e0, y.fac);            // < p (1 + 2 * 2.1 * 1.1 / 127)
    if (MODE != 1) s1 = s1 + F::mul_add(x.q, x.fac, y.q, y.fac);
    if (++pending == 6) {  // 1 canonical + 6 fresh terms: value < 8 p, limbs < 7 * 2^29 -- then back to < p
      s0 = s0.norm().canon();
      s1 = s1.norm().canon();
      pending = 0;
    }
  }
  if (id < h) {
    const EqTerm<FID, MODE> x = eq_term<FID, MODE>(A, B, C, eqL, eqR, shift, mask, h, nk, id);
    s0 = s0 + x.e0 * x.fac;
    if (MODE != 1) s1 = s1 + x.q * x.fac;
  }
  s0 = s0.norm().canon();
  s1 = s1.norm().canon();
}

// one lane of k_eq_rows: thread t of block `block` out of `nblocks`; g0, g1 canonical on return
template <int FID, int MODE>
NMX_HD void eq_rows_lane(const uint32_t* A, const uint32_t* B, const uint32_t* C, const uint32_t* eqL, const uint32_t* eqR,
                         uint32_t shift, uint32_t h, const Fp<FID>& nk, uint32_t t, uint32_t block, uint32_t nblocks,
                         Fp<FID>& g0, Fp<FID>& g1) {
  using F = Fp<FID>;
  const uint32_t row = 1u << shift, P = row < 256u ? row : 256u, rows_per_block = 256u / P, K = row / P;
  const uint32_t lo0 = t % P, sub = t / P;
  const uint32_t nrows = (uint32_t)(((uint64_t)h + row - 1) >> shift);
  g0 = F::zero(), g1 = F::zero();
  uint32_t pend_g = 0;
  for (uint32_t hi = block * rows_per_block + sub; hi < nrows; hi += nblocks * rows_per_block) {
    const uint32_t base = hi << shift;
    F r0 = F::zero(), r1 = F::zero();
    uint32_t pend = 0, k = 0;
    // mode 1 (evaluate_with): four indices per reduction (Fp::dot), whole groups inside the vector.  (Modes 2 / 3 would hold
    // twelve operands -- 221 registers, two waves per SIMD -- for 6 % fewer multiply-adds: they keep the pairs below.)
    if constexpr (MODE == 1) {
      for (; k + 3 < K; k += 4) {
        const uint32_t l0 = lo0 + k * P;
        if (base + l0 + 3 * P >= h) break;
        F e[4], fc[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
          e[j] = ldw<FID>(A, base + l0 + j * P);
          fc[j] = ldw<FID>(eqR, l0 + j * P);
        }
        r0 = r0 + F::template dot<4>(e, fc);  // < 1.04 p
        if (++pend == 6) {
          r0 = r0.norm().canon();
          pend = 0;
        }
      }
    }
    for (; k + 1 < K; k += 2) {  // two indices per reduction
      const uint32_t l0 = lo0 + k * P, l1 = l0 + P;
      if (base + l1 < h) {
        const EqTerm<FID, MODE> x = eq_term<FID, MODE>(A, B, C, nullptr, eqR, 0, 0, h, nk, base + l0, l0);
        const EqTerm<FID, MODE> y = eq_term<FID, MODE>(A, B, C, nullptr, eqR, 0, 0, h, nk, base + l1, l1);
        r0 = r0 + F::mul_add(x.e0, x.fac, y.e0, y.fac);
        if (MODE != 1) r1 = r1 + F::mul_add(x.q, x.fac, y.q, y.fac);
      } else if (base + l0 < h) {
        const EqTerm<FID, MODE> x = eq_term<FID, MODE>(A, B, C, nullptr, eqR, 0, 0, h, nk, base + l0, l0);
        r0 = r0 + x.e0 * x.fac;
        if (MODE != 1) r1 = r1 + x.q * x.fac;
      }
      if (++pend == 6) {
        r0 = r0.norm().canon();
        r1 = r1.norm().canon();
        pend = 0;
      }
    }
    if (k < K) {
      const uint32_t l0 = lo0 + k * P;
      if (base + l0 < h) {
        const EqTerm<FID, MODE> x = eq_term<FID, MODE>(A, B, C, nullptr, eqR, 0, 0, h, nk, base + l0, l0);
        r0 = r0 + x.e0 * x.fac;
        if (MODE != 1) r1 = r1 + x.q * x.fac;
      }
    }
    const F el = ldw<FID>(eqL, hi);
    g0 = g0 + r0.norm().canon() * el;
    if (MODE != 1) g1 = g1 + r1.norm().canon() * el;
    if (++pend_g == 6) {
      g0 = g0.norm().canon();
      g1 = g1.norm().canon();
      pend_g = 0;
    }
  }
  g0 = g0.norm().canon();
  g1 = g1.norm().canon();
}

// X[id], X[id + hq] bound with r from X[id + 2 hq], X[id + 3 hq]: written to oX and returned canonical
template <int FID>
NMX_HD void bind_eq_bind2(const uint32_t* X, uint32_t* oX, uint32_t id, uint32_t hq, const Fp<FID>& r, Fp<FID>& y0, Fp<FID>& y1) {
  using F = Fp<FID>;
  const F x00 = ldw<FID>(X, id), x01 = ldw<FID>(X, (size_t)id + hq);
  const F x10 = ldw<FID>(X, (size_t)id + 2 * (size_t)hq), x11 = ldw<FID>(X, (size_t)id + 3 * (size_t)hq);
  y0 = (x00 + r * F::sub8(x10, x00).norm()).norm().canon();   // lo + r * (hi - lo), as BindTopFn: any words, < 6.5 p
  y1 = (x01 + r * F::sub8(x11, x01).norm()).norm().canon();
  y0.to_words(oX + 8 * (size_t)id);
  y1.to_words(oX + 8 * ((size_t)id + hq));
}

// one lane of k_bind_eq_sums: binds its indices (first, first + stride, ... below hq) and adds the next round's terms; s0, s1
// canonical on return
template <int FID, int MODE>
NMX_HD void bind_eq_sums_lane(const uint32_t* A, const uint32_t* B, const uint32_t* C, uint32_t* oA, uint32_t* oB, uint32_t* oC,
                              const Fp<FID>& r, const uint32_t* eqL, const uint32_t* eqR, uint32_t shift, uint32_t mask, uint32_t hq,
                              const Fp<FID>& nk, uint32_t first, uint32_t stride, Fp<FID>& s0, Fp<FID>& s1) {
  using F = Fp<FID>;
  s0 = F::zero(), s1 = F::zero();
  uint32_t pending = 0;
  for (uint32_t id = first; id < hq; id += stride) {
    F a0, a1, b0, b1, c0, c1;
    bind_eq_bind2<FID>(A, oA, id, hq, r, a0, a1);
    if (MODE >= 2) bind_eq_bind2<FID>(B, oB, id, hq, r, b0, b1);
    if (MODE == 3) bind_eq_bind2<FID>(C, oC, id, hq, r, c0, c1);
    F fac = ldw<FID>(eqR, eqL ? (id & mask) : id);
    if (eqL) fac = ldw<FID>(eqL, id >> shift) * fac;
    if (MODE == 1) {
      s0 = s0 + a0 * fac;
    } else {
      const F e0 = MODE == 3 ? F::mul_add(a0, b0, c0, nk) : (a0 * b0 + nk).norm();  // a0*b0 - c0*k, one reduction
      const F q = F::sub2(a1, a0).norm() * F::sub2(b1, b0).norm();
      s0 = s0 + e0 * fac;
      s1 = s1 + q * fac;
    }
    if (++pending == 6) {
      s0 = s0.norm().canon();
      s1 = s1.norm().canon();
      pending = 0;
    }
  }
  s0 = s0.norm().canon();
  s1 = s1.norm().canon();
}

// one lane of k_plain_sums: indices first, first + stride, ... below h; s0, s1, s2 canonical on return (s2: kind 4 only, else zero)
template <int FID, int KIND>
NMX_HD void plain_sums_lane(const uint32_t* A, const uint32_t* B, const uint32_t* C, uint32_t h, uint32_t first, uint32_t stride,
                            Fp<FID>& s0, Fp<FID>& s1, Fp<FID>& s2) {
  using F = Fp<FID>;
  s0 = F::zero(), s1 = F::zero(), s2 = F::zero();
  uint32_t pending = 0;
  uint32_t id = first;
  if constexpr (KIND == 1 || KIND == 3) {
    // two indices per reduction (mul_add: 2 x 81 + 81 multiply-adds instead of 2 x 162)
    for (; (uint64_t)id + stride < h; id += 2 * stride) {
      const uint32_t jd = id + stride;
      F x[8] = {ldw<FID>(A, id), ldw<FID>(A, (size_t)id + h), ldw<FID>(B, id), ldw<FID>(B, (size_t)id + h),
                ldw<FID>(A, jd), ldw<FID>(A, (size_t)jd + h), ldw<FID>(B, jd), ldw<FID>(B, (size_t)jd + h)};
      below_p<FID, 8>(x);  // every operand enters a difference
      const F a0 = x[0], a1 = x[1], b0 = x[2], b1 = x[3], c0 = x[4], c1 = x[5], d0 = x[6], d1 = x[7];
      s0 = s0 + F::mul_add(a0, b0, c0, d0);
      if (KIND == 1)
        s1 = s1 + F::mul_add(F::sub2(a1, a0).norm(), F::sub2(b1, b0).norm(), F::sub2(c1, c0).norm(), F::sub2(d1, d0).norm());  // operands < 3 p -> < 1.15 p
      else
        s1 = s1 + F::mul_add(F::sub2(a0.dbl(), a1).norm(), F::sub2(b0.dbl(), b1).norm(), F::sub2(c0.dbl(), c1).norm(),
                             F::sub2(d0.dbl(), d1).norm());  // operands < 4 p -> < 1.26 p
      if (++pending == 6) {
        s0 = s0.norm().canon();
        s1 = s1.norm().canon();
        pending = 0;
      }
    }
  }
  for (; id < h; id += stride) {
    F x[4] = {ldw<FID>(A, id), ldw<FID>(A, (size_t)id + h), ldw<FID>(B, id), ldw<FID>(B, (size_t)id + h)};
    below_p<FID, 4>(x);  // every operand enters a difference
    const F a0 = x[0], a1 = x[1], b0 = x[2], b1 = x[3];
    if (KIND == 1) {
      s0 = s0 + a0 * b0;
      s1 = s1 + F::sub2(a1, a0).norm() * F::sub2(b1, b0).norm();          // operands < 3 p -> < 1.08 p
    } else if (KIND == 2) {
      s0 = s0 + F::sub2(a0, b0);                                          // < 3 p
      // the subtrahend 2 b0 - b1 + 2p reaches 4p - 2 (b0 = p - 1, b1 = 0), beyond the 4p - 2^233 that sub4 takes: sub8.  < 4p + 8p
      s1 = s1 + F::sub8(F::sub2(a0.dbl(), a1).norm(), F::sub2(b0.dbl(), b1).norm());
    } else if (KIND == 3) {
      s0 = s0 + a0 * b0;
      s1 = s1 + F::sub2(a0.dbl(), a1).norm() * F::sub2(b0.dbl(), b1).norm();  // operands < 4 p -> < 1.13 p
    } else {
      F y[2] = {ldw<FID>(C, id), ldw<FID>(C, (size_t)id + h)};
      below_p<FID, 2>(y);
      const F c0 = y[0], c1 = y[1];
      s0 = s0 + (a0 * b0) * c0;
      s1 = s1 + (F::sub2(a1, a0).norm() * F::sub2(b1, b0).norm()) * F::sub2(c1, c0).norm();
      s2 = s2 + (F::sub2(a0.dbl(), a1).norm() * F::sub2(b0.dbl(), b1).norm()) * F::sub2(c0.dbl(), c1).norm();
    }
    // kind 2 adds up to 12 p per term to a canonical sum (< 13 p, limbs < 2^31): canonicalise every term; products add < 1.2 p
    // (limbs < 2^29)
    if (KIND == 2 || ++pending == 6) {
      s0 = s0.norm().canon();
      s1 = s1.norm().canon();
      if (KIND == 4) s2 = s2.norm().canon();
      pending = 0;
    }
  }
  s0 = s0.norm().canon();
  s1 = s1.norm().canon();
  if (KIND == 4) s2 = s2.norm().canon();
}

}  // namespace nmx
