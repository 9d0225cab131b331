// fieldvec_maps.hpp -- the element-wise maps of the dense field-vector calls (one lane, one output element): the NIFS folds, the cross
// terms, the MLE bind / HyperKZG halving and the random linear combination.  Moved out of fieldvec.hip so that tests/host_emul runs
// them on the CPU with the limb bounds asserted (tests/host_emul/fieldvec_emul.cpp); fieldvec.hip includes this header first.
//
// Operand rule of every map here: a 32-byte word w of an input vector is ANY 256-bit value and stands for w mod p (2^256 < 5.3 p for
// BN254, < 4 p for Pasta); every output word is canonical (< p).  The challenge-derived constants are canonical, internal form.
#pragma once

#include <stdint.h>

#include "spmv_row.hpp"  // ld / st / below_p

namespace nmx {

template <int FID> struct AxpyFn {
  const uint32_t *a, *b;
  uint32_t* out;
  Fp<FID> r;  // r * 2^261, canonical
  NMX_HD void operator()(uint32_t i) const { st<FID>(out, i, (ld<FID>(a, i) + r * ld<FID>(b, i)).norm()); }
};
template <int FID> struct Axpy2Fn {
  const uint32_t *a, *b, *c;
  uint32_t* out;
  Fp<FID> r, r2;  // r * 2^261, r^2 * 2^261
  NMX_HD void operator()(uint32_t i) const {
    st<FID>(out, i, (ld<FID>(a, i) + Fp<FID>::mul_add(r, ld<FID>(b, i), r2, ld<FID>(c, i))).norm());  // one reduction for both products
  }
};
template <int FID> struct CrossTermFn {
  const uint32_t *az, *bz, *cz, *e;
  uint32_t* out;
  Fp<FID> u;  // (p - u) * 2^261: the product u*cz enters negated, so that az*bz*k - u*cz is ONE reduction (mul_add)
  Fp<FID> k;  // 2^522 / F: brings (az*F)(bz*F)/2^261 back to az*bz*F  (F = 1 canonical, 2^256 Montgomery)
  NMX_HD void operator()(uint32_t i) const {
    using F = Fp<FID>;
    F ab = ld<FID>(az, i) * ld<FID>(bz, i);              // words < 5.3 p: < 1.23 p
    F t = F::mul_add(ab, k, ld<FID>(cz, i), u);          // az bz k - u cz   < 1.06 p
    t = F::sub8(t, ld<FID>(e, i)).norm();                // - e + 8p   (e any word, < 5.3 p): < 9.1 p, canon() takes < 16 p
    st<FID>(out, i, t);
  }
};
// commit_T_relaxed's term (src/r1cs/mod.rs:652-659): az*bz - u*cz - e1 - e2, both error vectors in the one pass
template <int FID> struct CrossTerm2Fn {
  const uint32_t *az, *bz, *cz, *e1, *e2;
  uint32_t* out;
  Fp<FID> u, k;  // as CrossTermFn (u negated)
  NMX_HD void operator()(uint32_t i) const {
    using F = Fp<FID>;
    F ab = ld<FID>(az, i) * ld<FID>(bz, i);              // words < 5.3 p: < 1.23 p
    F t = F::mul_add(ab, k, ld<FID>(cz, i), u);          // az bz k - u cz          < 1.06 p
    // e1 + e2 of two arbitrary words (< 10.6 p) is beyond every subtraction constant: each is brought below p first
    F ee[2] = {ld<FID>(e1, i), ld<FID>(e2, i)};
    below_p<FID, 2>(ee);
    F es = (ee[0] + ee[1]).norm();                       // < 2 p
    t = F::sub4(t, es).norm();                           // - (e1 + e2) + 4p        < 5.1 p  (canon() takes < 16 p)
    st<FID>(out, i, t);
  }
};
template <int FID> struct VecAddFn {
  const uint32_t *a, *b;
  uint32_t* out;
  NMX_HD void operator()(uint32_t i) const { st<FID>(out, i, (ld<FID>(a, i) + ld<FID>(b, i)).norm()); }
};
template <int FID> struct BindTopFn {
  const uint32_t *lo, *hi;  // element i of each, `stride` elements apart
  uint32_t* out;
  Fp<FID> r;  // r * 2^261
  uint32_t stride;
  NMX_HD void operator()(uint32_t i) const {
    using F = Fp<FID>;
    F l = ld<FID>(lo, (size_t)i * stride), h = ld<FID>(hi, (size_t)i * stride);
    st<FID>(out, i, (l + r * F::sub8(h, l).norm()).norm());  // l, h any words (< 5.3 p): h - l + 8p < 13.3 p, sum < 6.5 p
  }
};

// NIFS fold in one launch (src/r1cs/mod.rs:1058-1067): W = W1 + r W2 over n_w elements, E = E1 + r T over n_e
template <int FID> struct FoldPairFn {
  const uint32_t *w1, *w2, *e1, *t;
  uint32_t *w, *e;
  uint32_t n_w;
  Fp<FID> r;
  NMX_HD void operator()(uint32_t i) const {
    if (i < n_w) st<FID>(w, i, (ld<FID>(w1, i) + r * ld<FID>(w2, i)).norm());
    else st<FID>(e, i - n_w, (ld<FID>(e1, i - n_w) + r * ld<FID>(t, i - n_w)).norm());
  }
};

// out[i] = sum_j w[j] * v_j[i], vectors shorter than the output read as zero-padded: PolyEvalWitness::batch and
// batch_diff_size with w[j] = s^j (/root/reference/src/spartan/mod.rs:165-277), the random linear combination in
// front of the batched PCS opening.  (k + 1) x 32 B per element against k modmuls: HBM-bound for every k.
template <int FID> struct LinCombFn {
  const uint64_t* vecs;  // k device addresses
  const uint64_t* lens;  // k element counts
  const uint32_t* w;     // k x 8, internal form (s^j * 2^261), canonical
  uint32_t* out;
  uint32_t k;
  NMX_HD void operator()(uint32_t i) const {
    using F = Fp<FID>;
    // four products under one reduction (Fp::dot: 4 x 81 + 81 multiply-adds instead of 4 x 162; the weights are wave-uniform):
    // the kernel was multiplier-bound at k = 8 (329 us at 2^22 against a VALU floor of 314 us, profiles/r03_fieldvec/lincomb8_pmc.json)
    F acc = F::zero();
    uint32_t pending = 0;
    for (uint32_t j = 0; j < k; j += 4) {
      F v[4], c[4];
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        const bool on = j + q < k && i < lens[j + q < k ? j + q : j];
        v[q] = on ? ld<FID>((const uint32_t*)(uintptr_t)vecs[j + q], i) : F::zero();
        c[q] = j + q < k ? ld<FID>(w, j + q) : F::zero();
      }
      acc = acc + F::template dot<4, true>(v, c);  // < 1.04 p each
      if (++pending == 6) {
        acc = acc.norm().canon();
        pending = 0;
      }
    }
    st<FID>(out, i, acc.norm());
  }
};

}  // namespace nmx
