// spmv_row.hpp -- the row primitive of the sparse-matrix kernels (one CSR row of M z, coefficient classes included), with the
// element load / store of the field-vector kernels.  Moved out of fieldvec.hip unchanged, so that a kernel header built on it
// (r1cs_eval.hpp) also compiles for the CPU under tests/host_emul; fieldvec.hip includes it first.
#pragma once

#include <cstddef>

#include "fp.hpp"

namespace nmx {

template <int FID> NMX_HD Fp<FID> ld(const uint32_t* p, size_t i) { return Fp<FID>::from_words(p + 8 * i); }
template <int FID> NMX_HD void st(uint32_t* p, size_t i, const Fp<FID>& v) { v.canon().to_words(p + 8 * i); }
// Operands whose formula needs them below p (subtrahends of sub2, factors of two weakly reduced operands), loaded with ld from words
// that may hold ANY 256-bit value (< 5.3 p): brought below p here.  A normalised v >= p has v.l[8] >= p's top limb, so ONE compare per
// operand and one branch per group decide; behind it every operand of the group is canonicalised (the identity on those already
// below p).  Canonical data -- the provers' -- almost never take the branch: its cost is N compares.
template <int FID, int N> NMX_HD void below_p(Fp<FID> (&v)[N]) {
  bool any = false;
#pragma unroll
  for (int j = 0; j < N; j++) any |= v[j].l[8] >= FpParams<FID>::P[8];
  if (any) {
#pragma unroll
    for (int j = 0; j < N; j++) v[j] = v[j].canon();
  }
}

// Coefficient classes, the GPU form of the reference's PrecomputedSparseMatrix (src/r1cs/sparse.rs:19-199: +-1 entries
// are added / subtracted, |k| <= 7 by repeated doubling, the rest multiplied).  R1CS matrices are almost all +-1: here
// the class rides in the top four bits of the 32-bit column index (columns < 2^28), so a unit or small entry costs
// 4 B of matrix traffic instead of 36 B and its 32-byte coefficient is never read -- SpMV is gather-bound, the saving
// is bytes, not multiplications.  Classes: 0 general, 1 +1, 2 -1, 3..8 +2..+7, 9..14 -2..-7.
static constexpr uint32_t kSpmvColBits = 28;
// what of an index word is the index, for a matrix whose gathered dimension has `extent` entries: the class bits are there only
// when the indices leave them room (otherwise every entry is class 0, general)
static inline uint32_t spmv_index_mask(size_t extent) { return extent <= ((size_t)1 << kSpmvColBits) ? (1u << kSpmvColBits) - 1u : 0xffffffffu; }

// coefficient class `cls` (>= 1) applied to z: a value < p, canonical.  z is any 256-bit value: it is reduced first (a
// z >= p -- the general Montgomery path reduces those correctly too -- would otherwise leave k z beyond canon()'s 16 p)
template <int FID> NMX_HD Fp<FID> spmv_small_term(uint32_t cls, const Fp<FID>& z_any) {
  using F = Fp<FID>;
  const uint32_t k = cls <= 2 ? 1u : (cls <= 8 ? cls - 1u : cls - 7u);  // |coefficient|
  const F zf = z_any.canon();                         // 2^256 < 6 p for all four fields
  F t;
#pragma unroll
  for (int i = 0; i < 9; i++) t.l[i] = zf.l[i] * k;  // z canonical: limbs < 2^29, k <= 7
  t = t.norm();                                       // value < 7 p
  if (cls == 2 || cls >= 9) t = F::sub8(F::zero(), t).norm();  // 8p - k z
  return t.canon();
}

// CSR sparse matrix x vector, one row per lane (src/r1cs/sparse.rs:201-229 multiply_vec).  Matrix values are stored in
// internal form at registration, so data * z comes out in z's own form with no correction.
// one row of M z, normalised (< 16 p: canon() brings it to the stored form)
template <int FID>
NMX_HD Fp<FID> spmv_row(const uint32_t* indptr, const uint32_t* indices, const uint32_t* data, const uint32_t* z, uint32_t colmask,
                        uint32_t row) {
  using F = Fp<FID>;
  F acc = F::zero();
  uint32_t pending = 0;
  for (uint32_t k = indptr[row]; k < indptr[row + 1]; k++) {
    const uint32_t w = indices[k], cls = (w & ~colmask) >> kSpmvColBits;
    const F zf = ld<FID>(z, w & colmask);
    acc = acc + (cls ? spmv_small_term<FID>(cls, zf) : ld<FID>(data, k) * zf);
    if (++pending == 6) {
      acc = acc.norm().canon();
      pending = 0;
    }
  }
  return acc.norm();
}

}  // namespace nmx
