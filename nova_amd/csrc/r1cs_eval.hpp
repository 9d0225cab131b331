// r1cs_eval.hpp -- the verifier's matrix evaluations (RelaxedR1CSSNARK::verify's multi_evaluate,
// src/spartan/snark.rs:325-353 of the reference):
//     evals[m] = sum over every entry (row, col, val) of M_m :  T_x[row] * T_y[col] * val,     m < k <= 8
//     T_x = EqPolynomial::evals_from_points(r_x),  T_y = EqPolynomial::evals_from_points(r_y)
// for k matrices resident as CSR (nmx_spmv_register) in ONE launch plus a one-block-per-matrix finish.  Included at the end of
// fieldvec.hip; the lane body has no wave-level intrinsic, so tests/host_emul runs it on the CPU (simt.hpp).
//
// A lane walks the rows of its matrix with a grid stride.  Per row:
//     rv  = spmv_row(indptr, indices, data, T_y, colmask, row)          the existing row primitive, coefficient classes included
//     t_x = xL[row >> sx] * xR[row & (2^sx - 1)]                        T_x is NEVER materialised: two sqrt-size tables
//     acc += t_x * rv
// Forms.  xL and xR both hold the INTERNAL form (e 2^261), so their product (a b / 2^261) is T_x[row] in the internal form again and
// t_x * rv is T_x[row] (M T_y)[row] in whatever form T_y is in -- the caller's (canonical, or Montgomery with NMX_SCALARS_MONT).
// Nothing is corrected afterwards: the canonical sum IS the result in the ABI form.  The variables of r_x / r_y above the bits that
// rows / cols need contribute the constant prod (1 - r_i) (the index bit is 0 for every row / column that exists); the host folds
// both constants into xL's starting value.  Rows >= rows of a matrix are never visited.
//
// Bounds (p = the modulus; a product of operands below a p and b p with a b < 127 is normalised and below p (1 + a b / 127)):
//   xL, xR     stored canonical (st() canonicalises): < p;        t_x = xL * xR < 1.01 p, limbs < 2^29
//   rv         spmv_row's return: normalised, < 16 p (its own cadence: a canonical accumulator and at most six terms below 2 p)
//   t_x * rv   16.2 p^2 < 127 p^2: normalised, < 1.13 p
//   acc        canonical (< p) plus at most six such terms: value < 7.8 p < 16 p, limbs < 7 * 2^29 < 2^32 -> norm(), canon()
//              (the cadence of spmv_row and k_spmv_heavy); the lane's result is canonical.
// Reduction (k_r1cs_eval): the 64 canonical lane sums of a wave are added limbwise through shuffles (normalised every second step,
// < 64 p < 2^261), one product with ONE brings the wave's sum below 2 p and canon4() makes it canonical; the four wave sums meet in
// LDS (< 4 p -> canon()).  A block stores ONE canonical partial per launch -- its matrix's -- and k_r1cs_eval_finish, one block per
// matrix behind the pass, adds the partials the same way.  Field addition is exact and every stored value is the canonical
// representative, so the result does not depend on the grid or on the order of the additions.  No atomics.
//
// T_y is a full table in workspace (eq_evals_t, shared by the k matrices), gathered by column like z in every other SpMV kernel.
// The alternative -- the split form T_y[col] = yL[col >> s] * yR[col & mask]: two L2-resident tables and one more product per entry
// instead of a 32-byte gather -- has not been timed against this one yet: docs/measurements.md.
#pragma once

#include "msm_partition.hpp"  // NMX_DEV, NMX_TID: the device / emulation spellings
#include "spmv_row.hpp"

namespace nmx {

static constexpr uint32_t kR1csEvalMaxMats = 8, kR1csEvalMaxBlocks = 1024;  // blocks PER MATRIX (the finish reads that many partials)

struct R1csEvalArgs {
  const uint32_t* indptr[kR1csEvalMaxMats];
  const uint32_t* indices[kR1csEvalMaxMats];
  const uint32_t* data[kR1csEvalMaxMats];
  uint32_t rows[kR1csEvalMaxMats], colmask[kR1csEvalMaxMats];
  const uint32_t *xL, *xR;  // 2^(effx - sx) and 2^sx entries, internal form, canonical
  const uint32_t* ty;       // T_y over the columns that exist (2^effy entries), in the vectors' form
  uint32_t* partial;        // k * bpm elements: [matrix][block]
  uint32_t sx;              // bits of the right half of T_x
  uint32_t bpm;             // blocks per matrix; the grid is k * bpm blocks of 256
};

// the lane's share of matrix m: rows blk * 256 + tid, + bpm * 256, ...; canonical
template <int FID> NMX_DEV Fp<FID> r1cs_eval_lane(const R1csEvalArgs& a, uint32_t m, uint32_t blk) {
  using F = Fp<FID>;
  const uint32_t rows = a.rows[m], colmask = a.colmask[m], xmask = (1u << a.sx) - 1u;
  const uint32_t *ip = a.indptr[m], *ix = a.indices[m], *dt = a.data[m];
  F acc = F::zero();
  uint32_t pending = 0;
  for (uint64_t r = (uint64_t)blk * 256u + NMX_TID; r < rows; r += (uint64_t)a.bpm * 256u) {
    const uint32_t row = (uint32_t)r;
    const F rv = spmv_row<FID>(ip, ix, dt, a.ty, colmask, row);                           // < 16 p
    const F tx = ld<FID>(a.xL, row >> a.sx) * ld<FID>(a.xR, row & xmask);                 // < 1.01 p
    acc = acc + tx * rv;                                                                   // + (< 1.13 p)
    if (++pending == 6) {
      acc = acc.norm().canon();
      pending = 0;
    }
  }
  return acc.norm().canon();
}

// blocks per matrix for the longest of the matrices
static inline uint32_t r1cs_eval_blocks(size_t max_rows) {
  const size_t b = (max_rows + 255) / 256;
  return (uint32_t)(b < 1 ? 1 : (b < kR1csEvalMaxBlocks ? b : kR1csEvalMaxBlocks));
}

#if defined(__HIPCC__) || defined(__HIP__)
// sum of the block's 256 canonical values, canonical, valid in thread 0.  lds: 36 words.
template <int FID> __device__ __forceinline__ Fp<FID> r1cs_eval_block_sum(Fp<FID> x, uint32_t* lds) {
  using F = Fp<FID>;
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
#pragma unroll
  for (uint32_t d = 32; d >= 1; d >>= 1) {
#pragma unroll
    for (int i = 0; i < 9; i++) x.l[i] += (uint32_t)__shfl_down((int)x.l[i], d, 64);
    if (d == 16 || d == 4 || d == 1) x = x.norm();  // limbs < 4 * 2^29 between two normalisations
  }
  x = (x * F::one()).canon4();  // lane 0: < 64 p -> < 1.51 p -> canonical
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 9; i++) lds[i * 4 + wave] = x.l[i];
  }
  __syncthreads();
  F acc = F::zero();
  if (t == 0) {
#pragma unroll
    for (int w = 0; w < 4; w++) {
      F o;
#pragma unroll
      for (int i = 0; i < 9; i++) o.l[i] = lds[i * 4 + w];
      acc = acc + o;
    }
    acc = acc.norm().canon();  // < 4 p
  }
  return acc;
}

template <int FID> __global__ __launch_bounds__(256) void k_r1cs_eval(R1csEvalArgs a) {
  __shared__ uint32_t lds[36];
  const uint32_t m = blockIdx.x / a.bpm, blk = blockIdx.x - m * a.bpm;  // (uniform: every wave of a block works on one matrix)
  const Fp<FID> s = r1cs_eval_block_sum<FID>(r1cs_eval_lane<FID>(a, m, blk), lds);
  if (threadIdx.x == 0) s.to_words(a.partial + 8 * (size_t)blockIdx.x);
}

// one block per matrix: out[m] = sum of its bpm partials (canonical in, canonical out)
template <int FID> __global__ __launch_bounds__(256) void k_r1cs_eval_finish(const uint32_t* partial, uint32_t bpm, uint32_t* out) {
  using F = Fp<FID>;
  __shared__ uint32_t lds[36];
  // a thread adds at most four partials: canonical values, limbs < 4 * 2^29, the sum < 4 p -- no intermediate reduction is needed
  static_assert(kR1csEvalMaxBlocks <= 4 * 256, "k_r1cs_eval_finish adds at most four canonical partials per thread before norm()");
  F acc = F::zero();
  for (uint32_t i = threadIdx.x; i < bpm; i += 256u) acc = acc + ld<FID>(partial, (size_t)blockIdx.x * bpm + i);
  const F s = r1cs_eval_block_sum<FID>(acc.norm().canon(), lds);
  if (threadIdx.x == 0) s.to_words(out + 8 * (size_t)blockIdx.x);
}

// smallest e with 2^e >= n (0 for n <= 1)
static inline uint32_t r1cs_eval_bits(size_t n) {
  uint32_t e = 0;
  while (((size_t)1 << e) < n) e++;
  return e;
}

template <int FID>
static void r1cs_eval_t(Ctx& c, const CsrView* it, size_t k, const void* r_x, uint32_t ell_x, const void* r_y, uint32_t ell_y,
                        uint32_t flags, uint8_t* out) {
  using F = Fp<FID>;
  const bool mont = flags & NMX_SCALARS_MONT;
  constexpr uint32_t kMax = EqDirectFn<FID>::kMaxEll;
  size_t max_rows = 0, max_cols = 0;
  for (size_t j = 0; j < k; j++) {
    max_rows = it[j].rows > max_rows ? it[j].rows : max_rows;
    max_cols = it[j].cols > max_cols ? it[j].cols : max_cols;
  }
  // the bits that rows / columns which exist can set; the variables above them see a 0 bit everywhere: the factor prod (1 - r_i)
  const uint32_t effx = r1cs_eval_bits(max_rows), effy = r1cs_eval_bits(max_cols), topx = ell_x - effx, topy = ell_y - effy;
  require(effx <= 2 * kMax, NMX_E_TOO_LARGE, "nmx_r1cs_evaluate: more than 2^24 rows");
  // every point is range-checked (challenge(): NMX_E_SCALAR_RANGE, as nmx_eq_evals_from_points) before anything is enqueued
  const F one_i = F::one();
  F top = one_i;
  std::vector<F> rx(effx), nrx(effx);
  for (uint32_t i = 0; i < ell_x; i++) {
    const F r = challenge<FID>((const uint8_t*)r_x + 32 * (size_t)i, mont), nr = F::sub2(one_i, r).norm().canon();
    if (i < topx) top = (top * nr).canon();
    else rx[i - topx] = r, nrx[i - topx] = nr;
  }
  for (uint32_t i = 0; i < ell_y; i++) {
    const F r = challenge<FID>((const uint8_t*)r_y + 32 * (size_t)i, mont);
    if (i < topy) top = (top * F::sub2(one_i, r).norm().canon()).canon();
  }
  const uint32_t sx = effx / 2, lx = effx - sx;
  const uint32_t bpm = r1cs_eval_blocks(max_rows);
  // arena: [0, kScratch) is what eq_evals_t stages its own sqrt-size tables in (its arena_reserve is then a no-op and moves nothing)
  constexpr size_t kScratch = 2 * ((size_t)32 << kMax) + 512;
  const size_t oXL = kScratch, oXR = oXL + pad256((size_t)32 << lx), oTY = oXR + pad256((size_t)32 << sx), oP = oTY + pad256((size_t)32 << effy),
               oOut = oP + pad256((size_t)32 * k * bpm), total = oOut + 256;
  arena_reserve(c, total);
  if (!c.pinned) HIPCHK(hipHostMalloc((void**)&c.pinned, DeviceBackend::kPinnedBytes, hipHostMallocDefault));
  const bool prof = G.profiling;
  DeviceBackend be(c, false, prof);
  try {
    be.mark("kernel");
    EqSplit2Fn<FID> f;  // both halves of T_x in the internal form; the constant of the upper variables rides in the left one
    f.outL = (uint32_t*)(c.arena + oXL), f.outR = (uint32_t*)(c.arena + oXR);
    f.ellL = lx, f.ellR = sx, f.oneL = top, f.oneR = one_i;
    for (uint32_t i = 0; i < 2 * kMax; i++) f.r[i] = f.nr[i] = F::zero();
    for (uint32_t i = 0; i < effx; i++) f.r[i] = rx[i], f.nr[i] = nrx[i];
    be.launch(f, (1u << lx) + (1u << sx));
    eq_evals_t<FID>(c, (const uint8_t*)r_y + 32 * (size_t)topy, effy, flags, (uint32_t*)(c.arena + oTY));
    R1csEvalArgs a{};
    for (size_t j = 0; j < k; j++) {
      a.indptr[j] = it[j].indptr, a.indices[j] = it[j].indices, a.data[j] = it[j].data;
      a.rows[j] = (uint32_t)it[j].rows;
      a.colmask[j] = spmv_index_mask(it[j].cols);
    }
    a.xL = f.outL, a.xR = f.outR, a.ty = (const uint32_t*)(c.arena + oTY);
    a.partial = (uint32_t*)(c.arena + oP), a.sx = sx, a.bpm = bpm;
    hipLaunchKernelGGL((k_r1cs_eval<FID>), dim3((uint32_t)k * bpm), dim3(256), 0, c.stream, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL((k_r1cs_eval_finish<FID>), dim3((uint32_t)k), dim3(256), 0, c.stream, (const uint32_t*)a.partial, bpm,
                       (uint32_t*)(c.arena + oOut));
    HIPCHK(hipGetLastError());
    be.mark("end");
    HIPCHK(hipMemcpyAsync(c.pinned, c.arena + oOut, 32 * k, hipMemcpyDeviceToHost, c.stream));
    stream_wait(c.stream);
  } catch (...) {
    (void)hipStreamSynchronize(c.stream);
    throw;
  }
  memcpy(out, c.pinned, 32 * k);
  if (prof && be.nmarks == 2) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
    prof_store(&ms, 1);
  }
}

void fv_r1cs_evaluate(Ctx& c, int field, const CsrView* mats, size_t k, const void* r_x, uint32_t ell_x, const void* r_y,
                      uint32_t ell_y, uint32_t flags, uint8_t* out) {
  with_field(field, [&](auto F) { r1cs_eval_t<F()>(c, mats, k, r_x, ell_x, r_y, ell_y, flags, out); });
}
#endif

}  // namespace nmx
