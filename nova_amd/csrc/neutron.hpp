// neutron.hpp -- the N-sized work of NeutronNova's folding step (src/neutron/ of the reference) that nothing else in the C ABI expresses:
//     PowPolynomial::split_evals   (src/spartan/polys/power.rs:62-86)   [tau^j, j < left] ++ [(tau^left)^i, i < right]
//     NIFS::prove_helper           (src/neutron/nifs.rs:29-186)         the five sums of the zero-fold at t = 0, 2, 3, 4, 5
//     Structure::is_sat, the sum   (src/neutron/relation.rs:83-97)      sum_i f[i] sum_j e[j] (Az Bz - Cz)[i * left + j]
//     FoldedWitness::fold          (src/neutron/relation.rs:131-156)    w1 + r_b (w2 - w1), W and E in one launch
// Included at the end of sumcheck.hip (whose block sum and one-block finish the two sums use).  The lane bodies use no wave-level
// intrinsic, so tests/host_emul/neutron_emul.cpp runs them on the CPU (simt.hpp) with the limb bounds asserted (NMX_DEBUG_BOUNDS).
//
// Notation.  E = e ++ f with e = E[0, left), f = E[left, left + right); an N-vector (N = left * right) is indexed k = i * left + j,
// i < right, j < left; X(t) = X1 + t (X2 - X1).
//
// The two sums, one kernel template (POINTS = 5: the fold sums; POINTS = 1: the relation sum, one instance).  The reference's factored
// form is kept: sum_i f(t)[i] * (sum_j e(t)[j] * (Az(t) Bz(t) - Cz(t))[k]), and since the outer factor distributes over ANY split of the
// inner sum, no lane ever waits for another: the work is cut into tiles of one row x kNeutronTileCols columns, a wave takes tiles
// wave, wave + waves, ... and each of its lanes adds up its own columns of the tile (lane, lane + 64, ...: a wave reads 2 KiB contiguous
// per vector), multiplies that partial inner sum by f(t)[i] and keeps five running totals.  Per element: 5 products for the terms + 5 for
// e(t) (+ 5 per lane and tile for f(t): 1.25 per element on full tiles) against 6 x 32 B of loads.  The points are walked incrementally,
// X(t + 1) = X(t) + (X2 - X1), as the reference does.  A block leaves one set of exact (canonical) partials; k_sum_partials_n, one block,
// adds them and the result comes back through the context's pinned buffer.  Every partial is the canonical representative, so the result
// depends neither on the grid nor on the option neutron_max_blocks (0 = by size; else the largest grid: tests force the tile loop of a
// wave at tiny shapes).  The e / f tables are sqrt-sized and read through L2; they are not staged in LDS.
//
// Forms.  Stored words are x Fm (Fm = 1 canonical, 2^256 Montgomery), R' = 2^261, nk = p - Fm as a plain integer:
//     P   = mul_add(A, B, C, nk)  = (A B - C)     Fm^2 / R'
//     S  += E * P                 = e (A B - C)   Fm^3 / R'^2
//     G  += S * F                 = f e (A B - C) Fm^4 / R'^3         -- four stored factors: the host's correction is eq_sums_t's, k = 4
//
// Bounds (p = the modulus; a product of operands below a p and b p with a b < 127 is normalised and below p (1 + a b / 127); stored
// words may be any 256-bit value, 2^256 < 6 p for all four fields):
//   fold sums      every operand goes through below_p (< p); a difference d = (x2 - x1 + 2 p).norm().canon4() < p; X(t) = X(t - 1) + d is
//                  normalised at every point it is used: X(t) < (t + 1) p <= 6 p, limbs < 2^29 (the top limb < 2^25)
//                  P(t) = A(t) B(t) + C(t) nk < p (1 + (36 + 6) / 127) < 1.34 p;   E(t) * P(t) < p (1 + 6 * 1.34 / 127) < 1.07 p
//   relation sum   no differences: the words enter products only.  P < p (1 + (36 + 6) / 127) < 1.34 p;  E * P < 1.07 p
//   S, G           a canonical accumulator plus at most six lazily added terms (< 1.07 p each, limbs < 2^29): value < 7.5 p, limbs
//                  < 7 * 2^29 < 2^32 - 2^4 -> norm().canon().  S canonical times F(t) (< 6 p) < 1.05 p.  The length of a sum does not
//                  enter: the accumulators return below p after every sixth term.
//   fold witness   w1, w2 any words: w2 - w1 + 8 p < 14 p, r (canonical) times it < 1.12 p, plus w1 < 7.2 p -> canon() (BindTopFn's bound)
//   pow tables     a running product < 1.01 p times a canonical squaring < 1.01 p
#pragma once

#include "msm_partition.hpp"  // NMX_DEV: the device / emulation spelling
#include "spmv_row.hpp"       // ld / st / below_p

namespace nmx {

static constexpr uint32_t kNeutronTileCols = 256;   // columns of a tile: four per lane
static constexpr uint32_t kNeutronMaxBlocks = 2048;  // the largest grid of the sums (the one-block finish reads one set of partials per block)
static constexpr int kNeutronPowBits = 31;           // left + right < 2^31

// ---- the two sums ----------------------------------------------------------------------------------------------------------------
template <int FID> struct NeutronSumArgs {
  const uint32_t *E1, *A1, *B1, *C1;  // instance 1 (the relation sum: the only one)
  const uint32_t *E2, *A2, *B2, *C2;  // instance 2 (POINTS = 5 only)
  Fp<FID> nk;                         // p - Fm, a plain integer, canonical
  uint32_t left, right;
};
// the extrapolation points of prove_helper (nifs.rs:163-183) are 0, 2, 3, 4, 5: slot s of a five-point sum is point s + (s > 0).
// X <- X at the point of slot s, from the point of slot s - 1 (s >= 1); normalised (limbs < 3 * 2^29 before)
template <int FID> NMX_DEV void neutron_step(Fp<FID>& x, const Fp<FID>& d, int s) { x = s == 1 ? (x + d + d).norm() : (x + d).norm(); }
// the canonical difference x2 - x1 of two operands below p
template <int FID> NMX_DEV Fp<FID> neutron_diff(const Fp<FID>& x2, const Fp<FID>& x1) { return Fp<FID>::sub2(x2, x1).norm().canon4(); }

template <int FID> NMX_DEV void neutron_acc_flush(Fp<FID>& s) { s = s.norm().canon(); }

// One lane's columns first, first + stride, ... (below col_end) of row `row`: S[s] += e(t_s)[j] (Az(t_s) Bz(t_s) - Cz(t_s))[k].  S canonical
// on entry and on return.
template <int FID, int POINTS>
NMX_DEV void neutron_tile_lane(const NeutronSumArgs<FID>& a, uint32_t row, uint32_t first, uint32_t col_end, uint32_t stride, Fp<FID> (&S)[POINTS]) {
  using F = Fp<FID>;
  uint32_t pending = 0;
  for (uint64_t j64 = first; j64 < col_end; j64 += stride) {
    const uint32_t j = (uint32_t)j64;
    const size_t k = (size_t)row * a.left + j;
    if constexpr (POINTS == 1) {
      const F P = F::mul_add(ld<FID>(a.A1, k), ld<FID>(a.B1, k), ld<FID>(a.C1, k), a.nk);  // words < 6 p
      P.check_below(1.34, "neutron relation sum: A B - C");
      const F T = ld<FID>(a.E1, j) * P;
      T.check_below(1.07, "neutron relation sum: e (A B - C)");
      S[0] = S[0] + T;
    } else {
      F x[8] = {ld<FID>(a.A1, k), ld<FID>(a.A2, k), ld<FID>(a.B1, k), ld<FID>(a.B2, k), ld<FID>(a.C1, k), ld<FID>(a.C2, k), ld<FID>(a.E1, j), ld<FID>(a.E2, j)};
      below_p<FID, 8>(x);  // every operand enters a difference
      F A = x[0], B = x[2], C = x[4], E = x[6];
      const F dA = neutron_diff<FID>(x[1], x[0]), dB = neutron_diff<FID>(x[3], x[2]), dC = neutron_diff<FID>(x[5], x[4]), dE = neutron_diff<FID>(x[7], x[6]);
#pragma unroll
      for (int s = 0; s < POINTS; s++) {
        if (s) {
          neutron_step<FID>(A, dA, s);
          neutron_step<FID>(B, dB, s);
          neutron_step<FID>(C, dC, s);
          neutron_step<FID>(E, dE, s);
        }
        A.check_below(6.0, "neutron fold sums: Az(t)");
        B.check_below(6.0, "neutron fold sums: Bz(t)");
        C.check_below(6.0, "neutron fold sums: Cz(t)");
        E.check_below(6.0, "neutron fold sums: e(t)");
        const F P = F::mul_add(A, B, C, a.nk);
        P.check_below(1.34, "neutron fold sums: Az(t) Bz(t) - Cz(t)");
        const F T = E * P;
        T.check_below(1.07, "neutron fold sums: e(t) (Az(t) Bz(t) - Cz(t))");
        S[s] = S[s] + T;
      }
    }
    if (++pending == 6) {
#pragma unroll
      for (int s = 0; s < POINTS; s++) neutron_acc_flush<FID>(S[s]);
      pending = 0;
    }
  }
#pragma unroll
  for (int s = 0; s < POINTS; s++) neutron_acc_flush<FID>(S[s]);
}

// What one lane adds up: tiles first_tile, first_tile + tile_stride, ... of the right * ceil(left / kNeutronTileCols) tiles, its columns
// of each (lane, lane + lanes, ...) times the row's f(t).  G canonical on return.
template <int FID, int POINTS>
NMX_DEV void neutron_sums_lane(const NeutronSumArgs<FID>& a, uint32_t first_tile, uint32_t tile_stride, uint32_t lane, uint32_t lanes, Fp<FID> (&G)[POINTS]) {
  using F = Fp<FID>;
  const uint32_t tiles_per_row = a.left / kNeutronTileCols + (a.left % kNeutronTileCols ? 1u : 0u);
  const uint64_t n_tiles = (uint64_t)a.right * tiles_per_row;  // <= left * right < 2^31
#pragma unroll
  for (int s = 0; s < POINTS; s++) G[s] = F::zero();
  uint32_t pending = 0;
  for (uint64_t t64 = first_tile; t64 < n_tiles; t64 += tile_stride) {
    const uint32_t row = (uint32_t)(t64 / tiles_per_row), col0 = (uint32_t)(t64 % tiles_per_row) * kNeutronTileCols;
    if ((uint64_t)col0 + lane >= a.left) continue;  // (a lane without a column in this tile: uniform per lane, no barrier below)
    const uint32_t col_end = a.left - col0 < kNeutronTileCols ? a.left : col0 + kNeutronTileCols;
    F S[POINTS];
#pragma unroll
    for (int s = 0; s < POINTS; s++) S[s] = F::zero();
    neutron_tile_lane<FID, POINTS>(a, row, col0 + lane, col_end, lanes, S);
    if constexpr (POINTS == 1) {
      const F T = S[0] * ld<FID>(a.E1, (size_t)a.left + row);  // f any word, < 6 p
      T.check_below(1.05, "neutron relation sum: f * inner sum");
      G[0] = G[0] + T;
    } else {
      F f[2] = {ld<FID>(a.E1, (size_t)a.left + row), ld<FID>(a.E2, (size_t)a.left + row)};
      below_p<FID, 2>(f);
      F Ft = f[0];
      const F dF = neutron_diff<FID>(f[1], f[0]);
#pragma unroll
      for (int s = 0; s < POINTS; s++) {
        if (s) neutron_step<FID>(Ft, dF, s);
        Ft.check_below(6.0, "neutron fold sums: f(t)");
        const F T = S[s] * Ft;
        T.check_below(1.05, "neutron fold sums: f(t) * inner sum");
        G[s] = G[s] + T;
      }
    }
    if (++pending == 6) {
#pragma unroll
      for (int s = 0; s < POINTS; s++) neutron_acc_flush<FID>(G[s]);
      pending = 0;
    }
  }
#pragma unroll
  for (int s = 0; s < POINTS; s++) neutron_acc_flush<FID>(G[s]);
}

// blocks of the sums' grid: four tiles (one per wave) per block, at most `opt` (the option neutron_max_blocks; 0: kNeutronMaxBlocks)
static inline uint32_t neutron_blocks(size_t left, size_t right, uint32_t opt) {
  const uint64_t tiles = (uint64_t)right * ((left + kNeutronTileCols - 1) / kNeutronTileCols);
  const uint64_t want = (tiles + 3) / 4;
  const uint32_t cap = opt && opt < kNeutronMaxBlocks ? opt : kNeutronMaxBlocks;
  return (uint32_t)(want < cap ? want : cap);
}

// ---- FoldedWitness::fold: both vectors in one launch (lane i < n_w: W, else E), as FoldPairFn ----------------------------------------
template <int FID> struct NeutronFoldFn {
  const uint32_t *w1, *w2, *e1, *e2;
  uint32_t *w, *e;
  uint32_t n_w;
  Fp<FID> r;  // r_b * 2^261, canonical
  static NMX_HD void one(const uint32_t* lo, const uint32_t* hi, uint32_t* out, uint32_t i, const Fp<FID>& r) {
    using F = Fp<FID>;
    const F l = ld<FID>(lo, i), h = ld<FID>(hi, i);  // a lane reads its own element before it writes it: in place is safe
    const F y = (l + r * F::sub8(h, l).norm()).norm();
    y.check_below(7.2, "neutron fold witness: w1 + r (w2 - w1)");
    st<FID>(out, i, y);
  }
  NMX_HD void operator()(uint32_t i) const {
    if (i < n_w) one(w1, w2, w, i, r);
    else one(e1, e2, e, i - n_w, r);
  }
};

// ---- PowPolynomial::split_evals: lane id multiplies the squarings its index's bits select (no serial chain, one launch) ---------------
template <int FID> struct NeutronPowFn {
  uint32_t* out;
  Fp<FID> sq_e[kNeutronPowBits];  // tau^(2^b) * 2^261, canonical
  Fp<FID> sq_f[kNeutronPowBits];  // (tau^left)^(2^b) * 2^261, canonical
  Fp<FID> unit;                   // Fm as a plain integer: the stored form of 1
  uint32_t left;
  NMX_HD void operator()(uint32_t id) const {
    using F = Fp<FID>;
    const bool hi = id >= left;
    const uint32_t x = hi ? id - left : id;
    F acc = unit;
#pragma unroll
    for (int b = 0; b < kNeutronPowBits; b++) {  // (unrolled: the squarings are read at constant offsets of the kernel arguments)
      if ((x >> b) == 0) break;
      if ((x >> b) & 1u) {
        F s;
#pragma unroll
        for (int i = 0; i < 9; i++) s.l[i] = hi ? sq_f[b].l[i] : sq_e[b].l[i];
        acc = acc * s;
        acc.check_below(1.01, "neutron pow tables: running product");
      }
    }
    st<FID>(out, id, acc);
  }
};

#if defined(__HIPCC__) || defined(__HIP__)
template <int FID, int POINTS> __global__ __launch_bounds__(256) void k_neutron_sums(NeutronSumArgs<FID> a, uint32_t* partial /* 8 elements per block */) {
  using F = Fp<FID>;
  __shared__ uint32_t lds[36 * POINTS];
  F G[POINTS];
  neutron_sums_lane<FID, POINTS>(a, blockIdx.x * 4u + (threadIdx.x >> 6), gridDim.x * 4u, threadIdx.x & 63u, 64u, G);
  block_sum_waves<FID, POINTS>(G, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int s = 0; s < POINTS; s++) G[s].to_words(partial + 64 * (size_t)blockIdx.x + 8 * s);
  }
}

// ---- the host half ---------------------------------------------------------------------------------------------------------------
// host operands are staged through the context arena (as VecIO and MercuryArena do in fieldvec.hip, the other translation unit); device
// operands are used in place
struct NeutronArena {
  Ctx& c;
  bool dev;
  size_t used = 0;
  char* take(size_t bytes) {
    char* d = c.arena + used;
    used += pad256(bytes);
    return d;
  }
  const uint32_t* in(const void* p, size_t elems) {
    if (dev || !elems) return (const uint32_t*)p;
    char* d = take(elems * 32);
    HIPCHK(hipMemcpyAsync(d, p, elems * 32, hipMemcpyHostToDevice, c.stream));
    return (const uint32_t*)d;
  }
};
static void neutron_finish(Ctx& c, DeviceBackend& be, bool prof, bool async) {
  if (async) {
    async_mark(c);  // no wait: the next call of this host thread is ordered behind this one
    return;
  }
  stream_wait(c.stream);
  if (prof && be.nmarks == 2) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
    prof_store(&ms, 1);
  }
}

// v: E1, Az1, Bz1, Cz1 (and E2, Az2, Bz2, Cz2 for the fold sums); out: POINTS elements on the host
template <int FID, int POINTS>
static void neutron_sums_t(Ctx& c, size_t left, size_t right, const void* const* v, const void* rho, uint32_t flags, uint8_t* out) {
  using F = Fp<FID>;
  const bool mont = flags & NMX_SCALARS_MONT, dev = flags & NMX_SCALARS_DEVICE;
  const size_t n = left * right, n_e = left + right;
  // c_t(rho) = (1 - rho) + t (2 rho - 1), internal form; NMX_E_SCALAR_RANGE before anything is enqueued
  F ct[POINTS];
  if constexpr (POINTS == 5) {
    const F r = challenge_internal<FID>(rho, mont), one = F::one();
    const F step = F::sub2(r.dbl().norm(), one).norm().canon();  // 2 rho - 1
    F cur = F::sub2(one, r).norm().canon();                      // 1 - rho
    for (int s = 0; s < POINTS; s++) {
      if (s) cur = (s == 1 ? cur + step + step : cur + step).norm().canon();
      ct[s] = cur;
    }
  }
  const uint32_t blocks = neutron_blocks(left, right, G.neutron_max_blocks.load(std::memory_order_relaxed));
  const int n_inst = POINTS == 5 ? 2 : 1;
  arena_reserve(c, pad256((size_t)blocks * 256) + 256 + (dev ? 0 : n_inst * (pad256(n_e * 32) + 3 * pad256(n * 32))) + 512);
  NeutronArena ws{c, dev};
  uint32_t* partial = (uint32_t*)ws.take((size_t)blocks * 256);
  uint32_t* dout = (uint32_t*)ws.take(256);
  const F fm = sc_form_factor<FID>(mont);
  NeutronSumArgs<FID> a;
  const uint32_t* d[8] = {};
  const bool prof = G.profiling;
  DeviceBackend be(c, false, prof);
  uint32_t res[8 * POINTS];
  try {
    for (int i = 0; i < 4 * n_inst; i++) d[i] = ws.in(v[i], i % 4 == 0 ? n_e : n);
    a.E1 = d[0], a.A1 = d[1], a.B1 = d[2], a.C1 = d[3], a.E2 = d[4], a.A2 = d[5], a.B2 = d[6], a.C2 = d[7];
    a.nk = F::sub2(F::zero(), fm.canon()).norm().canon();
    a.left = (uint32_t)left, a.right = (uint32_t)right;
    be.mark("kernel");
    hipLaunchKernelGGL((k_neutron_sums<FID, POINTS>), dim3(blocks), dim3(256), 0, c.stream, a, partial);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL((k_sum_partials_n<FID, POINTS, 8>), dim3(1), dim3(256), 0, c.stream, partial, blocks, dout);
    HIPCHK(hipGetLastError());
    be.mark("end");
    be.d2h(res, dout, 32 * POINTS);  // through the context's pinned landing buffer
    be.sync();
  } catch (...) {
    (void)hipStreamSynchronize(c.stream);  // nothing of this call still reads the caller's vectors
    throw;
  }
  if (prof && be.nmarks == 2) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
    prof_store(&ms, 1);
  }
  // the sums carry x Fm^4 / R'^3 (four stored factors: eq_sums_t's correction with k = 4), then c_t(rho) in the internal form
  const F corr = pow2_plain<FID>(261u * 4 - (mont ? 256u * 3 : 0u));
  for (int s = 0; s < POINTS; s++) {
    F y = (F::from_words(res + 8 * s) * corr).canon();
    if constexpr (POINTS == 5) y = (y * ct[s]).canon();
    uint32_t w[8];
    y.to_words(w);
    memcpy(out + 32 * s, w, 32);
  }
}

template <int FID>
static void neutron_fold_witness_t(Ctx& c, const void* w1, const void* w2, size_t n_w, const void* e1, const void* e2, size_t n_e, const void* r_b,
                                   uint32_t flags, void* w, void* e) {
  const bool dev = flags & NMX_SCALARS_DEVICE, async = dev && (flags & NMX_ASYNC);
  const Fp<FID> r = challenge_internal<FID>(r_b, flags & NMX_SCALARS_MONT);  // NMX_E_SCALAR_RANGE before anything is enqueued
  arena_reserve(c, (dev ? 0 : 3 * (pad256(n_w * 32) + pad256(n_e * 32))) + 256);
  NeutronArena ws{c, dev};
  const bool prof = G.profiling;
  DeviceBackend be(c, false, prof);
  try {
    NeutronFoldFn<FID> f;
    f.w1 = ws.in(w1, n_w), f.w2 = ws.in(w2, n_w), f.e1 = ws.in(e1, n_e), f.e2 = ws.in(e2, n_e);
    f.w = dev ? (uint32_t*)w : (uint32_t*)ws.take(n_w * 32), f.e = dev ? (uint32_t*)e : (uint32_t*)ws.take(n_e * 32);
    f.n_w = (uint32_t)n_w, f.r = r;
    be.mark("kernel");
    be.launch(f, (uint32_t)(n_w + n_e));
    be.mark("end");
    if (!dev) {
      if (n_w) HIPCHK(hipMemcpyAsync(w, f.w, n_w * 32, hipMemcpyDeviceToHost, c.stream));
      if (n_e) HIPCHK(hipMemcpyAsync(e, f.e, n_e * 32, hipMemcpyDeviceToHost, c.stream));
    }
  } catch (...) {
    (void)hipStreamSynchronize(c.stream);
    throw;
  }
  neutron_finish(c, be, prof, async);
}

template <int FID>
static void neutron_pow_t(Ctx& c, const void* tau, size_t left, size_t right, uint32_t flags, void* out) {
  using F = Fp<FID>;
  using H = HostFp4<FID>;
  const bool mont = flags & NMX_SCALARS_MONT, dev = flags & NMX_SCALARS_DEVICE, async = dev && (flags & NMX_ASYNC);
  (void)challenge_internal<FID>(tau, mont);  // NMX_E_SCALAR_RANGE before anything is enqueued
  const size_t n = left + right;
  // the squarings, on the host: tau^(2^b), then tau^left from them, then (tau^left)^(2^b)
  NeutronPowFn<FID> f;
  H sq = mont ? H::from_mont256(tau) : H::from_canonical(tau), tl = H::one();
  for (int b = 0; b < kNeutronPowBits; b++) {
    f.sq_e[b] = sq.to_device();
    if ((left >> b) & 1u) tl = tl * sq;
    sq = sq * sq;
  }
  for (int b = 0; b < kNeutronPowBits; b++) {
    f.sq_f[b] = tl.to_device();
    tl = tl * tl;
  }
  f.unit = sc_form_factor<FID>(mont);
  f.left = (uint32_t)left;
  arena_reserve(c, (dev ? 0 : pad256(n * 32)) + 256);
  NeutronArena ws{c, dev};
  const bool prof = G.profiling;
  DeviceBackend be(c, false, prof);
  try {
    f.out = dev ? (uint32_t*)out : (uint32_t*)ws.take(n * 32);
    be.mark("kernel");
    be.launch(f, (uint32_t)n);
    be.mark("end");
    if (!dev) HIPCHK(hipMemcpyAsync(out, f.out, n * 32, hipMemcpyDeviceToHost, c.stream));
  } catch (...) {
    (void)hipStreamSynchronize(c.stream);
    throw;
  }
  neutron_finish(c, be, prof, async);
}

void fv_pow_split_evals(Ctx& c, int field, const void* tau, size_t left, size_t right, uint32_t flags, void* out) {
  with_field(field, [&](auto F) { neutron_pow_t<F()>(c, tau, left, right, flags, out); });
}
void fv_neutron_fold_sums(Ctx& c, int field, size_t left, size_t right, const void* const* v8, const void* rho, uint32_t flags, uint8_t* out160) {
  with_field(field, [&](auto F) { neutron_sums_t<F(), 5>(c, left, right, v8, rho, flags, out160); });
}
void fv_neutron_relation_sum(Ctx& c, int field, size_t left, size_t right, const void* const* v4, uint32_t flags, uint8_t* out32) {
  with_field(field, [&](auto F) { neutron_sums_t<F(), 1>(c, left, right, v4, nullptr, flags, out32); });
}
void fv_neutron_fold_witness(Ctx& c, int field, const void* w1, const void* w2, size_t n_w, const void* e1, const void* e2, size_t n_e, const void* r_b,
                             uint32_t flags, void* w, void* e) {
  with_field(field, [&](auto F) { neutron_fold_witness_t<F()>(c, w1, w2, n_w, e1, e2, n_e, r_b, flags, w, e); });
}
#endif

}  // namespace nmx
