// sumcheck_ppsnark.hpp -- ppsnark's batched inner sum-check as ONE C call (nmx_sumcheck_prove_ppsnark).  Included by sumcheck.hip
// behind sumcheck_batched.hpp; the mailbox, the eq heaps and the host algebra are sumcheck_prove.hpp's and sc_host.hpp's.
//
//   RelaxedR1CSSNARK::prove_helper                                     src/spartan/ppsnark.rs:886-983
//   MemorySumcheckInstance (claims 0-5, ten tables)                    src/spartan/ppsnark.rs:520-670
//   InnerBatchedSumcheckInstance (claims 6-7, four tables)             src/spartan/ppsnark.rs:725-786
//   WitnessBoundSumcheck (claim 8, two tables)                         src/spartan/ppsnark.rs:293-325
//   compute_eval_points_linear / _quadratic / _cubic                   src/spartan/sumcheck.rs:356-443
//   evaluation_points_cubic_with_three_inputs / _two_inputs / quadratic_with_one_input and their fallbacks
//                                                                      src/spartan/sumcheck.rs:900-1222
//
// A round needs 18 sums over 16 tables.  In the 9-limb form that is 162 registers of accumulators, so the pass is cut by instance,
// one kernel family and one mailbox slot per group:
//   memory group   5 tables (t, tinv, w, winv, ts), 6 sums -- run for row (slot 0) and for col (slot 1) by the same code:
//                  D(0) = sum (tinv - winv) low, D(1) = the same over the high halves (claim 0 / 1 is linear: D(-1) = 2 D(0) - D(1));
//                  (t(0), t(inf)) of (tinv t - ts) and of (winv w - 1), both under eq(rhos)
//   inner group    4 tables (L_row, L_col, val, E), 4 sums (slot 2): sum a b c, sum da db dc, sum a(-1) b(-1) c(-1) without an eq factor;
//                  t(0) of E under eq(r_outer)
//   witness group  2 tables (W, masked_eq), 2 sums (slot 3): sum A B, sum A(-1) B(-1)
// Three pass kinds per group, one index per lane, each index visited once:
//   sums         id in [0, len/2) over the tables as they are: round 1.  Pointed at the HIGH halves with with_inf = 0 it gives t(1) of
//                the claims under an eq whose tau is zero (t(0)'s summand alone, reading X[id] only): the fallback's third sum,
//                t(-1) = 2 t(inf) + 2 t(0) - t(1), or 2 t(0) - t(1) for E.  (The witness group has no eq and no such form.)
//   bind + sums  id in [0, len/4): every table of the group bound with the round's challenge in place (four loads, two stores per
//                table: a lane reads exactly the elements it overwrites) and the NEXT round's sums over the bound values.
//   bind only    id in [0, len/2): the last device bind, ONE kernel over all 16 tables (two loads, one store per table, no sums);
//                the bound tables also go to a contiguous staging area which one stream-ordered copy brings to the host.
// Each pass leaves its sums per block in the group's partials area; k_sum_partials_mail (one block) adds them into the group's
// mailbox slot.  Every kernel is launched after its challenge exists and ends on its own: no pre-launched pass, no resident kernel,
// nothing on the device waits for the host.  Of the sc_* options only sc_host_tail and sc_poll_us apply.
//
// Bytes per index (32 B elements).  bind + sums: memory 5 x (4 loads + 2 stores) = 960 B, inner 768 B, witness 384 B, plus the eq
// reads (32 B, 64 B in the first half of the rounds) in the memory and inner groups: ~3.2 KB per index of len/4 for all four passes.
// sums: memory 9 loads = 288 B (t(1) form: 5 = 160 B), inner 7 = 224 B (t(1) form: 32 B), witness 4 = 128 B.  bind only: 16 x 96 B
// and 16 x 32 B to the staging area.
//
// Powers of R' = 2^261 (fp.hpp: a product of two stored words x~ y~ comes out as x~ y~ / R').  With Fm the vectors' form factor
// (1 canonical, 2^256 Montgomery), nk = p - Fm and `one` = Fm (the stored ONE):
//   D              a difference of stored words                       x Fm             1 stored factor   (ScDev::raw(., 1))
//   tinv t - ts    mul_add(tinv, t, ts, nk)                           x Fm^2 / R'
//   winv w - 1     mul_add(winv, w, one, nk)                          x Fm^2 / R'      times the eq factor (Fm / R' per table):
//                                                                     3 factors with eqR alone, 4 with eqL    (raw(., 3 / 4))
//   a b c          (a * b) * c                                        x Fm^3 / R'^2    3 factors
//   E eq           e * fac                                            2 factors with eqR alone, 3 with eqL
//   A B            a * b                                              x Fm^2 / R'      2 factors
#pragma once

#include "msm_partition.hpp"  // NMX_DEV, NMX_TID: the device / emulation spellings
#include "spmv_row.hpp"       // ld

namespace nmx {

// ---- arguments (POD, by value) ------------------------------------------------------------------------------------------------------
template <int FID> struct ScPpsMemArgs {
  uint32_t *t, *tinv, *w, *winv, *ts;  // table order of the header within a group: NMX_PPS_T_ROW ..
  Fp<FID> r, nk, one;                  // the challenge (internal form, canonical); p - Fm; Fm
  const uint32_t *eqL, *eqR;           // ScEqDev::tables (eq(rhos)) of the round the sums belong to
  uint32_t shift, mask;
  uint32_t n;         // indices of the pass: len / 2 (sums) or len / 4 (bind + sums)
  uint32_t with_inf;  // sums: 1 = all six sums; 0 = the two t(0) sums alone, reading X[id] only
};
template <int FID> struct ScPpsInnerArgs {
  uint32_t *a, *b, *c, *e;    // L_row, L_col, val, E
  Fp<FID> r;
  const uint32_t *eqL, *eqR;  // eq(r_outer)
  uint32_t shift, mask, n, with_inf;  // with_inf = 0: E's t(0) alone, reading E[id] only
};
template <int FID> struct ScPpsWitArgs {
  uint32_t *w, *m;  // W, masked_eq
  Fp<FID> r;
  uint32_t n;
};
static constexpr uint32_t kScPpsTables = 16;
template <int FID> struct ScPpsBindArgs {
  uint32_t* X[kScPpsTables];
  Fp<FID> r;
  uint32_t* stage;  // table t at element t * n
  uint32_t n;       // len / 2
  uint32_t bind;    // 0: the tables go to the staging area as they are
};

template <int FID> NMX_DEV Fp<FID> sc_pps_factor(const uint32_t* eqL, const uint32_t* eqR, uint32_t shift, uint32_t mask, uint32_t id) {
  Fp<FID> fac = ld<FID>(eqR, eqL ? (id & mask) : id);
  if (eqL) fac = ld<FID>(eqL, id >> shift) * fac;  // < 1.01 p
  return fac;
}
// bind_poly_var_top (multilinear.rs:65-84) on the two elements of X that next-round index id reads: lo + r (hi - lo), in place.
// y0, y1 canonical.
template <int FID> NMX_DEV void sc_pps_bind2(uint32_t* X, const Fp<FID>& r, uint32_t id, uint32_t hq, Fp<FID>& y0, Fp<FID>& y1) {
  using F = Fp<FID>;
  const F x00 = ld<FID>(X, id), x01 = ld<FID>(X, (size_t)id + hq);
  const F x10 = ld<FID>(X, (size_t)id + 2 * (size_t)hq), x11 = ld<FID>(X, (size_t)id + 3 * (size_t)hq);
  y0 = (x00 + r * F::sub2(x10, x00).norm()).norm().canon();
  y1 = (x01 + r * F::sub2(x11, x01).norm()).norm().canon();
  y0.to_words(X + 8 * (size_t)id);
  y1.to_words(X + 8 * ((size_t)id + hq));
}

// Lazy-addition bounds shared by the three accumulator sets below.  Table elements and bound values are canonical (< p, limbs
// < 2^29).  Every term added to an eq-free or eq-factored product sum is ONE product, normalised (limbs < 2^29) and < 1.05 p:
//   e  = mul_add(x, y, z, nk)        < p (1 + 2 / 127)            < 1.02 p        fac = eqL * eqR < 1.01 p
//   q  = (x1 - x0)(y1 - y0)          operands < 3 p               < 1.08 p
//   e * fac, q * fac                 < p (1 + 1.08 * 1.01 / 127)  < 1.01 p
//   (a b) c                          < 1.01 p;   (da db) dc: 1.08 p x 3 p < 1.03 p;   (a(-1) b(-1)) c(-1): operands < 4 p: 1.13 p x 4 p < 1.04 p
//   A(-1) B(-1)                      operands < 4 p               < 1.13 p
// A sum is brought back below p (norm + canon) after every 6 terms: it holds at most 1 canonical + 6 fresh terms, value
// < 1 + 6 * 1.13 < 8 p (canon takes < 16 p), limbs < 7 * 2^29 < 2^32 - 2^4 (what norm takes).  The two D sums add a difference
// a + 2p - b (< 3 p, limbs < 2^29 + 2^31) per index and are brought back every index, as k_plain_sums kind 2 does: < 4 p.
static constexpr uint32_t kScPpsLazy = 6;

// ---- memory group -------------------------------------------------------------------------------------------------------------------
template <int FID> struct ScPpsMemAcc {  // s[0], s[1]: D(0), D(1); s[2], s[3]: T's t(0), t(inf); s[4], s[5]: W's
  using F = Fp<FID>;
  F s[6];
  uint32_t pending = 0;
  NMX_DEV ScPpsMemAcc() {
#pragma unroll
    for (int i = 0; i < 6; i++) s[i] = F::zero();
  }
  // one index: the low / high elements of the five tables (hi unused without with_inf)
  NMX_DEV void add(const ScPpsMemArgs<FID>& a, const F& fac, bool wi, const F& t0, const F& t1, const F& ti0, const F& ti1, const F& w0, const F& w1,
                   const F& wi0, const F& wi1, const F& ts0) {
    const F eT = F::mul_add(ti0, t0, ts0, a.nk), eW = F::mul_add(wi0, w0, a.one, a.nk);
    eT.check_below(1.02, "ppsnark memory: tinv t - ts"), eW.check_below(1.02, "ppsnark memory: winv w - 1");
    s[2] = s[2] + eT * fac, s[4] = s[4] + eW * fac;
    if (wi) {
      const F qT = F::sub2(ti1, ti0).norm() * F::sub2(t1, t0).norm(), qW = F::sub2(wi1, wi0).norm() * F::sub2(w1, w0).norm();
      qT.check_below(1.08, "ppsnark memory: dtinv dt"), qW.check_below(1.08, "ppsnark memory: dwinv dw");
      s[3] = s[3] + qT * fac, s[5] = s[5] + qW * fac;
      s[0] = (s[0] + F::sub2(ti0, wi0)).norm().canon(), s[1] = (s[1] + F::sub2(ti1, wi1)).norm().canon();
    }
    if (++pending == kScPpsLazy) flush();
  }
  NMX_DEV void flush() {
#pragma unroll
    for (int i = 2; i < 6; i++) {
      s[i] = s[i].norm();
      s[i].check_below(8.0, "ppsnark memory: a lane's lazy sum");
      s[i] = s[i].canon();
    }
    pending = 0;
  }
};
template <int FID> NMX_DEV void sc_pps_mem_sums_lane(const ScPpsMemArgs<FID>& a, uint32_t first, uint32_t stride, ScPpsMemAcc<FID>& acc) {
  using F = Fp<FID>;
  const bool wi = a.with_inf != 0;
  for (uint64_t i64 = first; i64 < a.n; i64 += stride) {
    const uint32_t id = (uint32_t)i64;
    const F t0 = ld<FID>(a.t, id), ti0 = ld<FID>(a.tinv, id), w0 = ld<FID>(a.w, id), wi0 = ld<FID>(a.winv, id), ts0 = ld<FID>(a.ts, id);
    F t1 = F::zero(), ti1 = F::zero(), w1 = F::zero(), wi1 = F::zero();
    if (wi) {
      const size_t hi = (size_t)id + a.n;
      t1 = ld<FID>(a.t, hi), ti1 = ld<FID>(a.tinv, hi), w1 = ld<FID>(a.w, hi), wi1 = ld<FID>(a.winv, hi);
    }
    acc.add(a, sc_pps_factor<FID>(a.eqL, a.eqR, a.shift, a.mask, id), wi, t0, t1, ti0, ti1, w0, w1, wi0, wi1, ts0);
  }
  acc.flush();
}
// bind + sums over [0, a.n = len / 4)
template <int FID> NMX_DEV void sc_pps_mem_bind_lane(const ScPpsMemArgs<FID>& a, uint32_t first, uint32_t stride, ScPpsMemAcc<FID>& acc) {
  using F = Fp<FID>;
  for (uint64_t i64 = first; i64 < a.n; i64 += stride) {
    const uint32_t id = (uint32_t)i64;
    F t0, t1, ti0, ti1, w0, w1, wi0, wi1, ts0, ts1;
    sc_pps_bind2<FID>(a.t, a.r, id, a.n, t0, t1);
    sc_pps_bind2<FID>(a.tinv, a.r, id, a.n, ti0, ti1);
    sc_pps_bind2<FID>(a.w, a.r, id, a.n, w0, w1);
    sc_pps_bind2<FID>(a.winv, a.r, id, a.n, wi0, wi1);
    sc_pps_bind2<FID>(a.ts, a.r, id, a.n, ts0, ts1);
    acc.add(a, sc_pps_factor<FID>(a.eqL, a.eqR, a.shift, a.mask, id), true, t0, t1, ti0, ti1, w0, w1, wi0, wi1, ts0);
  }
  acc.flush();
}

// ---- inner group --------------------------------------------------------------------------------------------------------------------
template <int FID> struct ScPpsInnerAcc {  // s[0..2]: sum a b c, sum da db dc, sum a(-1) b(-1) c(-1); s[3]: E's t(0)
  using F = Fp<FID>;
  F s[4];
  uint32_t pending = 0;
  NMX_DEV ScPpsInnerAcc() {
#pragma unroll
    for (int i = 0; i < 4; i++) s[i] = F::zero();
  }
  NMX_DEV void add(const F& fac, bool wi, const F& a0, const F& a1, const F& b0, const F& b1, const F& c0, const F& c1, const F& e0) {
    s[3] = s[3] + e0 * fac;
    if (wi) {
      const F da = F::sub2(a1, a0).norm(), db = F::sub2(b1, b0).norm(), dc = F::sub2(c1, c0).norm();
      const F ma = F::sub2(a0.dbl(), a1).norm(), mb = F::sub2(b0.dbl(), b1).norm(), mc = F::sub2(c0.dbl(), c1).norm();
      dc.check_below(3.01, "ppsnark inner: dc"), mc.check_below(4.01, "ppsnark inner: c(-1)");
      const F dab = da * db, mab = ma * mb;
      dab.check_below(1.08, "ppsnark inner: da db"), mab.check_below(1.13, "ppsnark inner: a(-1) b(-1)");
      s[0] = s[0] + (a0 * b0) * c0, s[1] = s[1] + dab * dc, s[2] = s[2] + mab * mc;
    }
    if (++pending == kScPpsLazy) flush();
  }
  NMX_DEV void flush() {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      s[i] = s[i].norm();
      s[i].check_below(8.0, "ppsnark inner: a lane's lazy sum");
      s[i] = s[i].canon();
    }
    pending = 0;
  }
};
template <int FID> NMX_DEV void sc_pps_inner_sums_lane(const ScPpsInnerArgs<FID>& a, uint32_t first, uint32_t stride, ScPpsInnerAcc<FID>& acc) {
  using F = Fp<FID>;
  const bool wi = a.with_inf != 0;
  for (uint64_t i64 = first; i64 < a.n; i64 += stride) {
    const uint32_t id = (uint32_t)i64;
    const F e0 = ld<FID>(a.e, id);
    F a0 = F::zero(), a1 = a0, b0 = a0, b1 = a0, c0 = a0, c1 = a0;
    if (wi) {
      const size_t hi = (size_t)id + a.n;
      a0 = ld<FID>(a.a, id), a1 = ld<FID>(a.a, hi), b0 = ld<FID>(a.b, id), b1 = ld<FID>(a.b, hi), c0 = ld<FID>(a.c, id), c1 = ld<FID>(a.c, hi);
    }
    acc.add(sc_pps_factor<FID>(a.eqL, a.eqR, a.shift, a.mask, id), wi, a0, a1, b0, b1, c0, c1, e0);
  }
  acc.flush();
}
template <int FID> NMX_DEV void sc_pps_inner_bind_lane(const ScPpsInnerArgs<FID>& a, uint32_t first, uint32_t stride, ScPpsInnerAcc<FID>& acc) {
  using F = Fp<FID>;
  for (uint64_t i64 = first; i64 < a.n; i64 += stride) {
    const uint32_t id = (uint32_t)i64;
    F a0, a1, b0, b1, c0, c1, e0, e1;
    sc_pps_bind2<FID>(a.a, a.r, id, a.n, a0, a1);
    sc_pps_bind2<FID>(a.b, a.r, id, a.n, b0, b1);
    sc_pps_bind2<FID>(a.c, a.r, id, a.n, c0, c1);
    sc_pps_bind2<FID>(a.e, a.r, id, a.n, e0, e1);
    acc.add(sc_pps_factor<FID>(a.eqL, a.eqR, a.shift, a.mask, id), true, a0, a1, b0, b1, c0, c1, e0);
  }
  acc.flush();
}

// ---- witness group ------------------------------------------------------------------------------------------------------------------
template <int FID> struct ScPpsWitAcc {  // s[0]: sum A B; s[1]: sum A(-1) B(-1)
  using F = Fp<FID>;
  F s[2];
  uint32_t pending = 0;
  NMX_DEV ScPpsWitAcc() { s[0] = s[1] = F::zero(); }
  NMX_DEV void add(const F& a0, const F& a1, const F& b0, const F& b1) {
    const F m = F::sub2(a0.dbl(), a1).norm() * F::sub2(b0.dbl(), b1).norm();
    m.check_below(1.13, "ppsnark witness: A(-1) B(-1)");
    s[0] = s[0] + a0 * b0, s[1] = s[1] + m;
    if (++pending == kScPpsLazy) flush();
  }
  NMX_DEV void flush() {
#pragma unroll
    for (int i = 0; i < 2; i++) {
      s[i] = s[i].norm();
      s[i].check_below(8.0, "ppsnark witness: a lane's lazy sum");
      s[i] = s[i].canon();
    }
    pending = 0;
  }
};
template <int FID> NMX_DEV void sc_pps_wit_sums_lane(const ScPpsWitArgs<FID>& a, uint32_t first, uint32_t stride, ScPpsWitAcc<FID>& acc) {
  for (uint64_t i64 = first; i64 < a.n; i64 += stride) {
    const uint32_t id = (uint32_t)i64;
    const size_t hi = (size_t)id + a.n;
    acc.add(ld<FID>(a.w, id), ld<FID>(a.w, hi), ld<FID>(a.m, id), ld<FID>(a.m, hi));
  }
  acc.flush();
}
template <int FID> NMX_DEV void sc_pps_wit_bind_lane(const ScPpsWitArgs<FID>& a, uint32_t first, uint32_t stride, ScPpsWitAcc<FID>& acc) {
  using F = Fp<FID>;
  for (uint64_t i64 = first; i64 < a.n; i64 += stride) {
    const uint32_t id = (uint32_t)i64;
    F a0, a1, b0, b1;
    sc_pps_bind2<FID>(a.w, a.r, id, a.n, a0, a1);
    sc_pps_bind2<FID>(a.m, a.r, id, a.n, b0, b1);
    acc.add(a0, a1, b0, b1);
  }
  acc.flush();
}

// ---- the last device bind over [0, a.n = len / 2), all 16 tables: no sums; the bound (bind = 0: the unchanged) tables also land in the
// staging area.  (The table loop is unrolled: a table chosen by a run-time index would cost a copy of the arguments in scratch.)
template <int FID> NMX_DEV void sc_pps_bind_only_lane(const ScPpsBindArgs<FID>& a, uint32_t first, uint32_t stride) {
  using F = Fp<FID>;
  for (uint64_t i64 = first; i64 < a.n; i64 += stride) {
    const uint32_t id = (uint32_t)i64;
#pragma unroll
    for (uint32_t t = 0; t < kScPpsTables; t++) {
      uint32_t* X = a.X[t];
      F y = ld<FID>(X, id);
      if (a.bind) {
        const F x1 = ld<FID>(X, (size_t)id + a.n);
        y = (y + a.r * F::sub2(x1, y).norm()).norm().canon();
        y.to_words(X + 8 * (size_t)id);
      }
      y.to_words(a.stage + 8 * ((size_t)t * a.n + id));
    }
  }
}

#if defined(__HIPCC__) || defined(__HIP__)
// Launch bounds 256: DESIGN.md ("ppsnark sum-check") has the compiler's register, scratch and occupancy figures.
template <int FID, int J, class ACC> __device__ __forceinline__ void sc_pps_block_out(ACC& acc, uint32_t* lds, uint32_t* partial) {
  block_sum_waves<FID, J, true>(acc.s, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < J; j++) acc.s[j].to_words(partial + 8 * (J * (size_t)blockIdx.x + j));
  }
}
template <int FID> __global__ __launch_bounds__(256) void k_pps_mem_sums(ScPpsMemArgs<FID> a, uint32_t* partial) {
  __shared__ uint32_t lds[36 * 6];
  ScPpsMemAcc<FID> acc;
  sc_pps_mem_sums_lane<FID>(a, blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, acc);
  sc_pps_block_out<FID, 6>(acc, lds, partial);
}
template <int FID> __global__ __launch_bounds__(256) void k_pps_mem_bind_sums(ScPpsMemArgs<FID> a, uint32_t* partial) {
  __shared__ uint32_t lds[36 * 6];
  ScPpsMemAcc<FID> acc;
  sc_pps_mem_bind_lane<FID>(a, blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, acc);
  sc_pps_block_out<FID, 6>(acc, lds, partial);
}
template <int FID> __global__ __launch_bounds__(256) void k_pps_inner_sums(ScPpsInnerArgs<FID> a, uint32_t* partial) {
  __shared__ uint32_t lds[36 * 4];
  ScPpsInnerAcc<FID> acc;
  sc_pps_inner_sums_lane<FID>(a, blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, acc);
  sc_pps_block_out<FID, 4>(acc, lds, partial);
}
template <int FID> __global__ __launch_bounds__(256) void k_pps_inner_bind_sums(ScPpsInnerArgs<FID> a, uint32_t* partial) {
  __shared__ uint32_t lds[36 * 4];
  ScPpsInnerAcc<FID> acc;
  sc_pps_inner_bind_lane<FID>(a, blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, acc);
  sc_pps_block_out<FID, 4>(acc, lds, partial);
}
template <int FID> __global__ __launch_bounds__(256) void k_pps_wit_sums(ScPpsWitArgs<FID> a, uint32_t* partial) {
  __shared__ uint32_t lds[36 * 2];
  ScPpsWitAcc<FID> acc;
  sc_pps_wit_sums_lane<FID>(a, blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, acc);
  sc_pps_block_out<FID, 2>(acc, lds, partial);
}
template <int FID> __global__ __launch_bounds__(256) void k_pps_wit_bind_sums(ScPpsWitArgs<FID> a, uint32_t* partial) {
  __shared__ uint32_t lds[36 * 2];
  ScPpsWitAcc<FID> acc;
  sc_pps_wit_bind_lane<FID>(a, blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, acc);
  sc_pps_block_out<FID, 2>(acc, lds, partial);
}
template <int FID> __global__ __launch_bounds__(256) void k_pps_bind_only(ScPpsBindArgs<FID> a) {
  sc_pps_bind_only_lane<FID>(a, blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u);
}

// the partials of one group: 4096 blocks (sc_blocks_bind's cap) x up to 6 elements; kScPartialBytes is sized for 4
static constexpr size_t kScPpsPartialBytes = (size_t)4096 * 6 * 32;
static constexpr uint32_t kScPpsSlots = 4;  // mailbox slots 0..3: memory row, memory col, inner, witness

// the device side of one proof: the launches over the 16 in-place tables, the context's stream
template <int FID> struct ScPpsDev {
  using F = Fp<FID>;
  using H = HostFp4<FID>;
  using Tables = typename ScEqDev<FID>::Tables;
  using Sums = typename ScPps<FID>::Sums;
  ScDev<FID>& h;
  uint32_t* X[kScPpsTables];
  F nk, one;
  uint32_t* stage;  // behind the four partials areas: 16 x tail_len elements
  uint32_t seq[kScPpsSlots] = {};
  ScPpsDev(ScDev<FID>& h_, void* const* tables) : h(h_), stage((uint32_t*)(h_.c.arena + kScPpsSlots * kScPpsPartialBytes)) {
    for (uint32_t t = 0; t < kScPpsTables; t++) X[t] = (uint32_t*)tables[t];
    F fm = F::zero();  // the form factor as a plain integer, as ScPass<FID, 3>
    if (h.mont) fm = pow2_plain<FID>(256);
    else fm.l[0] = 1;
    one = fm.canon();
    nk = F::sub2(F::zero(), one).norm().canon();
  }
  uint32_t* partial(uint32_t slot) const { return (uint32_t*)(h.c.arena + slot * kScPpsPartialBytes); }
  static uint32_t blocks(uint32_t n) { return sc_blocks_bind(n); }  // one index per lane, at most 4096 blocks (the partials' areas)
  template <int J> void finish(uint32_t slot, uint32_t nblocks) {
    seq[slot] = h.next_seq();
    hipLaunchKernelGGL((k_sum_partials_mail<FID, J, J>), dim3(1), dim3(256), 0, h.c.stream, partial(slot), nblocks, h.slot_dev(slot), seq[slot]);
    HIPCHK(hipGetLastError());
    h.launched(2);
  }
  ScPpsMemArgs<FID> mem_args(uint32_t g, size_t off, const Tables& t, uint32_t n, const F& r, bool with_inf) const {
    uint32_t* const* T = X + 5 * g;
    return ScPpsMemArgs<FID>{T[0] + 8 * off, T[1] + 8 * off, T[2] + 8 * off, T[3] + 8 * off, T[4] + 8 * off, r, nk, one,
                             t.eqL, t.eqR, t.shift, t.mask, n, with_inf ? 1u : 0u};
  }
  ScPpsInnerArgs<FID> inner_args(size_t off, const Tables& t, uint32_t n, const F& r, bool with_inf) const {
    return ScPpsInnerArgs<FID>{X[10] + 8 * off, X[11] + 8 * off, X[12] + 8 * off, X[13] + 8 * off, r, t.eqL, t.eqR, t.shift, t.mask, n, with_inf ? 1u : 0u};
  }
  // the sums pass of memory group g over tables of len elements; high: the t(1) form over the high halves
  void mem_sums(uint32_t g, size_t len, const Tables& t, bool high) {
    const uint32_t n = (uint32_t)(len / 2), nb = blocks(n);
    hipLaunchKernelGGL((k_pps_mem_sums<FID>), dim3(nb), dim3(256), 0, h.c.stream, mem_args(g, high ? len / 2 : 0, t, n, F::zero(), !high), partial(g));
    HIPCHK(hipGetLastError());
    finish<6>(g, nb);
  }
  void inner_sums(size_t len, const Tables& t, bool high) {
    const uint32_t n = (uint32_t)(len / 2), nb = blocks(n);
    hipLaunchKernelGGL((k_pps_inner_sums<FID>), dim3(nb), dim3(256), 0, h.c.stream, inner_args(high ? len / 2 : 0, t, n, F::zero(), !high), partial(2));
    HIPCHK(hipGetLastError());
    finish<4>(2, nb);
  }
  // round 1: the 18 sums over the tables as they are (tR: eq(rhos)'s tables of the round, tO: eq(r_outer)'s)
  void sums(size_t len, const Tables& tR, const Tables& tO) {
    mem_sums(0, len, tR, false), mem_sums(1, len, tR, false), inner_sums(len, tO, false);
    const uint32_t n = (uint32_t)(len / 2), nb = blocks(n);
    hipLaunchKernelGGL((k_pps_wit_sums<FID>), dim3(nb), dim3(256), 0, h.c.stream, ScPpsWitArgs<FID>{X[14], X[15], F::zero(), n}, partial(3));
    HIPCHK(hipGetLastError());
    finish<2>(3, nb);
  }
  // bind the 16 tables (len elements, len >= 4) with r in place and take the next round's sums (its eq tables: tR, tO)
  void bind_sums(size_t len, const H& r, const Tables& tR, const Tables& tO) {
    const F rd = r.to_device();
    const uint32_t n = (uint32_t)(len / 4), nb = blocks(n);
    for (uint32_t g = 0; g < 2; g++) {
      hipLaunchKernelGGL((k_pps_mem_bind_sums<FID>), dim3(nb), dim3(256), 0, h.c.stream, mem_args(g, 0, tR, n, rd, true), partial(g));
      HIPCHK(hipGetLastError());
      finish<6>(g, nb);
    }
    hipLaunchKernelGGL((k_pps_inner_bind_sums<FID>), dim3(nb), dim3(256), 0, h.c.stream, inner_args(0, tO, n, rd, true), partial(2));
    HIPCHK(hipGetLastError());
    finish<4>(2, nb);
    hipLaunchKernelGGL((k_pps_wit_bind_sums<FID>), dim3(nb), dim3(256), 0, h.c.stream, ScPpsWitArgs<FID>{X[14], X[15], rd, n}, partial(3));
    HIPCHK(hipGetLastError());
    finish<2>(3, nb);
  }
  // the pending sums of the four groups as elements
  Sums collect(const Tables& tR, const Tables& tO) {
    Sums s;
    const uint32_t fR = 3u + (tR.eqL ? 1u : 0u), fO = 2u + (tO.eqL ? 1u : 0u);
    for (uint32_t g = 0; g < 2; g++) {
      const uint32_t* res = h.wait(g, seq[g]);
      s.lin[g][0] = h.raw(res, 1), s.lin[g][1] = h.raw(res + 8, 1);
      for (uint32_t w = 0; w < 2; w++) s.mem[g][w][0] = h.raw(res + 16 + 16 * w, fR), s.mem[g][w][1] = h.raw(res + 24 + 16 * w, fR);
    }
    const uint32_t* res = h.wait(2, seq[2]);
    for (uint32_t i = 0; i < 3; i++) s.cub[i] = h.raw(res + 8 * i, 3);
    s.e_t0 = h.raw(res + 24, fO);
    res = h.wait(3, seq[3]);
    s.wit[0] = h.raw(res, 2), s.wit[1] = h.raw(res + 8, 2);
    return s;
  }
  // t(1) of derived claim d (ScPps::round_poly) over tables of len elements: one more pass over the group's high halves.  Both claims
  // of a memory group come from one pass (cache).
  bool have_t1[3] = {false, false, false};
  H t1_val[ScPps<FID>::kDerived];
  void new_round() { have_t1[0] = have_t1[1] = have_t1[2] = false; }
  H t1(uint32_t d, size_t len, const Tables& tR, const Tables& tO) {
    const uint32_t g = d / 2;  // 0, 1: the memory groups; 2: inner
    if (!have_t1[g]) {
      if (g < 2) {
        mem_sums(g, len, tR, true);
        const uint32_t* res = h.wait(g, seq[g]);
        const uint32_t fR = 3u + (tR.eqL ? 1u : 0u);
        t1_val[2 * g] = h.raw(res + 16, fR), t1_val[2 * g + 1] = h.raw(res + 32, fR);
      } else {
        inner_sums(len, tO, true);
        t1_val[4] = h.raw(h.wait(2, seq[2]) + 24, 2u + (tO.eqL ? 1u : 0u));
      }
      have_t1[g] = true;
    }
    return t1_val[d];
  }
  // the hand-over: bind with r (rp == nullptr: no bind) and bring the 16 tables of `half` elements to the host
  void to_host(size_t half, const H* rp, std::vector<H>* T) {
    require(half >= 1 && half <= kTailMax, NMX_E_HIP, "sum-check: tail hand-over out of range");
    ScPpsBindArgs<FID> a;
    for (uint32_t t = 0; t < kScPpsTables; t++) a.X[t] = X[t];
    a.r = rp ? rp->to_device() : F::zero();
    a.stage = stage, a.n = (uint32_t)half, a.bind = rp ? 1u : 0u;
    hipLaunchKernelGGL((k_pps_bind_only<FID>), dim3(blocks(a.n)), dim3(256), 0, h.c.stream, a);
    HIPCHK(hipGetLastError());
    h.launched();
    std::vector<uint32_t> land((size_t)kScPpsTables * half * 8);
    HIPCHK(hipMemcpyAsync(land.data(), stage, land.size() * 4, hipMemcpyDeviceToHost, h.c.stream));
    stream_wait(h.c.stream);
    for (uint32_t t = 0; t < kScPpsTables; t++) {
      T[t].resize(half);
      const uint32_t* src = land.data() + 8 * ((size_t)t * half);
      for (size_t x = 0; x < half; x++) T[t][x] = h.stored(src + 8 * x);
    }
  }
};

// RelaxedR1CSSNARK::prove_helper (ppsnark.rs:886-983).  Of the sc_* options only sc_host_tail and sc_poll_us apply.
template <int FID>
static void sc_prove_ppsnark_t(Ctx& c, size_t num_rounds, void* const* tables, const void* rhos, const void* r_outer, const void* claims2,
                               const void* coeffs9, uint32_t flags, TranscriptFn cb, void* cb_ctx, uint8_t* out_polys, uint8_t* out_r,
                               uint8_t* out_finals) {
  using H = HostFp4<FID>;
  const auto T0 = std::chrono::steady_clock::now();
  const uint32_t l = (uint32_t)num_rounds;
  try {
    ScDev<FID> h(c, flags);
    try {
      // every scalar is read (and range-checked) before anything is launched (the C entry point has checked them already, before it
      // leased a device; this layer does not rely on that)
      ScPps<FID> st;
      st.init(h.alg, rhos, r_outer, claims2, coeffs9, l);
      size_t len = (size_t)1 << l;
      arena_reserve(c, kScPpsSlots * kScPpsPartialBytes + pad256((size_t)kScPpsTables * kTailMax * 32) + 512);
      ScEqDev<FID> eqR, eqO;
      if (len > h.tail_len) {
        const size_t hb = pad256(ScEqDev<FID>::heap_bytes(l));
        aux_reserve(c, 2 * hb);
        eqR.init(h, st.eq[0], c.aux);
        eqO.init(h, st.eq[4], c.aux + hb);
      }
      ScPpsDev<FID> dev(h, tables);
      std::vector<H> hT[kScPpsTables];
      uint32_t j = 1;
      if (len <= h.tail_len) {
        dev.to_host(len, nullptr, hT);  // the whole instance fits the tail
      } else {
        typename ScEqDev<FID>::Tables tR = eqR.tables(1), tO = eqO.tables(1);
        dev.sums(len, tR, tO);
        for (;; j++) {
          const typename ScPps<FID>::Sums s = dev.collect(tR, tO);
          dev.new_round();
          H co[4];
          st.round_poly(s, [&](uint32_t d) { return dev.t1(d, len, tR, tO); }, co);
          const H r = h.ask(cb, cb_ctx, co, 4, out_polys ? out_polys + 128 * (size_t)(j - 1) : nullptr, out_r ? out_r + 32 * (size_t)(j - 1) : nullptr);
          st.bound(co, r);
          h.prof.rounds++;
          if (len / 2 <= h.tail_len) {  // the last device bind: no sums, the bound tables go to the host
            dev.to_host(len / 2, &r, hT);
            len /= 2;
            j++;
            break;
          }
          tR = eqR.tables(j + 1), tO = eqO.tables(j + 1);
          dev.bind_sums(len, r, tR, tO);
          len /= 2;
        }
      }
      if (j <= l) {
        h.prof.host_rounds += l - j + 1;
        sc_tail_rounds_ppsnark<FID>(h.alg, st, l, j, hT, cb, cb_ctx, out_polys, out_r);
      }
      if (out_finals)
        for (uint32_t t = 0; t < kScPpsTables; t++) h.alg.out(hT[t][0], out_finals + 32 * t);
      stream_wait(c.stream);  // the (partly bound) tables are the caller's again
      h.finish_profile(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count());
    } catch (...) {
      h.sync_all_quiet();  // whatever failed: no kernel of this call still writes the tables
      throw;
    }
  } catch (const ScFail& f) {
    rethrow(f);
  }
}

void fv_sumcheck_prove_ppsnark(Ctx& c, int field, size_t num_rounds, void* const* tables, const void* rhos, const void* r_outer,
                               const void* claims2, const void* coeffs9, uint32_t flags, TranscriptFn cb, void* cb_ctx, uint8_t* out_polys,
                               uint8_t* out_r, uint8_t* out_finals) {
  with_field(field, [&](auto F) { sc_prove_ppsnark_t<F()>(c, num_rounds, tables, rhos, r_outer, claims2, coeffs9, flags, cb, cb_ctx, out_polys, out_r, out_finals); });
}
#endif

}  // namespace nmx
