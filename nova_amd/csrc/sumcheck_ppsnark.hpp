// sumcheck_ppsnark.hpp -- ppsnark's batched inner sum-check as ONE C call (nmx_sumcheck_prove_ppsnark).  Included by sumcheck.hip
// behind sumcheck_inplace.hpp, whose passes, kernel, hand-over and round loop it fills in; the host algebra is sc_host.hpp's ScPps.
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
// Three pass kinds (sumcheck_inplace.hpp) per group.  The sums pass pointed at the HIGH halves with with_inf = 0 gives t(1) of the claims
// under an eq whose tau is zero (t(0)'s summand alone, reading X[id] only): the fallback's third sum, t(-1) = 2 t(inf) + 2 t(0) - t(1), or
// 2 t(0) - t(1) for E.  (The witness group has no eq and no such form.)  The last device bind is ONE kernel over all 16 tables.
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

#include "sumcheck_inplace.hpp"

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
    acc.add(a, sc_eq_factor<FID>(a.eqL, a.eqR, a.shift, a.mask, id), wi, t0, t1, ti0, ti1, w0, w1, wi0, wi1, ts0);
  }
  acc.flush();
}
// bind + sums over [0, a.n = len / 4)
template <int FID> NMX_DEV void sc_pps_mem_bind_lane(const ScPpsMemArgs<FID>& a, uint32_t first, uint32_t stride, ScPpsMemAcc<FID>& acc) {
  using F = Fp<FID>;
  for (uint64_t i64 = first; i64 < a.n; i64 += stride) {
    const uint32_t id = (uint32_t)i64;
    F t0, t1, ti0, ti1, w0, w1, wi0, wi1, ts0, ts1;
    sc_bind2<FID>(a.t, a.r, id, a.n, t0, t1);
    sc_bind2<FID>(a.tinv, a.r, id, a.n, ti0, ti1);
    sc_bind2<FID>(a.w, a.r, id, a.n, w0, w1);
    sc_bind2<FID>(a.winv, a.r, id, a.n, wi0, wi1);
    sc_bind2<FID>(a.ts, a.r, id, a.n, ts0, ts1);
    acc.add(a, sc_eq_factor<FID>(a.eqL, a.eqR, a.shift, a.mask, id), true, t0, t1, ti0, ti1, w0, w1, wi0, wi1, ts0);
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
    acc.add(sc_eq_factor<FID>(a.eqL, a.eqR, a.shift, a.mask, id), wi, a0, a1, b0, b1, c0, c1, e0);
  }
  acc.flush();
}
template <int FID> NMX_DEV void sc_pps_inner_bind_lane(const ScPpsInnerArgs<FID>& a, uint32_t first, uint32_t stride, ScPpsInnerAcc<FID>& acc) {
  using F = Fp<FID>;
  for (uint64_t i64 = first; i64 < a.n; i64 += stride) {
    const uint32_t id = (uint32_t)i64;
    F a0, a1, b0, b1, c0, c1, e0, e1;
    sc_bind2<FID>(a.a, a.r, id, a.n, a0, a1);
    sc_bind2<FID>(a.b, a.r, id, a.n, b0, b1);
    sc_bind2<FID>(a.c, a.r, id, a.n, c0, c1);
    sc_bind2<FID>(a.e, a.r, id, a.n, e0, e1);
    acc.add(sc_eq_factor<FID>(a.eqL, a.eqR, a.shift, a.mask, id), true, a0, a1, b0, b1, c0, c1, e0);
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
    sc_bind2<FID>(a.w, a.r, id, a.n, a0, a1);
    sc_bind2<FID>(a.m, a.r, id, a.n, b0, b1);
    acc.add(a0, a1, b0, b1);
  }
  acc.flush();
}

// ---- the six sums-bearing lane bodies as passes of k_sc_sums ---------------------------------------------------------------------------
template <int FID> struct ScPpsMemSums {
  using Args = ScPpsMemArgs<FID>;
  using Acc = ScPpsMemAcc<FID>;
  static constexpr int J = 6;
  static NMX_DEV void lane(const Args& a, uint32_t first, uint32_t stride, Acc& acc) { sc_pps_mem_sums_lane<FID>(a, first, stride, acc); }
};
template <int FID> struct ScPpsMemBindSums {
  using Args = ScPpsMemArgs<FID>;
  using Acc = ScPpsMemAcc<FID>;
  static constexpr int J = 6;
  static NMX_DEV void lane(const Args& a, uint32_t first, uint32_t stride, Acc& acc) { sc_pps_mem_bind_lane<FID>(a, first, stride, acc); }
};
template <int FID> struct ScPpsInnerSums {
  using Args = ScPpsInnerArgs<FID>;
  using Acc = ScPpsInnerAcc<FID>;
  static constexpr int J = 4;
  static NMX_DEV void lane(const Args& a, uint32_t first, uint32_t stride, Acc& acc) { sc_pps_inner_sums_lane<FID>(a, first, stride, acc); }
};
template <int FID> struct ScPpsInnerBindSums {
  using Args = ScPpsInnerArgs<FID>;
  using Acc = ScPpsInnerAcc<FID>;
  static constexpr int J = 4;
  static NMX_DEV void lane(const Args& a, uint32_t first, uint32_t stride, Acc& acc) { sc_pps_inner_bind_lane<FID>(a, first, stride, acc); }
};
template <int FID> struct ScPpsWitSums {
  using Args = ScPpsWitArgs<FID>;
  using Acc = ScPpsWitAcc<FID>;
  static constexpr int J = 2;
  static NMX_DEV void lane(const Args& a, uint32_t first, uint32_t stride, Acc& acc) { sc_pps_wit_sums_lane<FID>(a, first, stride, acc); }
};
template <int FID> struct ScPpsWitBindSums {
  using Args = ScPpsWitArgs<FID>;
  using Acc = ScPpsWitAcc<FID>;
  static constexpr int J = 2;
  static NMX_DEV void lane(const Args& a, uint32_t first, uint32_t stride, Acc& acc) { sc_pps_wit_bind_lane<FID>(a, first, stride, acc); }
};

// ---- the last device bind over [0, a.n = len / 2), all 16 tables: no sums; the bound (bind = 0: the unchanged) tables also land in the
// staging area.  (The table loop is unrolled: a table chosen by a run-time index would cost a copy of the arguments in scratch.)
template <int FID> NMX_DEV void sc_pps_bind_only_lane(const ScPpsBindArgs<FID>& a, uint32_t first, uint32_t stride) {
  for (uint64_t i64 = first; i64 < a.n; i64 += stride) {
    const uint32_t id = (uint32_t)i64;
#pragma unroll
    for (uint32_t t = 0; t < kScPpsTables; t++) sc_bind_stage_one<FID>(a.X[t], a.r, a.n, a.bind, a.stage, t, id);
  }
}

#if defined(__HIPCC__) || defined(__HIP__)
template <int FID> __global__ __launch_bounds__(256) void k_pps_bind_only(ScPpsBindArgs<FID> a) {
  sc_pps_bind_only_lane<FID>(a, blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u);
}

// the partials of one group: 4096 blocks (sc_blocks_bind's cap) x up to 6 elements; kScPartialBytes is sized for 4
static constexpr size_t kScPpsPartialBytes = (size_t)4096 * 6 * 32;
static constexpr uint32_t kScPpsSlots = 4;  // mailbox slots 0..3: memory row, memory col, inner, witness

// the device side of one proof: the launches over the 16 in-place tables; the arena holds the four partials areas, then the staging
// area of 16 x tail_len elements
template <int FID> struct ScPpsDev : ScInplaceDev<FID> {
  using Base = ScInplaceDev<FID>;
  using typename Base::F;
  using typename Base::H;
  using typename Base::Tables;
  using Base::h;
  using Sums = typename ScPps<FID>::Sums;
  uint32_t* X[kScPpsTables];
  uint32_t seq[kScPpsSlots] = {};
  ScPpsDev(ScDev<FID>& h_, void* const* tables) : Base(h_, kScPpsSlots * kScPpsPartialBytes) {
    for (uint32_t t = 0; t < kScPpsTables; t++) X[t] = (uint32_t*)tables[t];
  }
  template <class P> void pass(uint32_t slot, const typename P::Args& a) {
    seq[slot] = this->template launch_pass<P>(slot, (uint32_t*)(h.c.arena + slot * kScPpsPartialBytes), a);
  }
  ScPpsMemArgs<FID> mem_args(uint32_t g, size_t off, const Tables& t, uint32_t n, const F& r, bool with_inf) const {
    uint32_t* const* T = X + 5 * g;
    return ScPpsMemArgs<FID>{T[0] + 8 * off, T[1] + 8 * off, T[2] + 8 * off, T[3] + 8 * off, T[4] + 8 * off, r, this->nk, this->one,
                             t.eqL, t.eqR, t.shift, t.mask, n, with_inf ? 1u : 0u};
  }
  ScPpsInnerArgs<FID> inner_args(size_t off, const Tables& t, uint32_t n, const F& r, bool with_inf) const {
    return ScPpsInnerArgs<FID>{X[10] + 8 * off, X[11] + 8 * off, X[12] + 8 * off, X[13] + 8 * off, r, t.eqL, t.eqR, t.shift, t.mask, n, with_inf ? 1u : 0u};
  }
  // the sums pass of memory group g over tables of len elements; high: the t(1) form over the high halves
  void mem_sums(uint32_t g, size_t len, const Tables& t, bool high) {
    pass<ScPpsMemSums<FID>>(g, mem_args(g, high ? len / 2 : 0, t, (uint32_t)(len / 2), F::zero(), !high));
  }
  void inner_sums(size_t len, const Tables& t, bool high) {
    pass<ScPpsInnerSums<FID>>(2, inner_args(high ? len / 2 : 0, t, (uint32_t)(len / 2), F::zero(), !high));
  }
  // round 1: the 18 sums over the tables as they are (tR: eq(rhos)'s tables of the round, tO: eq(r_outer)'s)
  void sums(size_t len, const Tables& tR, const Tables& tO) {
    mem_sums(0, len, tR, false), mem_sums(1, len, tR, false), inner_sums(len, tO, false);
    pass<ScPpsWitSums<FID>>(3, ScPpsWitArgs<FID>{X[14], X[15], F::zero(), (uint32_t)(len / 2)});
  }
  // bind the 16 tables (len elements, len >= 4) with r in place and take the next round's sums (its eq tables: tR, tO)
  void bind_sums(size_t len, const H& r, const Tables& tR, const Tables& tO) {
    const F rd = r.to_device();
    const uint32_t n = (uint32_t)(len / 4);
    for (uint32_t g = 0; g < 2; g++) pass<ScPpsMemBindSums<FID>>(g, mem_args(g, 0, tR, n, rd, true));
    pass<ScPpsInnerBindSums<FID>>(2, inner_args(0, tO, n, rd, true));
    pass<ScPpsWitBindSums<FID>>(3, ScPpsWitArgs<FID>{X[14], X[15], rd, n});
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
  void to_host(size_t half, const H* rp, std::vector<H>* T) {
    Base::to_host(
        half, rp, kScPpsTables,
        [&](const F& r, uint32_t n, uint32_t bind) {
          ScPpsBindArgs<FID> a;
          for (uint32_t t = 0; t < kScPpsTables; t++) a.X[t] = X[t];
          a.r = r, a.stage = this->stage, a.n = n, a.bind = bind;
          hipLaunchKernelGGL((k_pps_bind_only<FID>), dim3(Base::blocks(n)), dim3(256), 0, h.c.stream, a);
        },
        [&](uint32_t t) -> std::vector<H>& { return T[t]; });
  }
};

// RelaxedR1CSSNARK::prove_helper (ppsnark.rs:886-983) as a prover of sc_prove_inplace
template <int FID> struct ScPpsProver {
  using H = HostFp4<FID>;
  void* const* tables;
  const void *rhos, *r_outer, *claims2, *coeffs9;
  TranscriptFn cb;
  void* cb_ctx;
  uint8_t *out_polys, *out_r, *out_finals;
  ScPps<FID> st;
  ScEqDev<FID> eqR, eqO;
  std::optional<ScPpsDev<FID>> dev;
  std::vector<H> hT[kScPpsTables];
  typename ScEqDev<FID>::Tables tR, tO;  // of the round the pending sums belong to

  void read_scalars(const ScAlg<FID>& alg, uint32_t l) { st.init(alg, rhos, r_outer, claims2, coeffs9, l); }
  void reserve(ScDev<FID>& h, uint32_t l, bool device_rounds) {
    arena_reserve(h.c, kScPpsSlots * kScPpsPartialBytes + pad256((size_t)kScPpsTables * kTailMax * 32) + 512);
    if (device_rounds) {
      const size_t hb = pad256(ScEqDev<FID>::heap_bytes(l));
      aux_reserve(h.c, 2 * hb);
      eqR.init(h, st.eq[0], h.c.aux);
      eqO.init(h, st.eq[4], h.c.aux + hb);
    }
    dev.emplace(h, tables);
  }
  void first_sums(size_t len) {
    tR = eqR.tables(1), tO = eqO.tables(1);
    dev->sums(len, tR, tO);
  }
  void round_poly(size_t len, H* co) {
    const typename ScPps<FID>::Sums s = dev->collect(tR, tO);
    dev->new_round();
    st.round_poly(s, [&](uint32_t d) { return dev->t1(d, len, tR, tO); }, co);
  }
  void bound(const H* co, const H& r) { st.bound(co, r); }
  void bind_sums(size_t len, const H& r, uint32_t next) {
    tR = eqR.tables(next), tO = eqO.tables(next);
    dev->bind_sums(len, r, tR, tO);
  }
  void to_host(size_t half, const H* rp) { dev->to_host(half, rp, hT); }
  void host_tail(const ScAlg<FID>& alg, uint32_t l, uint32_t j) { sc_tail_rounds_ppsnark<FID>(alg, st, l, j, hT, cb, cb_ctx, out_polys, out_r); }
  void outputs(const ScAlg<FID>& alg) {
    if (out_finals)
      for (uint32_t t = 0; t < kScPpsTables; t++) alg.out(hT[t][0], out_finals + 32 * t);
  }
};

void fv_sumcheck_prove_ppsnark(Ctx& c, int field, size_t num_rounds, void* const* tables, const void* rhos, const void* r_outer,
                               const void* claims2, const void* coeffs9, uint32_t flags, TranscriptFn cb, void* cb_ctx, uint8_t* out_polys,
                               uint8_t* out_r, uint8_t* out_finals) {
  with_field(field, [&](auto F) {
    ScPpsProver<F()> p{tables, rhos, r_outer, claims2, coeffs9, cb, cb_ctx, out_polys, out_r, out_finals};
    sc_prove_inplace<F()>(c, flags, num_rounds, p);
  });
}
#endif

}  // namespace nmx
