// sumcheck_batched.hpp -- SumcheckProof::prove_batched_cubic as ONE C call (nmx_sumcheck_prove_batched_cubic).  Included by
// sumcheck.hip behind sumcheck_inplace.hpp, whose passes, kernel, hand-over and round loop it fills in.
//
//   prove_batched_cubic                                               src/spartan/sumcheck.rs:509-577
//   evaluation_points_batched_cubic / fallback_eval_inf_batched_cubic src/spartan/sumcheck.rs:749-894
//
//   sum_x eq(tau, x) * sum_i alpha_i (A_i(x) B_i(x) - C_i(x)) = claim      for K <= 16 triples under one sum-check
//
// Both sums-bearing passes loop over the K triples inside the index (the eq factor is applied once per index, not once per triple, as the
// reference does) and leave (t(0), t(inf)) of a round.  The sums pass pointed at the high halves with with_inf = 0 gives t(1) of a round
// whose tau is zero: t(-1) = 2 t(inf) + 2 t(0) - t(1) (the fallback's third sum).  Everything goes through mailbox slot 0.
//
// Bytes per index of the bind + sums pass: 12 K loads + 6 K stores of 32 B (576 K B) plus the eq reads (32 B, 64 B in the first
// half of the rounds); the sums pass reads 5 K x 32 B (3 K for the t(1) form).
//
// Powers of R' = 2^261 (fp.hpp: a product of two stored words x~ y~ comes out as x~ y~ / R').  With Fm the vectors' form factor
// (1 canonical, 2^256 Montgomery) and nk = p - Fm:
//   e_i  = mul_add(a0, b0, c0, nk)          = (a b - c)            Fm^2 / R'
//   q_i  = (a1 - a0) * (b1 - b0)            = (da db)              Fm^2 / R'
//   the alphas arrive as alpha_i R' (HostFp4::to_device: the internal residue), so alpha_i * e_i = alpha_i (a b - c) Fm^2 / R':
//   the weighted sum carries exactly the power ONE triple carries in the cubic prover, in both layouts;
//   times the eq factor (stored: Fm / R' each): a sum is x Fm^3 / R'^2 without eqL, x Fm^4 / R'^3 with it -- three / four stored
//   factors in ScDev::raw's count, the same as ScPass<FID, 3>::factors.
#pragma once

#include "sumcheck_inplace.hpp"

namespace nmx {

static constexpr uint32_t kScBatchedMaxK = 16;  // triples per call: pointers and alphas travel by value in the kernel arguments

template <int FID> struct ScBatchedArgs {  // POD, ~1.1 KB
  uint32_t* A[kScBatchedMaxK];
  uint32_t* B[kScBatchedMaxK];
  uint32_t* C[kScBatchedMaxK];
  Fp<FID> alpha[kScBatchedMaxK];  // alpha_i R', canonical
  Fp<FID> r, nk;                  // the challenge (internal form, canonical); p - Fm
  const uint32_t *eqL, *eqR;      // ScEqDev::tables of the round the sums belong to
  uint32_t* stage;                // bind only: table t of the 3 k (A_0, B_0, C_0, A_1, ...) at element t * n
  uint32_t shift, mask, k;
  uint32_t n;                     // indices of the pass: len / 2 (sums, bind only) or len / 4 (bind + sums)
  uint32_t with_inf;              // sums: 1 = t(0) and t(inf); 0 = t(0) alone, reading X[id] only
  uint32_t bind;                  // bind only: 0 = the tables go to the staging area as they are
};

// The alpha-weighted terms of one index, lazily added.  Limb bound: every product is normalised (limbs < 2^29) and < 1.08 p
// (operands: alpha < p, e_i < 1.02 p, q_i < 1.08 p from differences < 3 p); an accumulator is normalised after every 6 additions,
// so it never holds more than 1 normalised + 6 fresh terms: limbs < 7 * 2^29 < 2^32 - 2^4, what norm() takes.  Its VALUE is not
// reduced inside the index: 16 terms stay below 16 * 1.01 p < 16.2 p, and 16.2 p * (factor < 1.01 p) < 127 p^2 is within what a
// product takes -- so the factor multiply is the index's only reduction.  (All tables and alphas p - 1 at k = 16: tests/.)
template <int FID> struct ScBatchedAcc {
  using F = Fp<FID>;
  F e = F::zero(), q = F::zero();
  uint32_t pending = 0;
  NMX_DEV void add(const F& alpha, const F& a0, const F& a1, const F& b0, const F& b1, const F& c0, const F& nk, bool with_inf) {
    e = e + alpha * F::mul_add(a0, b0, c0, nk);  // a0 b0 - c0 Fm in one reduction (nk = p - Fm), < 1.02 p
    if (with_inf) q = q + alpha * (F::sub2(a1, a0).norm() * F::sub2(b1, b0).norm());
    if (++pending == 6) {
      e = e.norm(), q = q.norm();
      pending = 0;
    }
  }
};
// one index's two terms into the lane's sums: s += (sum_i ...) * factor, each < p (1 + 16.4 / 127) < 1.13 p; a lane's sum is
// brought back below p after every 6 of them (1 + 6 * 1.13 < 8 p, limbs < 7 * 2^29)
template <int FID>
NMX_DEV void sc_batched_fold(const ScBatchedAcc<FID>& t, const Fp<FID>& fac, bool with_inf, Fp<FID>& s0, Fp<FID>& s1, uint32_t& pending) {
  const Fp<FID> e = t.e.norm(), q = t.q.norm();
  e.check_below(16.2, "batched cubic: t(0) terms of one index");
  q.check_below(16.2, "batched cubic: t(inf) terms of one index");
  s0 = s0 + e * fac;
  if (with_inf) s1 = s1 + q * fac;
  if (++pending == 6) {
    s0 = s0.norm().canon();
    s1 = s1.norm().canon();
    pending = 0;
  }
}

// ---- the sums pass: indices first, first + stride, ... of [0, a.n = len / 2); on return s0 / s1 are canonical ------------------------
template <int FID> NMX_DEV void sc_batched_sums_lane(const ScBatchedArgs<FID>& a, uint32_t first, uint32_t stride, Fp<FID>& s0, Fp<FID>& s1) {
  using F = Fp<FID>;
  const bool wi = a.with_inf != 0;
  uint32_t pending = 0;
  for (uint64_t i64 = first; i64 < a.n; i64 += stride) {
    const uint32_t id = (uint32_t)i64;
    ScBatchedAcc<FID> t;
    for (uint32_t i = 0; i < a.k; i++) {
      const F a0 = ld<FID>(a.A[i], id), b0 = ld<FID>(a.B[i], id), c0 = ld<FID>(a.C[i], id);
      F a1 = F::zero(), b1 = F::zero();
      if (wi) a1 = ld<FID>(a.A[i], (size_t)id + a.n), b1 = ld<FID>(a.B[i], (size_t)id + a.n);
      t.add(a.alpha[i], a0, a1, b0, b1, c0, a.nk, wi);
    }
    sc_batched_fold<FID>(t, sc_eq_factor<FID>(a.eqL, a.eqR, a.shift, a.mask, id), wi, s0, s1, pending);
  }
  s0 = s0.norm().canon();
  s1 = s1.norm().canon();
}
// ---- the bind + sums pass over [0, a.n = len / 4) ------------------------------------------------------------------------------------
template <int FID> NMX_DEV void sc_batched_bind_lane(const ScBatchedArgs<FID>& a, uint32_t first, uint32_t stride, Fp<FID>& s0, Fp<FID>& s1) {
  using F = Fp<FID>;
  uint32_t pending = 0;
  for (uint64_t i64 = first; i64 < a.n; i64 += stride) {
    const uint32_t id = (uint32_t)i64;
    ScBatchedAcc<FID> t;
    for (uint32_t i = 0; i < a.k; i++) {
      F a0, a1, b0, b1, c0, c1;
      sc_bind2<FID>(a.A[i], a.r, id, a.n, a0, a1);
      sc_bind2<FID>(a.B[i], a.r, id, a.n, b0, b1);
      sc_bind2<FID>(a.C[i], a.r, id, a.n, c0, c1);
      t.add(a.alpha[i], a0, a1, b0, b1, c0, a.nk, true);
    }
    sc_batched_fold<FID>(t, sc_eq_factor<FID>(a.eqL, a.eqR, a.shift, a.mask, id), true, s0, s1, pending);
  }
  s0 = s0.norm().canon();
  s1 = s1.norm().canon();
}
// the two as passes of k_sc_sums: a lane's two running sums are the pass's s[2] (s[0] t(0)'s, s[1] t(inf)'s)
template <int FID> struct ScBatchedLaneAcc {
  Fp<FID> s[2] = {Fp<FID>::zero(), Fp<FID>::zero()};
};
template <int FID> struct ScBatchedSums {
  using Args = ScBatchedArgs<FID>;
  using Acc = ScBatchedLaneAcc<FID>;
  static constexpr int J = 2;
  static NMX_DEV void lane(const Args& a, uint32_t first, uint32_t stride, Acc& acc) { sc_batched_sums_lane<FID>(a, first, stride, acc.s[0], acc.s[1]); }
};
template <int FID> struct ScBatchedBindSums {
  using Args = ScBatchedArgs<FID>;
  using Acc = ScBatchedLaneAcc<FID>;
  static constexpr int J = 2;
  static NMX_DEV void lane(const Args& a, uint32_t first, uint32_t stride, Acc& acc) { sc_batched_bind_lane<FID>(a, first, stride, acc.s[0], acc.s[1]); }
};
// ---- the last device bind over [0, a.n = len / 2) (len == 2 included: one lane) --------------------------------------------------------
template <int FID> NMX_DEV void sc_batched_bind_only_lane(const ScBatchedArgs<FID>& a, uint32_t first, uint32_t stride) {
  for (uint64_t i64 = first; i64 < a.n; i64 += stride) {
    const uint32_t id = (uint32_t)i64;
    for (uint32_t i = 0; i < a.k; i++) {  // (one array per statement: a table chosen by a run-time index into {A, B, C} costs a copy of the arguments in scratch)
      sc_bind_stage_one<FID>(a.A[i], a.r, a.n, a.bind, a.stage, 3 * i, id);
      sc_bind_stage_one<FID>(a.B[i], a.r, a.n, a.bind, a.stage, 3 * i + 1, id);
      sc_bind_stage_one<FID>(a.C[i], a.r, a.n, a.bind, a.stage, 3 * i + 2, id);
    }
  }
}

#if defined(__HIPCC__) || defined(__HIP__)
template <int FID> __global__ __launch_bounds__(256) void k_scb_bind_only(ScBatchedArgs<FID> a) {
  sc_batched_bind_only_lane<FID>(a, blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u);
}

// the device side of one proof: the launches over the 3 k in-place tables; the arena holds kScPartialBytes of partials, then the
// staging area of 3 k x tail_len elements
template <int FID> struct ScBatchedDev : ScInplaceDev<FID> {
  using Base = ScInplaceDev<FID>;
  using typename Base::F;
  using typename Base::H;
  using typename Base::Tables;
  ScBatchedArgs<FID> base{};
  uint32_t k;
  uint32_t* partial;
  ScBatchedDev(ScDev<FID>& h_, void* const* As, void* const* Bs, void* const* Cs, const std::vector<H>& alphas)
      : Base(h_, kScPartialBytes), k((uint32_t)alphas.size()), partial((uint32_t*)h_.c.arena) {
    for (uint32_t i = 0; i < kScBatchedMaxK; i++) {
      base.A[i] = i < k ? (uint32_t*)As[i] : nullptr, base.B[i] = i < k ? (uint32_t*)Bs[i] : nullptr, base.C[i] = i < k ? (uint32_t*)Cs[i] : nullptr;
      base.alpha[i] = i < k ? alphas[i].to_device() : F::zero();
    }
    base.nk = this->nk;
    base.r = F::zero(), base.eqL = base.eqR = nullptr, base.stage = this->stage;
    base.shift = 0, base.mask = 0xffffffffu, base.k = k, base.n = 0, base.with_inf = 1, base.bind = 0;
  }
  static uint32_t factors(const Tables& t) { return 3u + (t.eqL ? 1u : 0u); }
  // (t(0), t(inf)) over tables of len elements; high = true: t(0)'s sum alone over the HIGH halves, which is t(1)
  uint32_t sums(size_t len, const Tables& t, bool high) {
    ScBatchedArgs<FID> a = base;
    const size_t half = len / 2;
    if (high)
      for (uint32_t i = 0; i < k; i++) a.A[i] += 8 * half, a.B[i] += 8 * half, a.C[i] += 8 * half;
    a.eqL = t.eqL, a.eqR = t.eqR, a.shift = t.shift, a.mask = t.mask, a.n = (uint32_t)half, a.with_inf = high ? 0u : 1u;
    return this->template launch_pass<ScBatchedSums<FID>>(0, partial, a);
  }
  // bind the tables (len elements, len >= 4) with r in place and the next round's sums (its eq tables: t)
  uint32_t bind_sums(size_t len, const H& r, const Tables& t) {
    ScBatchedArgs<FID> a = base;
    a.r = r.to_device();
    a.eqL = t.eqL, a.eqR = t.eqR, a.shift = t.shift, a.mask = t.mask, a.n = (uint32_t)(len / 4);
    return this->template launch_pass<ScBatchedBindSums<FID>>(0, partial, a);
  }
  void to_host(size_t half, const H* rp, std::vector<std::vector<H>>& hA, std::vector<std::vector<H>>& hB, std::vector<std::vector<H>>& hC) {
    std::vector<std::vector<H>>* out[3] = {&hA, &hB, &hC};
    Base::to_host(
        half, rp, 3 * k,
        [&](const F& r, uint32_t n, uint32_t bind) {
          ScBatchedArgs<FID> a = base;
          a.r = r, a.n = n, a.bind = bind;
          hipLaunchKernelGGL((k_scb_bind_only<FID>), dim3(Base::blocks(n)), dim3(256), 0, this->h.c.stream, a);
        },
        [&](uint32_t t) -> std::vector<H>& { return (*out[t % 3])[t / 3]; });
  }
};

// SumcheckProof::prove_batched_cubic (sumcheck.rs:509-577) as a prover of sc_prove_inplace
template <int FID> struct ScBatchedProver {
  using H = HostFp4<FID>;
  const void *claim, *taus;
  void *const *As, *const *Bs, *const *Cs;
  const void* alphas;
  size_t k;
  TranscriptFn cb;
  void* cb_ctx;
  uint8_t *out_polys, *out_r, *out_claims;
  typename ScAlg<FID>::Eq eq;
  H cl;
  std::vector<H> al;
  ScEqDev<FID> eqd;
  std::optional<ScBatchedDev<FID>> dev;
  std::vector<std::vector<H>> hA, hB, hC;
  typename ScEqDev<FID>::Tables tb;
  uint32_t seq = 0;  // of the pending sums

  void read_scalars(const ScAlg<FID>& alg, uint32_t l) {
    eq.init(alg, (const uint8_t*)taus, l);
    cl = alg.in(claim);
    al.resize(k);
    for (size_t i = 0; i < k; i++) al[i] = alg.in((const uint8_t*)alphas + 32 * i);
  }
  void reserve(ScDev<FID>& h, uint32_t l, bool device_rounds) {
    arena_reserve(h.c, kScPartialBytes + pad256((size_t)3 * k * kTailMax * 32) + 512);
    if (device_rounds) {
      aux_reserve(h.c, ScEqDev<FID>::heap_bytes(l));
      eqd.init(h, eq, h.c.aux);
    }
    dev.emplace(h, As, Bs, Cs, al);
    hA.resize(k), hB.resize(k), hC.resize(k);
  }
  void first_sums(size_t len) {
    tb = eqd.tables(1);
    seq = dev->sums(len, tb, false);
    eq.prepare();
  }
  void round_poly(size_t len, H* co) {
    ScDev<FID>& h = dev->h;
    const uint32_t* res = h.wait(0, seq);
    const uint32_t nf = ScBatchedDev<FID>::factors(tb);
    const H t0 = h.raw(res, nf), tinf = h.raw(res + 8, nf);
    H s0, lead, sm1;
    eq.derive(t0, tinf, cl, false, s0, lead, sm1, [&] {  // tau_j = 0: t(-1) = 2 t(inf) + 2 t(0) - t(1), t(1) from the high halves
      const H t1 = h.raw(h.wait(0, dev->sums(len, tb, true)), nf);
      return t0.dbl() + tinf.dbl() - t1;
    });
    ScAlg<FID>::from_evals_deg3(s0, cl, lead, sm1, co);
  }
  void bound(const H* co, const H& r) {
    cl = ScAlg<FID>::poly_eval(co, 4, r);
    eq.bound(r);
  }
  void bind_sums(size_t len, const H& r, uint32_t next) {
    tb = eqd.tables(next);
    seq = dev->bind_sums(len, r, tb);
    eq.prepare();
  }
  void to_host(size_t half, const H* rp) { dev->to_host(half, rp, hA, hB, hC); }
  void host_tail(const ScAlg<FID>& alg, uint32_t l, uint32_t j) { sc_tail_rounds_batched<FID>(alg, &eq, l, j, cl, hA, hB, hC, al, cb, cb_ctx, out_polys, out_r); }
  void outputs(const ScAlg<FID>& alg) {
    if (out_claims)
      for (size_t i = 0; i < k; i++) {
        alg.out(hA[i][0], out_claims + 96 * i), alg.out(hB[i][0], out_claims + 96 * i + 32), alg.out(hC[i][0], out_claims + 96 * i + 64);
      }
  }
};

void fv_sumcheck_prove_batched_cubic(Ctx& c, int field, const void* claim, const void* taus, size_t num_rounds, void* const* As, void* const* Bs,
                                     void* const* Cs, const void* alphas, size_t k, uint32_t flags, TranscriptFn cb, void* cb_ctx,
                                     uint8_t* out_polys, uint8_t* out_r, uint8_t* out_claims) {
  require(k >= 1 && k <= kScBatchedMaxK, NMX_E_ARG, "prove_batched_cubic: between 1 and 16 triples");
  with_field(field, [&](auto F) {
    ScBatchedProver<F()> p{claim, taus, As, Bs, Cs, alphas, k, cb, cb_ctx, out_polys, out_r, out_claims};
    sc_prove_inplace<F()>(c, flags, num_rounds, p);
  });
}
#endif

}  // namespace nmx
