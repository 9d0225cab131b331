// sumcheck_batched.hpp -- SumcheckProof::prove_batched_cubic as ONE C call (nmx_sumcheck_prove_batched_cubic).  Included by
// sumcheck.hip behind sumcheck_prove.hpp, whose mailbox, eq heaps and host algebra it uses.
//
//   prove_batched_cubic                                               src/spartan/sumcheck.rs:509-577
//   evaluation_points_batched_cubic / fallback_eval_inf_batched_cubic src/spartan/sumcheck.rs:749-894
//
//   sum_x eq(tau, x) * sum_i alpha_i (A_i(x) B_i(x) - C_i(x)) = claim      for K <= 16 triples under one sum-check
//
// Two passes, both one index per lane with a loop over the K triples inside the index (the eq factor is applied once per index,
// not once per triple, as the reference does):
//   sums         id in [0, len/2): (t(0), t(inf)) of a round over the tables as they are.  Round 1 -- and, pointed at the high halves
//                with with_inf = 0, t(1) of a round whose tau is zero: t(-1) = 2 t(inf) + 2 t(0) - t(1) (the fallback's third sum).
//   bind + sums  id in [0, len/4): every table bound with the round's challenge in place (four loads, two stores per table) and the
//                NEXT round's two sums over the bound values in the same pass.
//   bind only    id in [0, len/2): the last bind of the device part (two loads, one store per table; no sums).  The bound tables also
//                go to a contiguous staging area which one stream-ordered copy brings to the host (len == 2 included: one lane).
// Each pass leaves one pair of partial sums per block; k_sum_partials_mail (one block) adds them into the mailbox slot.  Every
// kernel is launched after its challenge exists and ends on its own: nothing here waits on the device for the host (no pre-launched
// pass, no resident kernel, no four-lane form -- those are the three existing provers').
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

#include "msm_partition.hpp"  // NMX_DEV, NMX_TID: the device / emulation spellings
#include "spmv_row.hpp"       // ld

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
template <int FID> NMX_DEV Fp<FID> sc_batched_factor(const ScBatchedArgs<FID>& a, uint32_t id) {
  Fp<FID> fac = ld<FID>(a.eqR, a.eqL ? (id & a.mask) : id);
  if (a.eqL) fac = ld<FID>(a.eqL, id >> a.shift) * fac;  // < 1.01 p
  return fac;
}
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

// ---- the sums pass: indices first, first + stride, ... of [0, a.n); on return s0 / s1 are canonical -------------------------------
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
    sc_batched_fold<FID>(t, sc_batched_factor<FID>(a, id), wi, s0, s1, pending);
  }
  s0 = s0.norm().canon();
  s1 = s1.norm().canon();
}

// bind_poly_var_top (multilinear.rs:65-84) on the two elements of X that next-round index id reads: lo + r (hi - lo), in place
template <int FID> NMX_DEV void sc_batched_bind2(uint32_t* X, const Fp<FID>& r, uint32_t id, uint32_t hq, Fp<FID>& y0, Fp<FID>& y1) {
  using F = Fp<FID>;
  const F x00 = ld<FID>(X, id), x01 = ld<FID>(X, (size_t)id + hq);
  const F x10 = ld<FID>(X, (size_t)id + 2 * (size_t)hq), x11 = ld<FID>(X, (size_t)id + 3 * (size_t)hq);
  y0 = (x00 + r * F::sub2(x10, x00).norm()).norm().canon();
  y1 = (x01 + r * F::sub2(x11, x01).norm()).norm().canon();
  y0.to_words(X + 8 * (size_t)id);
  y1.to_words(X + 8 * ((size_t)id + hq));
}
// ---- the bind + sums pass over [0, a.n = len / 4).  A lane reads exactly the low-half elements it overwrites: binding in place is safe
template <int FID> NMX_DEV void sc_batched_bind_lane(const ScBatchedArgs<FID>& a, uint32_t first, uint32_t stride, Fp<FID>& s0, Fp<FID>& s1) {
  using F = Fp<FID>;
  uint32_t pending = 0;
  for (uint64_t i64 = first; i64 < a.n; i64 += stride) {
    const uint32_t id = (uint32_t)i64;
    ScBatchedAcc<FID> t;
    for (uint32_t i = 0; i < a.k; i++) {
      F a0, a1, b0, b1, c0, c1;
      sc_batched_bind2<FID>(a.A[i], a.r, id, a.n, a0, a1);
      sc_batched_bind2<FID>(a.B[i], a.r, id, a.n, b0, b1);
      sc_batched_bind2<FID>(a.C[i], a.r, id, a.n, c0, c1);
      t.add(a.alpha[i], a0, a1, b0, b1, c0, a.nk, true);
    }
    sc_batched_fold<FID>(t, sc_batched_factor<FID>(a, id), true, s0, s1, pending);
  }
  s0 = s0.norm().canon();
  s1 = s1.norm().canon();
}
// ---- the last device bind over [0, a.n = len / 2): no sums; the bound (bind = 0: the unchanged) tables also land in the staging area
template <int FID> NMX_DEV void sc_batched_bind_only_one(const ScBatchedArgs<FID>& a, uint32_t* X, uint32_t t, uint32_t id) {
  using F = Fp<FID>;
  F y = ld<FID>(X, id);
  if (a.bind) {
    const F x1 = ld<FID>(X, (size_t)id + a.n);
    y = (y + a.r * F::sub2(x1, y).norm()).norm().canon();
    y.to_words(X + 8 * (size_t)id);
  }
  y.to_words(a.stage + 8 * ((size_t)t * a.n + id));
}
template <int FID> NMX_DEV void sc_batched_bind_only_lane(const ScBatchedArgs<FID>& a, uint32_t first, uint32_t stride) {
  for (uint64_t i64 = first; i64 < a.n; i64 += stride) {
    const uint32_t id = (uint32_t)i64;
    for (uint32_t i = 0; i < a.k; i++) {  // (one array per statement: a table chosen by a run-time index into {A, B, C} costs a copy of the arguments in scratch)
      sc_batched_bind_only_one<FID>(a, a.A[i], 3 * i, id);
      sc_batched_bind_only_one<FID>(a, a.B[i], 3 * i + 1, id);
      sc_batched_bind_only_one<FID>(a, a.C[i], 3 * i + 2, id);
    }
  }
}

#if defined(__HIPCC__) || defined(__HIP__)
// Launch bounds 256: DESIGN.md ("batched cubic sum-check") has the compiler's register and LDS figures they were chosen from.
template <int FID> __global__ __launch_bounds__(256) void k_scb_sums(ScBatchedArgs<FID> a, uint32_t* partial) {
  using F = Fp<FID>;
  __shared__ uint32_t lds[72];
  F s0 = F::zero(), s1 = F::zero();
  sc_batched_sums_lane<FID>(a, blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, s0, s1);
  block_sum_pair<FID, true>(s0, s1, lds);
  if (threadIdx.x == 0) {
    s0.to_words(partial + 16 * (size_t)blockIdx.x);
    s1.to_words(partial + 16 * (size_t)blockIdx.x + 8);
  }
}
template <int FID> __global__ __launch_bounds__(256) void k_scb_bind_sums(ScBatchedArgs<FID> a, uint32_t* partial) {
  using F = Fp<FID>;
  __shared__ uint32_t lds[72];
  F s0 = F::zero(), s1 = F::zero();
  sc_batched_bind_lane<FID>(a, blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, s0, s1);
  block_sum_pair<FID, true>(s0, s1, lds);
  if (threadIdx.x == 0) {
    s0.to_words(partial + 16 * (size_t)blockIdx.x);
    s1.to_words(partial + 16 * (size_t)blockIdx.x + 8);
  }
}
template <int FID> __global__ __launch_bounds__(256) void k_scb_bind_only(ScBatchedArgs<FID> a) {
  sc_batched_bind_only_lane<FID>(a, blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u);
}

// the device side of one proof: the launches over the 3 k in-place tables, the context's stream, mailbox slot 0
template <int FID> struct ScBatchedDev {
  using F = Fp<FID>;
  using H = HostFp4<FID>;
  using Tables = typename ScEqDev<FID>::Tables;
  ScDev<FID>& h;
  ScBatchedArgs<FID> base{};
  uint32_t k;
  uint32_t* partial;  // kScPartialBytes of the arena
  uint32_t* stage;    // behind it: 3 k x tail_len elements
  ScBatchedDev(ScDev<FID>& h_, void* const* As, void* const* Bs, void* const* Cs, const std::vector<H>& alphas)
      : h(h_), k((uint32_t)alphas.size()), partial((uint32_t*)h_.c.arena), stage((uint32_t*)(h_.c.arena + kScPartialBytes)) {
    for (uint32_t i = 0; i < kScBatchedMaxK; i++) {
      base.A[i] = i < k ? (uint32_t*)As[i] : nullptr, base.B[i] = i < k ? (uint32_t*)Bs[i] : nullptr, base.C[i] = i < k ? (uint32_t*)Cs[i] : nullptr;
      base.alpha[i] = i < k ? alphas[i].to_device() : F::zero();
    }
    F fm = F::zero();  // the form factor as a plain integer, as ScPass<FID, 3>
    if (h.mont) fm = pow2_plain<FID>(256);
    else fm.l[0] = 1;
    base.nk = F::sub2(F::zero(), fm.canon()).norm().canon();
    base.r = F::zero(), base.eqL = base.eqR = nullptr, base.stage = nullptr;
    base.shift = 0, base.mask = 0xffffffffu, base.k = k, base.n = 0, base.with_inf = 1, base.bind = 0;
  }
  static uint32_t factors(const Tables& t) { return 3u + (t.eqL ? 1u : 0u); }
  static uint32_t blocks(uint32_t n) { return sc_blocks_bind(n); }  // one index per lane, at most 4096 blocks (the partials' scratch)
  void finish(uint32_t nblocks, uint32_t seq) {
    hipLaunchKernelGGL((k_sum_partials_mail<FID, 2, 2>), dim3(1), dim3(256), 0, h.c.stream, partial, nblocks, h.slot_dev(0), seq);
    HIPCHK(hipGetLastError());
    h.launched(2);
  }
  // (t(0), t(inf)) over tables of len elements; high = true: t(0)'s sum alone over the HIGH halves, which is t(1)
  uint32_t sums(size_t len, const Tables& t, bool high) {
    ScBatchedArgs<FID> a = base;
    const size_t half = len / 2;
    if (high)
      for (uint32_t i = 0; i < k; i++) a.A[i] += 8 * half, a.B[i] += 8 * half, a.C[i] += 8 * half;
    a.eqL = t.eqL, a.eqR = t.eqR, a.shift = t.shift, a.mask = t.mask, a.n = (uint32_t)half, a.with_inf = high ? 0u : 1u;
    const uint32_t nb = blocks(a.n), seq = h.next_seq();
    hipLaunchKernelGGL((k_scb_sums<FID>), dim3(nb), dim3(256), 0, h.c.stream, a, partial);
    HIPCHK(hipGetLastError());
    finish(nb, seq);
    return seq;
  }
  // bind the tables (len elements, len >= 4) with r in place and the next round's sums (its eq tables: t)
  uint32_t bind_sums(size_t len, const H& r, const Tables& t) {
    ScBatchedArgs<FID> a = base;
    a.r = r.to_device();
    a.eqL = t.eqL, a.eqR = t.eqR, a.shift = t.shift, a.mask = t.mask, a.n = (uint32_t)(len / 4);
    const uint32_t nb = blocks(a.n), seq = h.next_seq();
    hipLaunchKernelGGL((k_scb_bind_sums<FID>), dim3(nb), dim3(256), 0, h.c.stream, a, partial);
    HIPCHK(hipGetLastError());
    finish(nb, seq);
    return seq;
  }
  // the hand-over: bind with r (rp == nullptr: no bind) and bring the 3 k tables of `half` elements to the host
  void to_host(size_t half, const H* rp, std::vector<std::vector<H>>& hA, std::vector<std::vector<H>>& hB, std::vector<std::vector<H>>& hC) {
    require(half >= 1 && half <= kTailMax, NMX_E_HIP, "sum-check: tail hand-over out of range");
    ScBatchedArgs<FID> a = base;
    a.r = rp ? rp->to_device() : F::zero();
    a.n = (uint32_t)half, a.bind = rp ? 1u : 0u, a.stage = stage;
    hipLaunchKernelGGL((k_scb_bind_only<FID>), dim3(blocks(a.n)), dim3(256), 0, h.c.stream, a);
    HIPCHK(hipGetLastError());
    h.launched();
    std::vector<uint32_t> land((size_t)3 * k * half * 8);
    HIPCHK(hipMemcpyAsync(land.data(), stage, land.size() * 4, hipMemcpyDeviceToHost, h.c.stream));
    stream_wait(h.c.stream);
    std::vector<std::vector<H>>* out[3] = {&hA, &hB, &hC};
    for (uint32_t i = 0; i < k; i++)
      for (uint32_t w = 0; w < 3; w++) {
        std::vector<H>& v = (*out[w])[i];
        v.resize(half);
        const uint32_t* src = land.data() + 8 * ((size_t)(3 * i + w) * half);
        for (size_t x = 0; x < half; x++) v[x] = h.stored(src + 8 * x);
      }
  }
};

// SumcheckProof::prove_batched_cubic (sumcheck.rs:509-577).  Of the sc_* options only sc_host_tail and sc_poll_us apply.
template <int FID>
static void sc_prove_batched_t(Ctx& c, const void* claim, const void* taus, size_t num_rounds, void* const* As, void* const* Bs, void* const* Cs,
                               const void* alphas, size_t k, uint32_t flags, TranscriptFn cb, void* cb_ctx, uint8_t* out_polys, uint8_t* out_r,
                               uint8_t* out_claims) {
  using H = HostFp4<FID>;
  const auto T0 = std::chrono::steady_clock::now();
  const uint32_t l = (uint32_t)num_rounds;
  try {
    ScDev<FID> h(c, flags);
    try {
      // every scalar is read (and range-checked) before anything is launched (the C entry point has checked them already, before
      // it leased a device; this layer does not rely on that)
      typename ScAlg<FID>::Eq eq;
      eq.init(h.alg, (const uint8_t*)taus, l);
      H cl = h.alg.in(claim);
      std::vector<H> al(k);
      for (size_t i = 0; i < k; i++) al[i] = h.alg.in((const uint8_t*)alphas + 32 * i);
      size_t len = (size_t)1 << l;
      arena_reserve(c, kScPartialBytes + pad256((size_t)3 * k * kTailMax * 32) + 512);
      ScEqDev<FID> eqd;
      if (len > h.tail_len) {
        aux_reserve(c, ScEqDev<FID>::heap_bytes(l));
        eqd.init(h, eq, c.aux);
      }
      ScBatchedDev<FID> dev(h, As, Bs, Cs, al);
      std::vector<std::vector<H>> hA(k), hB(k), hC(k);
      uint32_t j = 1;
      if (len <= h.tail_len) {
        dev.to_host(len, nullptr, hA, hB, hC);  // the whole instance fits the tail
      } else {
        typename ScEqDev<FID>::Tables tb = eqd.tables(1);
        uint32_t seq = dev.sums(len, tb, false);
        eq.prepare();
        for (;; j++) {
          const uint32_t* res = h.wait(0, seq);
          const uint32_t nf = ScBatchedDev<FID>::factors(tb);
          const H t0 = h.raw(res, nf), tinf = h.raw(res + 8, nf);
          H s0, lead, sm1, co[4];
          eq.derive(t0, tinf, cl, false, s0, lead, sm1, [&] {  // tau_j = 0: t(-1) = 2 t(inf) + 2 t(0) - t(1), t(1) from the high halves
            const H t1 = h.raw(h.wait(0, dev.sums(len, tb, true)), nf);
            return t0.dbl() + tinf.dbl() - t1;
          });
          ScAlg<FID>::from_evals_deg3(s0, cl, lead, sm1, co);
          const H r = h.ask(cb, cb_ctx, co, 4, out_polys ? out_polys + 128 * (size_t)(j - 1) : nullptr, out_r ? out_r + 32 * (size_t)(j - 1) : nullptr);
          cl = ScAlg<FID>::poly_eval(co, 4, r);
          eq.bound(r);
          h.prof.rounds++;
          if (len / 2 <= h.tail_len) {  // the last device bind: no sums, the bound tables go to the host
            dev.to_host(len / 2, &r, hA, hB, hC);
            len /= 2;
            j++;
            break;
          }
          tb = eqd.tables(j + 1);
          seq = dev.bind_sums(len, r, tb);
          eq.prepare();
          len /= 2;
        }
      }
      if (j <= l) {
        h.prof.host_rounds += l - j + 1;
        sc_tail_rounds_batched<FID>(h.alg, &eq, l, j, cl, hA, hB, hC, al, cb, cb_ctx, out_polys, out_r);
      }
      if (out_claims)
        for (size_t i = 0; i < k; i++) {
          h.alg.out(hA[i][0], out_claims + 96 * i), h.alg.out(hB[i][0], out_claims + 96 * i + 32), h.alg.out(hC[i][0], out_claims + 96 * i + 64);
        }
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

void fv_sumcheck_prove_batched_cubic(Ctx& c, int field, const void* claim, const void* taus, size_t num_rounds, void* const* As, void* const* Bs,
                                     void* const* Cs, const void* alphas, size_t k, uint32_t flags, TranscriptFn cb, void* cb_ctx,
                                     uint8_t* out_polys, uint8_t* out_r, uint8_t* out_claims) {
  require(k >= 1 && k <= kScBatchedMaxK, NMX_E_ARG, "prove_batched_cubic: between 1 and 16 triples");
  with_field(field, [&](auto F) { sc_prove_batched_t<F()>(c, claim, taus, num_rounds, As, Bs, Cs, alphas, k, flags, cb, cb_ctx, out_polys, out_r, out_claims); });
}
#endif

}  // namespace nmx
