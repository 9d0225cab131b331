// sumcheck_inplace.hpp -- what the provers that bind their tables IN PLACE, one index per lane, have in common (the batched cubic prover,
// sumcheck_batched.hpp; ppsnark's inner one, sumcheck_ppsnark.hpp).  Included by sumcheck.hip behind sumcheck_prove.hpp, whose mailbox,
// eq heaps and host algebra the host half uses; the lane helpers also compile under g++ for the emulation (tests/host_emul/).
//
// The scheme: a sums pass for round 1 (id in [0, len/2), the tables as they are); per round one bind + sums pass (id in [0, len/4): every
// table bound with the round's challenge in place -- four loads, two stores per table, a lane reads exactly the elements it overwrites --
// and the NEXT round's sums over the bound values); one sum-less bind (id in [0, len/2)) that also copies the bound tables to a staging
// area, which one stream-ordered copy brings to the host tail.  Each sums-bearing pass leaves J partial sums per block;
// k_sum_partials_mail (one block) adds them into a mailbox slot.  Every kernel is launched after its challenge exists and ends on its own:
// nothing on the device waits for the host (no pre-launched pass, no resident kernel, no four-lane form -- those are the three older
// provers').  Of the sc_* options only sc_host_tail and sc_poll_us apply.
#pragma once

#include <optional>  // the provers hold their device side in one: it needs the driver's ScDev

#include "msm_partition.hpp"  // NMX_DEV, NMX_TID: the device / emulation spellings
#include "spmv_row.hpp"       // ld

namespace nmx {

// the eq factor of index id (ScEqDev::tables of the round the sums belong to): eqR alone, or eqL * eqR < 1.01 p
template <int FID> NMX_DEV Fp<FID> sc_eq_factor(const uint32_t* eqL, const uint32_t* eqR, uint32_t shift, uint32_t mask, uint32_t id) {
  Fp<FID> fac = ld<FID>(eqR, eqL ? (id & mask) : id);
  if (eqL) fac = ld<FID>(eqL, id >> shift) * fac;
  return fac;
}
// bind_poly_var_top (multilinear.rs:65-84) on the two elements of X that next-round index id reads: lo + r (hi - lo), in place.
// y0, y1 canonical.
template <int FID> NMX_DEV void sc_bind2(uint32_t* X, const Fp<FID>& r, uint32_t id, uint32_t hq, Fp<FID>& y0, Fp<FID>& y1) {
  using F = Fp<FID>;
  const F x00 = ld<FID>(X, id), x01 = ld<FID>(X, (size_t)id + hq);
  const F x10 = ld<FID>(X, (size_t)id + 2 * (size_t)hq), x11 = ld<FID>(X, (size_t)id + 3 * (size_t)hq);
  y0 = (x00 + r * F::sub2(x10, x00).norm()).norm().canon();
  y1 = (x01 + r * F::sub2(x11, x01).norm()).norm().canon();
  y0.to_words(X + 8 * (size_t)id);
  y1.to_words(X + 8 * ((size_t)id + hq));
}
// the last device bind of element id of X (n = len / 2 elements stay): two loads, one store, no sums; the bound (bind = 0: the unchanged)
// element also lands in the staging area, table t at element t * n
template <int FID> NMX_DEV void sc_bind_stage_one(uint32_t* X, const Fp<FID>& r, uint32_t n, uint32_t bind, uint32_t* stage, uint32_t t, uint32_t id) {
  using F = Fp<FID>;
  F y = ld<FID>(X, id);
  if (bind) {
    const F x1 = ld<FID>(X, (size_t)id + n);
    y = (y + r * F::sub2(x1, y).norm()).norm().canon();
    y.to_words(X + 8 * (size_t)id);
  }
  y.to_words(stage + 8 * ((size_t)t * n + id));
}

#if defined(__HIPCC__) || defined(__HIP__)
// The one kernel of the sums-bearing passes.  A pass type P names Args (POD, by value, with the index count n), Acc (the lane's J sums
// s[J], zero on construction), J and lane(args, first, stride, acc), which visits indices first, first + stride, ... of [0, n) and
// leaves acc.s canonical.  Block b writes its J sums at element J * b of `partial`.  Launch bounds 256: DESIGN.md has the compiler's
// register, LDS and occupancy figures per pass.
template <int FID, class P> __global__ __launch_bounds__(256) void k_sc_sums(typename P::Args a, uint32_t* partial) {
  __shared__ uint32_t lds[36 * P::J];
  typename P::Acc acc;
  P::lane(a, blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, acc);
  block_sum_waves<FID, P::J, true>(acc.s, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < P::J; j++) acc.s[j].to_words(partial + 8 * (P::J * (size_t)blockIdx.x + j));
  }
}

// what the device side of one proof shares: the context's stream, the form constants, the launches and the hand-over
template <int FID> struct ScInplaceDev {
  using F = Fp<FID>;
  using H = HostFp4<FID>;
  using Tables = typename ScEqDev<FID>::Tables;
  ScDev<FID>& h;
  F one, nk;        // Fm, the stored ONE; p - Fm
  uint32_t* stage;  // in the arena behind the partials: (tables) x tail_len elements
  ScInplaceDev(ScDev<FID>& h_, size_t partial_bytes)
      : h(h_), one(sc_form_factor<FID>(h_.mont).canon()), nk(F::sub2(F::zero(), one).norm().canon()), stage((uint32_t*)(h_.c.arena + partial_bytes)) {}
  static uint32_t blocks(uint32_t n) { return sc_blocks_bind(n); }  // one index per lane, at most 4096 blocks (the partials' areas)
  // one sums-bearing pass over a.n indices and the sum of its partials into mailbox slot `slot`; returns the sequence number to wait for
  template <class P> uint32_t launch_pass(uint32_t slot, uint32_t* partial, const typename P::Args& a) {
    const uint32_t nb = blocks(a.n), seq = h.next_seq();
    hipLaunchKernelGGL((k_sc_sums<FID, P>), dim3(nb), dim3(256), 0, h.c.stream, a, partial);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL((k_sum_partials_mail<FID, P::J, P::J>), dim3(1), dim3(256), 0, h.c.stream, partial, nb, h.slot_dev(slot), seq);
    HIPCHK(hipGetLastError());
    h.launched(2);
    return seq;
  }
  // the hand-over: bind with r (rp == nullptr: no bind) and bring the ntables tables of `half` elements to the host, table t into out(t).
  // launch_bind_only(r, n, bind) launches the prover's bind-only kernel on the context's stream.
  template <class Launch, class Out> void to_host(size_t half, const H* rp, uint32_t ntables, Launch&& launch_bind_only, Out&& out) {
    require(half >= 1 && half <= kTailMax, NMX_E_HIP, "sum-check: tail hand-over out of range");
    launch_bind_only(rp ? rp->to_device() : F::zero(), (uint32_t)half, rp ? 1u : 0u);
    HIPCHK(hipGetLastError());
    h.launched();
    std::vector<uint32_t> land((size_t)ntables * half * 8);
    HIPCHK(hipMemcpyAsync(land.data(), stage, land.size() * 4, hipMemcpyDeviceToHost, h.c.stream));
    stream_wait(h.c.stream);
    for (uint32_t t = 0; t < ntables; t++) {
      std::vector<H>& v = out(t);
      v.resize(half);
      const uint32_t* src = land.data() + 8 * ((size_t)t * half);
      for (size_t x = 0; x < half; x++) v[x] = h.stored(src + 8 * x);
    }
  }
};

// The round loop, once.  A prover P of this family provides
//   cb, cb_ctx, out_polys, out_r   the transcript callback and where the round polynomials (4 coefficients) and challenges go (or null)
//   read_scalars(alg, l)           every scalar read and range-checked (ScFail) -- before anything is launched
//   reserve(h, l, device_rounds)   the arena (partials + staging) and its device side; with device_rounds also aux and the eq heaps
//   first_sums(len)                round 1's sums over the tables as they are
//   round_poly(len, co)            waits for the pending sums and turns them into the round's coefficients, its t(1) fall-back passes included
//   bound(co, r)                   the claim(s) and eq scalars after challenge r
//   bind_sums(len, r, next)        bind with r in place and the sums of round `next` (its eq tables)
//   to_host(half, rp)              ScInplaceDev::to_host into its host tables
//   host_tail(alg, l, j)           rounds j .. l on the host tables
//   outputs(alg)                   the final evaluations
// The (partly bound) tables are the caller's again on return and on every failure.
template <int FID, class P> static void sc_prove_inplace(Ctx& c, uint32_t flags, size_t num_rounds, P& p) {
  using H = HostFp4<FID>;
  const auto T0 = std::chrono::steady_clock::now();
  const uint32_t l = (uint32_t)num_rounds;
  try {
    ScDev<FID> h(c, flags);
    try {
      // (the C entry point has checked the scalars already, before it leased a device; this layer does not rely on that)
      p.read_scalars(h.alg, l);
      size_t len = (size_t)1 << l;
      p.reserve(h, l, len > h.tail_len);
      uint32_t j = 1;
      if (len <= h.tail_len) {
        p.to_host(len, nullptr);  // the whole instance fits the tail
      } else {
        p.first_sums(len);
        for (;; j++) {
          H co[4];
          p.round_poly(len, co);
          const H r = h.ask(p.cb, p.cb_ctx, co, 4, p.out_polys ? p.out_polys + 128 * (size_t)(j - 1) : nullptr, p.out_r ? p.out_r + 32 * (size_t)(j - 1) : nullptr);
          p.bound(co, r);
          h.prof.rounds++;
          if (len / 2 <= h.tail_len) {  // the last device bind: no sums, the bound tables go to the host
            p.to_host(len / 2, &r);
            len /= 2;
            j++;
            break;
          }
          p.bind_sums(len, r, j + 1);
          len /= 2;
        }
      }
      if (j <= l) {
        h.prof.host_rounds += l - j + 1;
        p.host_tail(h.alg, l, j);
      }
      p.outputs(h.alg);
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
#endif

}  // namespace nmx
