// hyperkzg.hpp -- the batched multi-point quotients of HyperKZG's kzg_open_batch (src/provider/hyperkzg.rs:1007-1072 of the reference):
// with B[t] = sum_{i : len_i > t} q^i f_i[t] over k coefficient vectors of any lengths (B is :1059, never stored by default) and m <= 3
// points u_j,
//     out_j[t] = sum_{s >= t} B[s] u_j^(s - t),  t < n_out = max len_i
// so that out_j[0] = B(u_j) (poly_eval, :1011-1020) and out_j[1..] is the quotient of div_by_monomial(B, u_j) (:961-999).
// Included at the end of fieldvec.hip.  The lane bodies use no wave-level intrinsic and no LDS, so tests/host_emul runs them on the CPU
// (simt.hpp); the plan (lq_plan, lq_point_powers, lq_q_powers) is plain C++ and tests/cpp/hyperkzg_plan_test.cpp runs it under g++.
//
// The pass has the shape of Mercury's division (mercury.hpp): no block or wave waits for another one.
//     level 0   LqHeadsFn   lane c sums the K coefficients B[K c .. K c + K) from the f_i long enough to reach them (K = 4, option
//                           kzg_quot_chunk: 8) and runs m Horner chains over them from a zero carry: heads_j[c] = sum_e B[K c + e] u_j^e.
//                           It also stores the canonical B in workspace (option kzg_quot_scratch, 1 by default).
//     levels>0  LqUpHeadsFn / LqUpWalkFn: the suffix Horner of heads_j at u_j^K, 16-element chunks per lane, level after level until one
//                           chunk is left -- the recursion of the two-pass suffix Horner (fieldvec.hip), all m points in one launch per
//                           level (lane = (point, chunk)).  Its result: carries_j[c] = out_j[K c].
//     level 0   LqWalkFn    lane c reads its K coefficients of B back (kzg_quot_scratch = 0: sums them again), and for every point walks
//                           the chunk down from carries_j[c + 1] (0 above the top chunk), stores its K results of every out_j back to back.
// Algorithmic traffic on prove's shape (n, n/2, ..., 2: two reads per coefficient on average): 2n + n read, n + 3n written, plus 3n/K heads
// and carries each written and read once.  Summing again instead: 2n + 2n read, 3n written.
// Measured on one MI355X (scripts/bench_hyperkzg_prove.py, docs/measurements.md; BN254 Fr, prove's shape, three points, medians in ms):
//     n = 2^20   K = 4 + stored B 0.377   K = 4, summed twice 0.383   K = 8 + stored B 0.422   K = 8, summed twice 0.481   (lincomb + 3 x Horner: 0.402)
//     n = 2^19                  0.374                          0.389                   0.382                          0.445   (                      0.307)
//     n = 2^14                  0.246                          0.262                   0.260                          0.315   (                      0.192)
// so K = 4 with the stored copy stayed as the default (K = 8 holds 243 VGPRs, two waves per SIMD; K = 4 holds 124), and below
// kKzgFusedMinN = 2^20 nmx_hyperkzg_prove keeps the composed division, which has fewer launches (capi.hip).  The pass is bound by its
// eleven dependent launches (2^20), not by bytes.  (Those figures were taken with the upper levels written to load a whole chunk ahead of
// its chain; the compiler did not unroll that form and it measured no better than the plain loops kept here -- 0.317 / 0.217 ms at
// 2^20 / 2^14 in the session that ran them.)
//
// Forms.  q^i and the powers of u_j are in the internal form (e 2^261), so w * x and u * t are in x's form: canonical words and
// Montgomery words (NMX_SCALARS_MONT) take the same kernels.
//
// Bounds (p = the modulus; a product of operands below a p and b p with a b < 127 is normalised and below p (1 + a b / 127); an input
// word is any 256-bit value, 2^256 < 6 p for all four fields):
//   sum      w_i (canonical, < p) * x (< 6 p) < 1.05 p per term; a canonical accumulator plus six terms < 7.3 p < 16 p, limbs < 8 * 2^29
//            -> norm().canon() every six terms and at the end: B[t] is canonical BEFORE it enters a chain
//   chains   t < 2.02 p throughout: B (< p) + u (canonical) * t (< p (1 + 2.02 / 127) = 1.016 p) -> norm(); a carry is a stored value, canonical
//   stores   every stored value is t.canon4() of a t < 2.02 p < 4 p: the canonical representative.  The results therefore depend neither
//            on the launch geometry nor on an option, and equal nmx_field_lincomb_powers + nmx_poly_suffix_horner byte for byte.
#pragma once

#include "host_fp4.hpp"
#include "msm_partition.hpp"  // NMX_DEV: the device / emulation spelling
#include "spmv_row.hpp"       // ld / st

namespace nmx {

static constexpr uint32_t kLqMaxPts = 3;      // points per call (r, -r, r^2)
static constexpr uint32_t kLqUpChunk = 16;    // elements per lane above level 0: those levels are pure latency (kHornerChunk, fieldvec.hip)
static constexpr uint32_t kLqMaxLevels = 12;  // n_out < 2^31: 2^31 / 4 = 2^29, then seven divisions by 16
static constexpr uint32_t kLqInline = 32;     // vectors whose descriptors travel in the kernel arguments (prove: ell <= 30)

// ---- the host's plan: plain C++ ------------------------------------------------------------------------------------------------------
struct LqPlan {
  uint32_t chunk;            // K of level 0: 4 or 8
  uint32_t levels;           // >= 1; level l has n[l] elements in chunks of (l ? 16 : K); the last level is ONE chunk
  uint32_t n[kLqMaxLevels];  // n[0] = n_out, n[l + 1] = ceil(n[l] / chunk of level l)
};
static inline uint32_t lq_level_chunk(const LqPlan& p, uint32_t l) { return l ? kLqUpChunk : p.chunk; }
// opt = the option kzg_quot_chunk: 8 -> 8, anything else -> 4.  1 <= n_out < 2^31.
static inline LqPlan lq_plan(size_t n_out, uint32_t opt) {
  LqPlan p{};
  p.chunk = opt == 8 ? 8u : 4u;
  p.n[0] = (uint32_t)n_out;
  p.levels = 1;
  while (p.n[p.levels - 1] > lq_level_chunk(p, p.levels - 1)) {
    const uint32_t K = lq_level_chunk(p, p.levels - 1);
    p.n[p.levels] = (p.n[p.levels - 1] + K - 1) / K;
    p.levels++;
  }
  return p;
}
// out[l] = u^(elements of level 0 per element of level l) = u, u^K, u^(16 K), ...: internal form, canonical
template <int FID> static inline void lq_point_powers(const HostFp4<FID>& u, const LqPlan& pl, Fp<FID>* out) {
  HostFp4<FID> ul = u;
  for (uint32_t l = 0; l < pl.levels; l++) {
    out[l] = ul.to_device();
    for (uint32_t s = lq_level_chunk(pl, l); s > 1; s >>= 1) ul = ul * ul;
  }
}
// w[8 i ..] = q^i, internal form, canonical (powers::<E>(&q, k), spartan/mod.rs:130-137)
template <int FID> static inline void lq_q_powers(const HostFp4<FID>& q, size_t k, uint32_t* w) {
  HostFp4<FID> pw = HostFp4<FID>::one();
  for (size_t i = 0; i < k; i++) {
    pw.to_device().to_words(w + 8 * i);
    pw = pw * q;
  }
}

// ---- lane bodies -----------------------------------------------------------------------------------------------------------------
struct LqPoly {
  const uint32_t* f;  // len elements
  uint32_t len, pad;
  uint32_t w[8];      // q^i, internal form, canonical
};
template <int FID> struct LqArgs {
  LqPoly tab[kLqInline];  // the first k descriptors when k <= kLqInline
  const LqPoly* ext;      // all k descriptors in device memory when k > kLqInline, else nullptr
  uint32_t k, m, n, nc;   // vectors, points, n_out, chunks of level 0
  Fp<FID> u[kLqMaxPts];
  uint32_t* heads[kLqMaxPts];          // nc elements each (heads pass)
  const uint32_t* carries[kLqMaxPts];  // carries[j][c] = out_j[K c], nc elements (walk; never read when nc == 1)
  uint32_t* out[kLqMaxPts];            // n elements each (walk)
  uint32_t* scratch;                   // n elements: B, written by the heads pass when not null
};

// b[e] = B[lo + e], e < cnt <= K: canonical
template <int FID, uint32_t K> NMX_DEV void lq_sum_chunk(const LqArgs<FID>& a, uint32_t lo, uint32_t cnt, Fp<FID> (&b)[K]) {
  using F = Fp<FID>;
#pragma unroll
  for (uint32_t e = 0; e < K; e++) b[e] = F::zero();
  uint32_t pending = 0;
  for (uint32_t i = 0; i < a.k; i++) {
    const LqPoly& P = a.ext ? a.ext[i] : a.tab[i];
    if (P.len <= lo) continue;  // this vector does not reach the chunk: not read
    const uint32_t have = P.len - lo < cnt ? P.len - lo : cnt;
    const F w = F::from_words(P.w);
    const uint32_t* __restrict__ f = P.f + 8 * (size_t)lo;
    if (have == K) {  // all the loads of the chunk are issued before the first product
      F x[K];
#pragma unroll
      for (uint32_t e = 0; e < K; e++) x[e] = ld<FID>(f, e);
#pragma unroll
      for (uint32_t e = 0; e < K; e++) b[e] = b[e] + w * x[e];  // + (< 1.05 p)
    } else {
#pragma unroll
      for (uint32_t e = 0; e < K; e++)
        if (e < have) b[e] = b[e] + w * ld<FID>(f, e);
    }
    if (++pending == 6) {
#pragma unroll
      for (uint32_t e = 0; e < K; e++) {
        b[e].check_below(7.3, "lq_sum_chunk: accumulator");
        b[e] = b[e].norm().canon();
      }
      pending = 0;
    }
  }
#pragma unroll
  for (uint32_t e = 0; e < K; e++) {
    b[e].check_below(7.3, "lq_sum_chunk: accumulator");
    b[e] = b[e].norm().canon();
  }
}
// the chunk of the walk when the heads pass stored B: canonical words
template <int FID, uint32_t K> NMX_DEV void lq_load_chunk(const uint32_t* B, uint32_t lo, uint32_t cnt, Fp<FID> (&b)[K]) {
#pragma unroll
  for (uint32_t e = 0; e < K; e++) b[e] = e < cnt ? ld<FID>(B, (size_t)lo + e) : Fp<FID>::zero();
}

template <int FID, uint32_t K> struct LqHeadsFn {
  LqArgs<FID> a;
  NMX_HD void operator()(uint32_t c) const {
    using F = Fp<FID>;
    const uint32_t lo = c * K, cnt = a.n - lo < K ? a.n - lo : K;
    F b[K];
    lq_sum_chunk<FID, K>(a, lo, cnt, b);
    if (a.scratch) {
#pragma unroll
      for (uint32_t e = 0; e < K; e++)
        if (e < cnt) b[e].to_words(a.scratch + 8 * ((size_t)lo + e));
    }
#pragma unroll  // (constant indices keep u[], heads[] in registers / scalars)
    for (uint32_t j = 0; j < kLqMaxPts; j++) {
      if (j >= a.m) break;
      F t = F::zero();
#pragma unroll
      for (uint32_t e = K; e-- > 0;)
        if (e < cnt) {
          t = (b[e] + a.u[j] * t).norm();
          t.check_below(2.02, "LqHeadsFn: t");
        }
      t.canon4().to_words(a.heads[j] + 8 * (size_t)c);
    }
  }
};
template <int FID, uint32_t K, bool SCRATCH> struct LqWalkFn {
  LqArgs<FID> a;
  NMX_HD void operator()(uint32_t c) const {
    using F = Fp<FID>;
    const uint32_t lo = c * K, cnt = a.n - lo < K ? a.n - lo : K;
    F b[K];
    if constexpr (SCRATCH) lq_load_chunk<FID, K>(a.scratch, lo, cnt, b);
    else lq_sum_chunk<FID, K>(a, lo, cnt, b);
#pragma unroll
    for (uint32_t j = 0; j < kLqMaxPts; j++) {
      if (j >= a.m) break;
      F t = c + 1 < a.nc ? ld<FID>(a.carries[j], (size_t)c + 1) : F::zero();  // canonical
      uint32_t* __restrict__ o = a.out[j] + 8 * (size_t)lo;
      if (cnt == K) {
        uint32_t w[K][8];
#pragma unroll
        for (uint32_t e = K; e-- > 0;) {
          t = (b[e] + a.u[j] * t).norm();
          t.check_below(2.02, "LqWalkFn: t");
          t.canon4().to_words(w[e]);
        }
#pragma unroll
        for (uint32_t e = 0; e < K; e++)
#pragma unroll
          for (int q = 0; q < 8; q++) o[8 * e + q] = w[e][q];
      } else {
#pragma unroll
        for (uint32_t e = K; e-- > 0;)
          if (e < cnt) {
            t = (b[e] + a.u[j] * t).norm();
            t.check_below(2.02, "LqWalkFn: t");
            t.canon4().to_words(o + 8 * e);
          }
      }
    }
  }
};

// levels above 0: m independent suffix Horners over stored (canonical) values, lane i = (point i / nc, chunk i % nc)
template <int FID> struct LqUpArgs {
  const uint32_t* src[kLqMaxPts];      // n elements each
  uint32_t* heads[kLqMaxPts];          // nc
  const uint32_t* carries[kLqMaxPts];  // nc (never read when nc == 1)
  uint32_t* out[kLqMaxPts];            // n
  Fp<FID> u[kLqMaxPts];                // u_j^(level-0 elements per element of this level)
  uint32_t m, n, nc;
};
template <int FID> struct LqUpHeadsFn {
  LqUpArgs<FID> a;
  NMX_HD void lane(const uint32_t* __restrict__ src, uint32_t* heads, const Fp<FID>& u, uint32_t c) const {
    using F = Fp<FID>;
    const uint32_t lo = c * kLqUpChunk, hi = a.n - lo < kLqUpChunk ? a.n : lo + kLqUpChunk;
    F t = F::zero();
    for (uint32_t e = hi; e-- > lo;) {
      t = (ld<FID>(src, e) + u * t).norm();
      t.check_below(2.02, "LqUpHeadsFn: t");
    }
    t.canon4().to_words(heads + 8 * (size_t)c);
  }
  NMX_HD void operator()(uint32_t i) const {
    const uint32_t j = i / a.nc, c = i % a.nc;
#pragma unroll  // (constant indices: the arguments stay where they are, no private copy)
    for (uint32_t jj = 0; jj < kLqMaxPts; jj++)
      if (jj == j) lane(a.src[jj], a.heads[jj], a.u[jj], c);
  }
};
template <int FID> struct LqUpWalkFn {
  LqUpArgs<FID> a;
  NMX_HD void lane(const uint32_t* __restrict__ src, const uint32_t* carries, uint32_t* out, const Fp<FID>& u, uint32_t c) const {
    using F = Fp<FID>;
    const uint32_t lo = c * kLqUpChunk, hi = a.n - lo < kLqUpChunk ? a.n : lo + kLqUpChunk;
    F t = c + 1 < a.nc ? ld<FID>(carries, (size_t)c + 1) : F::zero();
    for (uint32_t e = hi; e-- > lo;) {
      t = (ld<FID>(src, e) + u * t).norm();
      t.check_below(2.02, "LqUpWalkFn: t");
      t.canon4().to_words(out + 8 * (size_t)e);
    }
  }
  NMX_HD void operator()(uint32_t i) const {
    const uint32_t j = i / a.nc, c = i % a.nc;
#pragma unroll
    for (uint32_t jj = 0; jj < kLqMaxPts; jj++)
      if (jj == j) lane(a.src[jj], a.carries[jj], a.out[jj], a.u[jj], c);
  }
};

// ---- the launches of one pass: plain C++, shared by the host half below and by tests/host_emul ----------------------------------------
// a: tab / ext, k, m, out[], scratch filled in; up[j][l] = lq_point_powers of point j; take(elems) -> workspace of that many elements;
// launch(functor, lanes) runs functor(i) for i < lanes (256 lanes per block)
template <int FID, class Take, class Launch>
static inline void lq_run(const LqPlan& pl, LqArgs<FID> a, const Fp<FID> (*up)[kLqMaxLevels], Take&& take, Launch&& launch) {
  const uint32_t m = a.m;
  // per level l >= 1 and point: its input (the heads of the level below) and its result (the carries of the level below)
  uint32_t *lv_src[kLqMaxLevels + 1][kLqMaxPts] = {}, *lv_out[kLqMaxLevels + 1][kLqMaxPts] = {};
  for (uint32_t l = 1; l < pl.levels; l++)
    for (uint32_t j = 0; j < m; j++) lv_src[l][j] = take(pl.n[l]), lv_out[l][j] = take(pl.n[l]);
  a.n = pl.n[0], a.nc = pl.levels > 1 ? pl.n[1] : 1u;
  for (uint32_t j = 0; j < m; j++) a.u[j] = up[j][0], a.heads[j] = lv_src[1][j], a.carries[j] = lv_out[1][j];
  // down: the heads of every level that has more than one chunk
  if (pl.levels > 1) {
    if (pl.chunk == 4) launch(LqHeadsFn<FID, 4>{a}, a.nc);
    else launch(LqHeadsFn<FID, 8>{a}, a.nc);
  }
  LqUpArgs<FID> ua[kLqMaxLevels];
  for (uint32_t l = 1; l < pl.levels; l++) {
    LqUpArgs<FID>& x = ua[l];
    x = LqUpArgs<FID>{};
    x.m = m, x.n = pl.n[l], x.nc = l + 1 < pl.levels ? pl.n[l + 1] : 1u;
    for (uint32_t j = 0; j < m; j++) {
      x.src[j] = lv_src[l][j], x.out[j] = lv_out[l][j];
      x.heads[j] = lv_src[l + 1][j], x.carries[j] = lv_out[l + 1][j];  // (null at the top level: one chunk, no carry)
      x.u[j] = up[j][l];
    }
    if (l + 1 < pl.levels) launch(LqUpHeadsFn<FID>{x}, m * x.nc);
  }
  // up: every level walked from the carries of the level above
  for (uint32_t l = pl.levels; l-- > 1;) launch(LqUpWalkFn<FID>{ua[l]}, m * ua[l].nc);
  const bool from_scratch = a.scratch && pl.levels > 1;  // (one chunk: no heads pass has stored B)
  if (pl.chunk == 4) {
    if (from_scratch) launch(LqWalkFn<FID, 4, true>{a}, a.nc);
    else launch(LqWalkFn<FID, 4, false>{a}, a.nc);
  } else {
    if (from_scratch) launch(LqWalkFn<FID, 8, true>{a}, a.nc);
    else launch(LqWalkFn<FID, 8, false>{a}, a.nc);
  }
}

#if defined(__HIPCC__) || defined(__HIP__)
// ---- the host half ---------------------------------------------------------------------------------------------------------------
// `chain`: the call is a step of a longer one on the same stream (nmx_hyperkzg_prove): nothing is waited for and nothing is marked.
template <int FID>
static void lincomb_quotients_t(Ctx& c, const void* const* polys, const size_t* lens, size_t k, const void* q, const void* points, size_t m,
                                uint32_t flags, void* const* outs, bool chain) {
  using F = Fp<FID>;
  using H = HostFp4<FID>;
  const bool mont = flags & NMX_SCALARS_MONT, dev = flags & NMX_SCALARS_DEVICE;
  bool async = dev && (flags & NMX_ASYNC);
  // NMX_E_SCALAR_RANGE before anything is enqueued
  (void)challenge<FID>(q, mont);
  for (size_t j = 0; j < m; j++) (void)challenge<FID>((const uint8_t*)points + 32 * j, mont);
  size_t n_out = 0, in_bytes = 0;
  for (size_t i = 0; i < k; i++) {
    n_out = lens[i] > n_out ? lens[i] : n_out;
    in_bytes += pad256(lens[i] * 32);
  }
  if (n_out == 0) return;
  const LqPlan pl = lq_plan(n_out, G.kzg_quot_chunk.load(std::memory_order_relaxed));
  const bool scratch = G.kzg_quot_scratch.load(std::memory_order_relaxed) != 0;
  size_t need = 256 + (k > kLqInline ? pad256(k * sizeof(LqPoly)) : 0) + (scratch ? pad256(n_out * 32) : 0);
  for (uint32_t l = 1; l < pl.levels; l++) need += 2 * m * pad256((size_t)pl.n[l] * 32);
  if (!dev) need += in_bytes + m * pad256(n_out * 32);
  arena_reserve(c, need);
  MercuryArena ws{c};
  std::vector<LqPoly> desc(k);
  {
    const uint8_t* qb = (const uint8_t*)q;
    std::vector<uint32_t> w(8 * k);
    lq_q_powers<FID>(mont ? H::from_mont256(qb) : H::from_canonical(qb), k, w.data());
    for (size_t i = 0; i < k; i++) {
      desc[i].f = lens[i] ? ws.in(polys[i], lens[i], dev) : nullptr;
      desc[i].len = (uint32_t)lens[i], desc[i].pad = 0;
      memcpy(desc[i].w, w.data() + 8 * i, 32);
    }
  }
  F up[kLqMaxPts][kLqMaxLevels];
  for (size_t j = 0; j < m; j++) {
    const uint8_t* pj = (const uint8_t*)points + 32 * j;
    lq_point_powers<FID>(mont ? H::from_mont256(pj) : H::from_canonical(pj), pl, up[j]);
  }
  LqArgs<FID> a{};
  a.ext = nullptr;
  if (k > kLqInline) {  // the table is read from this stack frame by the copy: the call then always waits
    LqPoly* d = (LqPoly*)ws.take(k * sizeof(LqPoly));
    HIPCHK(hipMemcpyAsync(d, desc.data(), k * sizeof(LqPoly), hipMemcpyHostToDevice, c.stream));
    a.ext = d;
    async = false;
  } else {
    for (size_t i = 0; i < k; i++) a.tab[i] = desc[i];
  }
  a.k = (uint32_t)k, a.m = (uint32_t)m;
  a.scratch = scratch ? (uint32_t*)ws.take(n_out * 32) : nullptr;
  for (size_t j = 0; j < m; j++) a.out[j] = dev ? (uint32_t*)outs[j] : (uint32_t*)ws.take(n_out * 32);
  const bool prof = G.profiling && !chain;
  DeviceBackend be(c, false, prof);
  try {
    be.mark("kernel");
    lq_run<FID>(pl, a, up, [&](size_t elems) { return (uint32_t*)ws.take(elems * 32); }, [&](const auto& fn, uint32_t lanes) { be.launch(fn, lanes); });
    be.mark("end");
    if (!dev)
      for (size_t j = 0; j < m; j++) HIPCHK(hipMemcpyAsync(outs[j], a.out[j], n_out * 32, hipMemcpyDeviceToHost, c.stream));
  } catch (...) {
    (void)hipStreamSynchronize(c.stream);
    throw;
  }
  if (chain) {
    if (a.ext) stream_wait(c.stream);  // (desc is read by the copy above)
    return;
  }
  mercury_finish(c, be, prof, async);
}

void fv_lincomb_quotients(Ctx& c, int field, const void* const* polys, const size_t* lens, size_t k, const void* q, const void* points,
                          size_t m, uint32_t flags, void* const* outs, bool chain) {
  with_field(field, [&](auto F) { lincomb_quotients_t<F()>(c, polys, lens, k, q, points, m, flags, outs, chain); });
}
#endif

}  // namespace nmx
