// mercury_s.hpp -- make_s_polynomial of Mercury's prover (src/provider/mercury.rs:391-475) without an FFT.  The reference multiplies
// by X^(b-1), transforms at size 2b and keeps the upper b coefficients; nothing wraps mod X^(2b) - 1, so what it keeps is the
// cross-correlation
//     s[k] = sum_{i=0}^{b-2-k} ( a1[i+k+1] b1[i] + a1[i] b1[i+k+1] ) + gamma sum_{i=0}^{b-2-k} ( a2[i+k+1] b2[i] + a2[i] b2[i+k+1] ),  k < b - 1
// which is exact in any field (Grumpkin's scalar field has 2-adicity 1: no root of unity of order 2b exists there) and for any b.
// Included at the end of fieldvec.hip behind mercury.hpp.  The kernels use LDS and barriers and no wave-level intrinsic, so
// tests/host_emul runs them whole on the CPU (simt.hpp); the plan (mercury_s_plan) is plain C++.
//
// Decomposition.  The work is the triangle {(k, i): i + k + 1 < b} of 4 products per cell.  It is cut into square tiles of T outputs by T
// indices (T = the option mercury_s_tile: 16, 32 or 64; 0 = by size), and the index tiles of one row of output tiles into `chunks` runs of
// `cpt` tiles.  A block of 256 threads takes (output tile kt, chunk c): for each of its index tiles it stages two windows of the four
// operands in LDS -- the T elements at i and the 2T - 1 elements at i + k + 1, zero beyond b, so no cell needs a bounds test: a cell
// outside the triangle multiplies by a staged zero -- and thread (kk, q) sums the cells (k0 + kk, i0 + q + j G), G = 256 / T.  The G
// partial sums of an output meet in LDS; the block leaves ONE canonical partial per output, in `out` itself when chunks == 1, else in
// the workspace part[c][k], and a finish launch (MercurySFinishFn) adds an output's chunks.  No block waits for another block; every stored value is
// the canonical representative, so the bytes depend neither on the tile nor on the grid.  A block whose first index tile lies outside
// the triangle (i0 + k0 + 1 >= b) stores nothing and the finish does not read its slot (mercury_s_chunk_live, the same test).
// At b = 2^10 (a 2^20 proof) the default T = 32 gives 528 live blocks of 1024 cells each.
//
// Forms.  A prologue launch (MercurySPrepFn) brings a1 and gamma a2 into the internal form (e 2^261), canonical, ONCE; b1 and b2 are used as stored.
// A cell is then ONE Montgomery reduction over four products (Fp::dot<4>), and the result is in the form of b's words: canonical words
// and Montgomery words (NMX_SCALARS_MONT) take the same kernels.
//
// Bounds (p = the modulus; stored words may be any 256-bit value, 2^256 < 6 p for all four fields):
//   prep     a.to_internal() < 1.05 p (x gamma, canonical: < 1.01 p) -> canon()
//   cell     a (< p, limbs < 2^29) x b (< 6 p, limbs < 2^29): four products < 24 p^2 < 127 p^2, 45 x 2^58 < 2^64 per column -> < 1.19 p
//   lane     a canonical accumulator plus six cells < 8.2 p < 16 p, limbs < 7 x 2^29 < 2^32 -> norm().canon()
//   meet     a canonical accumulator plus six canonical lane sums < 7 p -> norm().canon()
//   finish   the same over an output's chunks
#pragma once

#include "msm_partition.hpp"  // NMX_DEV, NMX_KERNEL, NMX_LDS, NMX_SYNC: the device / emulation spelling
#include "spmv_row.hpp"       // ld / st

namespace nmx {

// ---- the host's plan: plain C++ ---------------------------------------------------------------------------------------------------
struct MercurySPlan {
  uint32_t tile;    // T: outputs per block = indices per staged window
  uint32_t ktiles;  // ceil((b - 1) / T) tiles of outputs
  uint32_t itiles;  // ceil((b - 1) / T) tiles of indices (i runs over 0 .. b - 2)
  uint32_t chunks;  // runs of index tiles per output tile: partial sums per output
  uint32_t cpt;     // index tiles per run
};
static constexpr uint32_t kMercurySBlocks = 1024;     // blocks the split aims for: 4 per CU
static constexpr uint32_t kMercurySMaxChunks = 32;    // partials per output the finish adds
// opt = the option mercury_s_tile: 0 = by size, else 16, 32 or 64.  b >= 2.
static inline MercurySPlan mercury_s_plan(size_t b, uint32_t opt) {
  MercurySPlan pl;
  pl.tile = opt ? opt : (b >= 8192 ? 64u : b >= 512 ? 32u : 16u);
  pl.ktiles = pl.itiles = (uint32_t)((b - 1 + pl.tile - 1) / pl.tile);
  uint32_t want = (kMercurySBlocks + pl.ktiles - 1) / pl.ktiles;
  want = want > kMercurySMaxChunks ? kMercurySMaxChunks : want;
  want = want > pl.itiles ? pl.itiles : want;
  pl.cpt = (pl.itiles + want - 1) / want;
  pl.chunks = (pl.itiles + pl.cpt - 1) / pl.cpt;
  return pl;
}

template <int FID> struct MercurySArgs {
  const uint32_t* a1;  // b elements, internal form, canonical (MercurySPrepFn)
  const uint32_t* a2;  // b elements: gamma a2, internal form, canonical
  const uint32_t* b1;  // b elements as stored
  const uint32_t* b2;
  uint32_t* part;      // chunks x (b - 1) elements of workspace (chunks > 1), else unused
  uint32_t* out;       // b - 1 elements
  uint32_t b, tile, chunks, cpt;
};
// does block (output tile at k0, chunk c) own a cell?  The one test of the kernel and of the finish.
NMX_HD bool mercury_s_chunk_live(uint32_t b, uint32_t tile, uint32_t cpt, uint32_t k0, uint32_t c) {
  return (uint64_t)c * cpt * tile + k0 + 1u < b;
}

// a1 -> internal; a2 -> gamma a2, internal; canonical words, 2 b lanes
template <int FID> struct MercurySPrepFn {
  const uint32_t* a1;
  const uint32_t* a2;
  uint32_t* out1;
  uint32_t* out2;
  Fp<FID> gamma;  // internal form, canonical
  uint32_t b, mont;
  NMX_HD void operator()(uint32_t t) const {
    const bool second = t >= b;
    const uint32_t e = second ? t - b : t;
    const Fp<FID> x = ld<FID>(second ? a2 : a1, e);
    Fp<FID> v = mont ? x.mont256_to_internal() : x.to_internal();
    if (second) v = v * gamma;
    v.canon().to_words((second ? out2 : out1) + 8 * (size_t)e);
  }
};

static constexpr uint32_t kMercurySLo = 64 + 1;    // words between two word rows of a low window (T <= 64 elements; odd: the staging
static constexpr uint32_t kMercurySHi = 128 + 1;   // stores of the 8 words of one element land in 8 banks), and of a high window (2T - 1)
// word w of element e of operand op sits at lds[(op * 8 + w) * stride + e]: the lanes of a wave read consecutive e (or all the same)
NMX_DEV void mercury_s_stage(uint32_t* lds, uint32_t stride, uint32_t op, const uint32_t* src, uint64_t first, uint32_t count, uint32_t b) {
  for (uint32_t t = NMX_TID; t < 8u * count; t += 256u) {
    const uint32_t e = t >> 3, w = t & 7u;
    const uint64_t at = first + e;
    lds[(op * 8u + w) * stride + e] = at < b ? src[8 * at + w] : 0u;
  }
}
template <int FID> NMX_DEV Fp<FID> mercury_s_at(const uint32_t* lds, uint32_t stride, uint32_t op, uint32_t e) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = lds[(op * 8u + (uint32_t)i) * stride + e];
  return Fp<FID>::from_words(w);
}

// block (kt, c) = (NMX_BID / chunks, NMX_BID % chunks), 256 threads
template <int FID> NMX_KERNEL void NMX_LAUNCH_BOUNDS(256) k_mercury_s(MercurySArgs<FID> a) {
  using F = Fp<FID>;
  NMX_LDS uint32_t lo[4 * 8 * kMercurySLo];
  NMX_LDS uint32_t hi[4 * 8 * kMercurySHi];
  NMX_LDS uint32_t red[256 * 8];
  const uint32_t T = a.tile, G = 256u / T, tid = NMX_TID;
  const uint32_t kt = NMX_BID / a.chunks, c = NMX_BID % a.chunks, k0 = kt * T;
  if (!mercury_s_chunk_live(a.b, T, a.cpt, k0, c)) return;  // (the whole block)
  const uint32_t kk = tid % T, q = tid / T;
  const uint32_t* const ops[4] = {a.a1, a.a2, a.b1, a.b2};
  F acc = F::zero();
  uint32_t pending = 0;
  for (uint32_t it = c * a.cpt; it < (c + 1u) * a.cpt; it++) {
    const uint64_t i0 = (uint64_t)it * T;
    if (i0 + k0 + 1u >= a.b) break;  // (the whole block) this tile and every later one lie outside the triangle
    for (uint32_t op = 0; op < 4; op++) {
      mercury_s_stage(lo, kMercurySLo, op, ops[op], i0, T, a.b);
      mercury_s_stage(hi, kMercurySHi, op, ops[op], i0 + k0 + 1u, 2u * T - 1u, a.b);
    }
    NMX_SYNC();
    for (uint32_t ii = q; ii < T; ii += G) {
      const uint32_t e = ii + kk;
      const F x[4] = {mercury_s_at<FID>(hi, kMercurySHi, 0, e), mercury_s_at<FID>(lo, kMercurySLo, 0, ii),
                      mercury_s_at<FID>(hi, kMercurySHi, 1, e), mercury_s_at<FID>(lo, kMercurySLo, 1, ii)};
      const F y[4] = {mercury_s_at<FID>(lo, kMercurySLo, 2, ii), mercury_s_at<FID>(hi, kMercurySHi, 2, e),
                      mercury_s_at<FID>(lo, kMercurySLo, 3, ii), mercury_s_at<FID>(hi, kMercurySHi, 3, e)};
      acc = acc + F::template dot<4>(x, y);  // + (< 1.19 p)
      if (++pending == 6) {
        acc = acc.norm();
        acc.check_below(8.2, "k_mercury_s: lane sum");
        acc = acc.canon();
        pending = 0;
      }
    }
    NMX_SYNC();  // the windows are restaged
  }
  acc.norm().canon().to_words(red + 8 * tid);
  NMX_SYNC();
  const uint64_t k = (uint64_t)k0 + kk;
  if (q == 0 && k + 1u < a.b) {
    F s = F::zero();
    pending = 0;
    for (uint32_t g = 0; g < G; g++) {
      s = s + F::from_words(red + 8 * (g * T + kk));
      if (++pending == 6) s = s.norm().canon(), pending = 0;
    }
    s = s.norm();
    s.check_below(7.0, "k_mercury_s: meet");
    uint32_t* dst = a.chunks > 1 ? a.part + 8 * ((size_t)c * (a.b - 1u)) : a.out;
    s.canon().to_words(dst + 8 * k);
  }
}

// out[k] = the sum of the partials of k's live chunks (chunks > 1 only), b - 1 lanes
template <int FID> struct MercurySFinishFn {
  const uint32_t* part;
  uint32_t* out;
  uint32_t b, tile, chunks, cpt;
  NMX_HD void operator()(uint32_t k) const {
    using F = Fp<FID>;
    const uint32_t k0 = k / tile * tile;
    F s = F::zero();
    uint32_t pending = 0;
    for (uint32_t c = 0; c < chunks && mercury_s_chunk_live(b, tile, cpt, k0, c); c++) {
      s = s + ld<FID>(part, (size_t)c * (b - 1u) + k);
      if (++pending == 6) s = s.norm().canon(), pending = 0;
    }
    s.norm().canon().to_words(out + 8 * (size_t)k);
  }
};

// d = g reversed (mercury.rs:1113-1120): out[i] = in[n - 1 - i], words copied as stored
struct MercuryReverseFn {
  const uint32_t* in;
  uint32_t* out;
  uint32_t n;
  NMX_HD void operator()(uint32_t i) const {
#pragma unroll
    for (int w = 0; w < 8; w++) out[8 * (size_t)i + w] = in[8 * (size_t)(n - 1u - i) + w];
  }
};

#if defined(__HIPCC__) || defined(__HIP__)
// ---- the host half ---------------------------------------------------------------------------------------------------------------
// workspace bytes of one call with device operands: the two converted tables and the partials
static inline size_t mercury_s_workspace(size_t b, const MercurySPlan& pl) {
  return 2 * pad256(b * 32) + (pl.chunks > 1 ? pad256((size_t)pl.chunks * (b - 1) * 32) : 0);
}
// everything device-resident, enqueued on the backend's stream; `ws` holds mercury_s_workspace bytes.  gamma: internal form, canonical.
template <int FID>
static void mercury_s_enqueue(DeviceBackend& be, const MercurySPlan& pl, char* ws, const uint32_t* a1, const uint32_t* b1, const uint32_t* a2,
                              const uint32_t* b2, size_t b, const Fp<FID>& gamma, bool mont, uint32_t* out) {
  uint32_t* t1 = (uint32_t*)ws;
  uint32_t* t2 = (uint32_t*)(ws + pad256(b * 32));
  MercurySArgs<FID> a;
  a.a1 = t1, a.a2 = t2, a.b1 = b1, a.b2 = b2;
  a.part = (uint32_t*)(ws + 2 * pad256(b * 32));
  a.out = out;
  a.b = (uint32_t)b, a.tile = pl.tile, a.chunks = pl.chunks, a.cpt = pl.cpt;
  be.launch(MercurySPrepFn<FID>{a1, a2, t1, t2, gamma, (uint32_t)b, mont ? 1u : 0u}, (uint32_t)(2 * b));
  be.launch_kernel(k_mercury_s<FID>, pl.ktiles * pl.chunks, 256, a);
  if (pl.chunks > 1) be.launch(MercurySFinishFn<FID>{a.part, out, a.b, pl.tile, pl.chunks, pl.cpt}, (uint32_t)(b - 1));
}

static inline MercurySPlan mercury_s_plan_now(size_t b) { return mercury_s_plan(b, G.mercury_s_tile.load(std::memory_order_relaxed)); }

template <int FID>
static void mercury_s_t(Ctx& c, const void* a1, const void* b1, const void* a2, const void* b2, size_t b, const void* gamma, uint32_t flags, void* out_s) {
  const bool dev = flags & NMX_SCALARS_DEVICE, async = dev && (flags & NMX_ASYNC), mont = flags & NMX_SCALARS_MONT;
  const Fp<FID> ga = challenge<FID>(gamma, mont);  // NMX_E_SCALAR_RANGE before anything is enqueued
  if (b == 1) return;                              // nothing to write
  const MercurySPlan pl = mercury_s_plan_now(b);
  const size_t wsb = mercury_s_workspace(b, pl);
  arena_reserve(c, wsb + (dev ? 0 : 4 * pad256(b * 32) + pad256((b - 1) * 32)) + 256);
  MercuryArena ws{c};
  char* w = ws.take(wsb);
  const uint32_t* d1 = ws.in(a1, b, dev);
  const uint32_t* e1 = ws.in(b1, b, dev);
  const uint32_t* d2 = ws.in(a2, b, dev);
  const uint32_t* e2 = ws.in(b2, b, dev);
  uint32_t* dout = dev ? (uint32_t*)out_s : (uint32_t*)ws.take((b - 1) * 32);
  const bool prof = G.profiling;
  DeviceBackend be(c, false, prof);
  try {
    be.mark("kernel");
    mercury_s_enqueue<FID>(be, pl, w, d1, e1, d2, e2, b, ga, mont, dout);
    be.mark("end");
    if (!dev) HIPCHK(hipMemcpyAsync(out_s, dout, (b - 1) * 32, hipMemcpyDeviceToHost, c.stream));
  } catch (...) {
    (void)hipStreamSynchronize(c.stream);
    throw;
  }
  mercury_finish(c, be, prof, async);
}

void fv_mercury_reverse(Ctx& c, const uint32_t* in, size_t n, uint32_t* out) {
  DeviceBackend be(c, false, false);
  be.launch(MercuryReverseFn{in, out, (uint32_t)n}, (uint32_t)n);
}
void fv_mercury_s_poly(Ctx& c, int field, const void* a1, const void* b1, const void* a2, const void* b2, size_t b, const void* gamma, uint32_t flags,
                       void* out_s) {
  with_field(field, [&](auto F) { mercury_s_t<F()>(c, a1, b1, a2, b2, b, gamma, flags, out_s); });
}
#endif

}  // namespace nmx
