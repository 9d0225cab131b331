// mercury.hpp -- the two N-sized passes of Mercury's prover (src/provider/mercury.rs of the reference) that nothing else in the C ABI can
// express, over a polynomial f of n_rows * n_cols coefficients resident in HBM, viewed as an n_rows x n_cols matrix (row-major):
//     compute_h_poly      (mercury.rs:369-386)   h[row] = sum_col f[row * n_cols + col] * eq_col[col]
//     divide_by_binomial  (mercury.rs:319-356, with divide_by_linear_polynomial :281-288 and transpose :291-312)
//                         f(X) = (X^n_cols - alpha) q(X) + g(X)
// Included at the end of fieldvec.hip.  The lane bodies use no wave-level intrinsic, so tests/host_emul runs them on the CPU (simt.hpp);
// the plan of the division (mercury_plan, mercury_alpha_pow) is plain C++ and tests/cpp/mercury_mirror_test.cpp runs it under g++.
//
// The division, column by column.  With T_j = f[j][c] + alpha T_{j+1}, T_{n_rows} = 0 (Horner from the top row down):
//     g[c] = T_0                                  = sum_j       f[j][c] alpha^j
//     q[k * n_cols + c] = T_{k+1}, k < n_rows - 1 = sum_{j > k} f[j][c] alpha^(j - k - 1)
// which is the reference's per-column divide_by_linear_polynomial followed by its transpose, without the all-zero tail of its b * b vector.
// A lane per column would be 16 waves at 1024 x 1024, so the rows are cut into `segs` segments of `seg_rows` rows (the top one may be
// shorter) and the recurrence runs in three launches, none of which waits for another block:
//     k_mercury_div_totals   lane (s, c), s >= 1: L_s = the local Horner total of segment s with a zero carry       -> tot[s][c]
//     k_mercury_div_carries  lane c: T_{(S-1) R} = L_{S-1};  T_{s R} = L_s + alpha^R T_{(s+1) R}  (only the TOP segment can be short and its
//                            carry is zero, so alpha^R is the only power needed: computed once on the host)          tot[s][c] <- carry into s
//     k_mercury_div_walk     lane (s, c): re-reads the segment's rows from its carry and writes q (and g from row 0)
// Traffic per division: f twice (the second read at 2^20 is 32 MiB, which the 256 MiB Infinity Cache should hold -- not isolated yet,
// DESIGN.md 3h, docs/measurements.md), q once, segs x n_cols totals written, read, rewritten and read again.  Lanes run across columns: a wave reads 2 KiB
// contiguous per row.  Results are exact (every stored value is the canonical representative), so they depend neither on the launch
// geometry nor on the option mercury_seg_rows.
//
// Forms.  alpha and alpha^R are in the internal form (e 2^261), so alpha * t is in t's form: canonical words and Montgomery words
// (NMX_SCALARS_MONT) take the same kernels.  h needs a product of two stored values: eq_col is brought into the internal form ONCE by
// a prologue launch (MercuryEqFn, which writes it [word][column]) and every block copies that table into LDS when it fits (<= 2048
// columns: 64 KiB).
//
// Bounds (p = the modulus; a product of operands below a p and b p with a b < 127 is normalised and below p (1 + a b / 127); stored
// coefficients may be any 256-bit words, 2^256 < 6 p for all four fields):
//   totals   t < 7.1 p:  alpha (canonical, < p) * t < 1.06 p, + f (< 6 p) < 7.06 p; limbs of the sum < 2^30 -> norm()
//   walk     t canonical after every step ((< 7.02 p).norm().canon()): it is what is stored
//   carries  L canonical + alpha^R * c (< 1.01 p) < 2.01 p -> norm().canon()
//   h lane   f * eq (< 6 p x < p) < 1.05 p per term; a canonical accumulator plus six terms < 7.3 p < 16 p, limbs < 7 * 2^29 -> norm().canon()
//   h wave   64 canonical lane sums added through shuffles (wave_total: < 64 p < 2^261), one product with ONE (< 1.51 p), canon4()
#pragma once

#include "msm_partition.hpp"  // NMX_DEV: the device / emulation spelling
#include "spmv_row.hpp"       // ld / st

namespace nmx {

// ---- the host's plan of a division: plain C++ --------------------------------------------------------------------------------------
struct MercuryPlan {
  uint32_t seg_rows;   // R: rows per segment
  uint32_t segs;       // S = ceil(n_rows / R)
  uint32_t last_rows;  // rows of the top segment, 1 .. R
};
static constexpr uint32_t kMercuryLanes = 1u << 16;  // lanes the division aims for: 4 waves per CU
static constexpr uint32_t kMercuryMaxSegs = 64;      // the carry pass is a chain of S - 1 dependent products per column
static constexpr uint32_t kMercuryMinSegRows = 4;    // below that the totals are not worth their launch
static constexpr uint32_t kMercuryGridSegs = 65535;  // whatever the option says: blocks per launch = ceil(n_cols / 256) * segs < 2^25
// opt = the option mercury_seg_rows: 0 = by size, else rows per segment (clamped to n_rows).  n_rows, n_cols >= 1, n_rows < 2^32.
static inline MercuryPlan mercury_plan(size_t n_rows, size_t n_cols, uint32_t opt) {
  size_t R;
  if (opt) {
    R = opt < n_rows ? opt : n_rows;
  } else {
    size_t want = kMercuryLanes / n_cols;
    want = want < 1 ? 1 : (want > kMercuryMaxSegs ? kMercuryMaxSegs : want);
    R = (n_rows + want - 1) / want;
    R = R < kMercuryMinSegRows ? kMercuryMinSegRows : R;
    R = R > n_rows ? n_rows : R;
  }
  if ((n_rows + R - 1) / R > kMercuryGridSegs) R = (n_rows + kMercuryGridSegs - 1) / kMercuryGridSegs;  // (a tiny option on a tall shape)
  const size_t S = (n_rows + R - 1) / R;
  return {(uint32_t)R, (uint32_t)S, (uint32_t)(n_rows - (S - 1) * R)};
}
// a^e for a in the internal form, canonical; the result likewise (e = 0: ONE)
template <int FID> static inline Fp<FID> mercury_alpha_pow(const Fp<FID>& a, uint64_t e) {
  Fp<FID> r = Fp<FID>::one();
  for (int b = 63; b >= 0; b--) {
    r = r.sqr().canon();
    if ((e >> b) & 1u) r = (r * a).canon();
  }
  return r;
}

// ---- lane bodies -----------------------------------------------------------------------------------------------------------------
template <int FID> struct MercuryDivArgs {
  const uint32_t* f;   // n_rows * n_cols elements
  uint32_t* q;         // (n_rows - 1) * n_cols elements (never dereferenced when n_rows == 1)
  uint32_t* g;         // n_cols elements
  uint32_t* tot;       // segs * n_cols elements of workspace: totals, then carries (unused when segs == 1)
  Fp<FID> alpha, alpha_seg;  // alpha and alpha^seg_rows, internal form, canonical
  uint32_t n_rows, n_cols, seg_rows, segs;
};

// rows hi - 1 down to lo of one column, step(j, f[j][col]) for each: the loads of a batch of kMercuryBatch rows are all issued before
// the dependent chain consumes the first of them (a lane then has 256 B in flight instead of 32)
static constexpr int kMercuryBatch = 8;
template <int FID, class Step>
NMX_DEV void mercury_rows_down(const uint32_t* __restrict__ f, uint32_t n_cols, uint32_t col, uint32_t lo, uint32_t hi, Step&& step) {
  uint32_t j = hi;
  for (; j - lo >= (uint32_t)kMercuryBatch; j -= (uint32_t)kMercuryBatch) {
    Fp<FID> x[kMercuryBatch];
#pragma unroll
    for (int i = 0; i < kMercuryBatch; i++) x[i] = ld<FID>(f, (size_t)(j - 1u - (uint32_t)i) * n_cols + col);
#pragma unroll
    for (int i = 0; i < kMercuryBatch; i++) step(j - 1u - (uint32_t)i, x[i]);
  }
  while (j > lo) {
    j--;
    step(j, ld<FID>(f, (size_t)j * n_cols + col));
  }
}
// L_s of column col: Horner over the rows of segment seg from a zero carry (seg >= 1; segment 0's total is never needed)
template <int FID> NMX_DEV void mercury_div_total_lane(const MercuryDivArgs<FID>& a, uint32_t seg, uint32_t col) {
  using F = Fp<FID>;
  const uint32_t lo = seg * a.seg_rows, hi = a.n_rows - lo < a.seg_rows ? a.n_rows : lo + a.seg_rows;
  F t = F::zero();
  mercury_rows_down<FID>(a.f, a.n_cols, col, lo, hi, [&](uint32_t, const F& x) {
    t = (x + a.alpha * t).norm();  // < 7.1 p
    t.check_below(7.1, "mercury_div_total_lane: t");
  });
  st<FID>(a.tot, (size_t)seg * a.n_cols + col, t);
}
// tot[s][col] <- the carry INTO segment s (T of the first row above it), top segment: 0
template <int FID> NMX_DEV void mercury_div_carry_lane(const MercuryDivArgs<FID>& a, uint32_t col) {
  using F = Fp<FID>;
  F c = F::zero();
  for (uint32_t s = a.segs; s-- > 1;) {
    const size_t at = (size_t)s * a.n_cols + col;
    const F L = ld<FID>(a.tot, at);  // canonical: k_mercury_div_totals stored it
    c.to_words(a.tot + 8 * at);
    c = (L + a.alpha_seg * c).norm().canon();  // < 2.01 p -> canonical
  }
  c.to_words(a.tot + 8 * (size_t)col);
}
// the rows of segment seg once more, from the carry: row j's T_j goes to q[j - 1] (j >= 1) or g (j == 0)
template <int FID> NMX_DEV void mercury_div_walk_lane(const MercuryDivArgs<FID>& a, uint32_t seg, uint32_t col) {
  using F = Fp<FID>;
  const uint32_t lo = seg * a.seg_rows, hi = a.n_rows - lo < a.seg_rows ? a.n_rows : lo + a.seg_rows;
  F t = a.segs > 1 ? ld<FID>(a.tot, (size_t)seg * a.n_cols + col) : F::zero();  // canonical
  mercury_rows_down<FID>(a.f, a.n_cols, col, lo, hi, [&](uint32_t j, const F& x) {
    t = (x + a.alpha * t).norm().canon();  // < 7.02 p -> canonical
    if (j) t.to_words(a.q + 8 * ((size_t)(j - 1u) * a.n_cols + col));
    else t.to_words(a.g + 8 * (size_t)col);
  });
}
// (segment, column) of a thread: 256 consecutive columns of ONE segment per block, cblocks = ceil(n_cols / 256) blocks per segment
NMX_DEV bool mercury_div_where(uint32_t bid, uint32_t tid, uint32_t n_cols, uint32_t first_seg, uint32_t* seg, uint32_t* col) {
  const uint32_t cblocks = n_cols / 256u + (n_cols % 256u ? 1u : 0u);
  *seg = first_seg + bid / cblocks;
  const uint64_t c = (uint64_t)(bid % cblocks) * 256u + tid;
  *col = (uint32_t)c;
  return c < n_cols;
}

// a lane's share of one row of h: columns lane, lane + 64, ...; eq(c) -> eq_col[c] in the internal form, canonical.  Canonical result.
template <int FID, class EqAt> NMX_DEV Fp<FID> mercury_h_lane(const uint32_t* f, size_t row, uint32_t n_cols, uint32_t lane, const EqAt& eq) {
  using F = Fp<FID>;
  const uint32_t* __restrict__ fr = f + 8 * row * (size_t)n_cols;
  F acc = F::zero();
  uint32_t pending = 0;
  for (uint64_t c = lane; c < n_cols; c += 64u) {
    acc = acc + ld<FID>(fr, (size_t)c) * eq((uint32_t)c);  // + (< 1.05 p)
    if (++pending == 6) {
      acc = acc.norm().canon();
      pending = 0;
    }
  }
  return acc.norm().canon();
}
// The converted table, stored [word][column] (word w of column c at t[w * n_cols + c]): consecutive lanes read consecutive words, from
// HBM / L2 as from LDS (64 consecutive banks), and the copy into LDS is linear.  `t` is the prologue's output or its image in LDS.
template <int FID> struct MercuryEqTable {
  const uint32_t* t;
  uint32_t n_cols;
  NMX_DEV Fp<FID> operator()(uint32_t c) const {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = t[(size_t)i * n_cols + c];
    return Fp<FID>::from_words(w);
  }
};
// eq_col -> the internal form, canonical words, in the [word][column] order (the prologue of k_mercury_h; one product per column, once per call)
template <int FID> struct MercuryEqFn {
  const uint32_t* in;
  uint32_t* out;
  uint32_t n_cols, mont;
  NMX_HD void operator()(uint32_t c) const {
    const Fp<FID> e = ld<FID>(in, c);
    uint32_t w[8];
    (mont ? e.mont256_to_internal() : e.to_internal()).canon().to_words(w);
#pragma unroll
    for (int i = 0; i < 8; i++) out[(size_t)i * n_cols + c] = w[i];
  }
};

#if defined(__HIPCC__) || defined(__HIP__)
template <int FID> __global__ __launch_bounds__(256) void k_mercury_div_totals(MercuryDivArgs<FID> a) {
  uint32_t seg, col;
  if (mercury_div_where(blockIdx.x, threadIdx.x, a.n_cols, 1u, &seg, &col)) mercury_div_total_lane<FID>(a, seg, col);
}
template <int FID> __global__ __launch_bounds__(256) void k_mercury_div_carries(MercuryDivArgs<FID> a) {
  const uint64_t col = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (col < a.n_cols) mercury_div_carry_lane<FID>(a, (uint32_t)col);
}
template <int FID> __global__ __launch_bounds__(256) void k_mercury_div_walk(MercuryDivArgs<FID> a) {
  uint32_t seg, col;
  if (mercury_div_where(blockIdx.x, threadIdx.x, a.n_cols, 0u, &seg, &col)) mercury_div_walk_lane<FID>(a, seg, col);
}

struct MercuryHArgs {
  const uint32_t* f;
  const uint32_t* eq;  // internal form, canonical, [word][column] (MercuryEqFn)
  uint32_t* out;       // n_rows elements
  uint32_t n_rows, n_cols;
};
static constexpr uint32_t kMercuryHLdsCols = 2048;  // 64 KiB of LDS
// a wave per row (rows wave, wave + 4 * gridDim.x, ...): 64 lanes stride over the row's columns, one store per row
template <int FID, bool LDS> __global__ __launch_bounds__(256) void k_mercury_h(MercuryHArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  using F = Fp<FID>;
  extern __shared__ uint32_t mercury_lds[];
  if constexpr (LDS) {
    for (uint32_t i = threadIdx.x; i < 8u * a.n_cols; i += 256u) mercury_lds[i] = a.eq[i];
    __syncthreads();
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint64_t row = (uint64_t)blockIdx.x * 4u + wave; row < a.n_rows; row += (uint64_t)gridDim.x * 4u) {  // (uniform in a wave)
    F s = mercury_h_lane<FID>(a.f, (size_t)row, a.n_cols, lane, MercuryEqTable<FID>{LDS ? mercury_lds : a.eq, a.n_cols});
    s = (wave_total<FID>(s) * F::one()).canon4();  // lane 0: < 64 p -> < 1.51 p -> canonical
    if (lane == 0) s.to_words(a.out + 8 * (size_t)row);
  }
#endif
}

// ---- the host half ---------------------------------------------------------------------------------------------------------------
// host operands are staged through the context arena (as VecIO does); device operands are used in place
struct MercuryArena {
  Ctx& c;
  size_t used = 0;
  char* take(size_t bytes) {
    char* d = c.arena + used;
    used += pad256(bytes);
    return d;
  }
  const uint32_t* in(const void* p, size_t elems, bool dev) {
    if (dev) return (const uint32_t*)p;
    char* d = take(elems * 32);
    HIPCHK(hipMemcpyAsync(d, p, elems * 32, hipMemcpyHostToDevice, c.stream));
    return (const uint32_t*)d;
  }
};
static void mercury_finish(Ctx& c, DeviceBackend& be, bool prof, bool async) {
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

template <int FID>
static void mercury_h_t(Ctx& c, const void* f, size_t n_rows, size_t n_cols, const void* eq_col, uint32_t flags, void* out_h) {
  const bool dev = flags & NMX_SCALARS_DEVICE, async = dev && (flags & NMX_ASYNC);
  const size_t n = n_rows * n_cols;
  arena_reserve(c, pad256(n_cols * 32) + (dev ? 0 : pad256(n * 32) + pad256(n_cols * 32) + pad256(n_rows * 32)) + 256);
  MercuryArena ws{c};
  uint32_t* eq_i = (uint32_t*)ws.take(n_cols * 32);
  const uint32_t* df = ws.in(f, n, dev);
  const uint32_t* deq = ws.in(eq_col, n_cols, dev);
  uint32_t* dout = dev ? (uint32_t*)out_h : (uint32_t*)ws.take(n_rows * 32);
  const bool prof = G.profiling;
  DeviceBackend be(c, false, prof);
  try {
    be.mark("kernel");
    be.launch(MercuryEqFn<FID>{deq, eq_i, (uint32_t)n_cols, (flags & NMX_SCALARS_MONT) ? 1u : 0u}, (uint32_t)n_cols);
    const MercuryHArgs a{df, eq_i, dout, (uint32_t)n_rows, (uint32_t)n_cols};
    const size_t blocks = (n_rows + 3) / 4;
    const dim3 grid((uint32_t)(blocks < 2048 ? blocks : 2048));
    if (n_cols <= kMercuryHLdsCols) hipLaunchKernelGGL((k_mercury_h<FID, true>), grid, dim3(256), n_cols * 32, c.stream, a);
    else hipLaunchKernelGGL((k_mercury_h<FID, false>), grid, dim3(256), 0, c.stream, a);
    HIPCHK(hipGetLastError());
    be.mark("end");
    if (!dev) HIPCHK(hipMemcpyAsync(out_h, dout, n_rows * 32, hipMemcpyDeviceToHost, c.stream));
  } catch (...) {
    (void)hipStreamSynchronize(c.stream);
    throw;
  }
  mercury_finish(c, be, prof, async);
}

template <int FID>
static void mercury_div_t(Ctx& c, const void* f, size_t n_rows, size_t n_cols, const void* alpha, uint32_t flags, void* out_q, void* out_g) {
  using F = Fp<FID>;
  const bool dev = flags & NMX_SCALARS_DEVICE, async = dev && (flags & NMX_ASYNC);
  const size_t n = n_rows * n_cols, nq = n - n_cols;
  const MercuryPlan pl = mercury_plan(n_rows, n_cols, G.mercury_seg_rows.load(std::memory_order_relaxed));
  const F al = challenge<FID>(alpha, flags & NMX_SCALARS_MONT);  // NMX_E_SCALAR_RANGE before anything is enqueued
  const size_t tot_bytes = pl.segs > 1 ? (size_t)pl.segs * n_cols * 32 : 0;
  arena_reserve(c, pad256(tot_bytes) + (dev ? 0 : pad256(n * 32) + pad256(nq * 32) + pad256(n_cols * 32)) + 256);
  MercuryArena ws{c};
  MercuryDivArgs<FID> a;
  a.tot = (uint32_t*)ws.take(tot_bytes);
  a.f = ws.in(f, n, dev);
  a.q = dev ? (uint32_t*)out_q : (uint32_t*)ws.take(nq * 32);
  a.g = dev ? (uint32_t*)out_g : (uint32_t*)ws.take(n_cols * 32);
  a.alpha = al, a.alpha_seg = mercury_alpha_pow<FID>(al, pl.seg_rows);
  a.n_rows = (uint32_t)n_rows, a.n_cols = (uint32_t)n_cols, a.seg_rows = pl.seg_rows, a.segs = pl.segs;
  const bool prof = G.profiling;
  DeviceBackend be(c, false, prof);
  try {
    be.mark("kernel");
    const uint32_t cblocks = (uint32_t)((n_cols + 255) / 256);
    if (pl.segs > 1) {
      be.launch_kernel(k_mercury_div_totals<FID>, cblocks * (pl.segs - 1), 256, a);
      be.launch_kernel(k_mercury_div_carries<FID>, cblocks, 256, a);
    }
    be.launch_kernel(k_mercury_div_walk<FID>, cblocks * pl.segs, 256, a);
    be.mark("end");
    if (!dev) {
      if (nq) HIPCHK(hipMemcpyAsync(out_q, a.q, nq * 32, hipMemcpyDeviceToHost, c.stream));
      HIPCHK(hipMemcpyAsync(out_g, a.g, n_cols * 32, hipMemcpyDeviceToHost, c.stream));
    }
  } catch (...) {
    (void)hipStreamSynchronize(c.stream);
    throw;
  }
  mercury_finish(c, be, prof, async);
}

void fv_mercury_h_poly(Ctx& c, int field, const void* f, size_t n_rows, size_t n_cols, const void* eq_col, uint32_t flags, void* out_h) {
  with_field(field, [&](auto F) { mercury_h_t<F()>(c, f, n_rows, n_cols, eq_col, flags, out_h); });
}
void fv_mercury_divide_by_binomial(Ctx& c, int field, const void* f, size_t n_rows, size_t n_cols, const void* alpha, uint32_t flags,
                                   void* out_q, void* out_g) {
  with_field(field, [&](auto F) { mercury_div_t<F()>(c, f, n_rows, n_cols, alpha, flags, out_q, out_g); });
}
#endif

}  // namespace nmx
