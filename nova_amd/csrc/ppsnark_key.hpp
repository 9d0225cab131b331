// ppsnark_key.hpp -- the prover key's share of the sixteen tables of the pre-processing SNARK's inner sum-check (sumcheck_ppsnark.hpp), from
// matrices that are already resident in HBM (nmx_spmv_register):
//     spark_repr   R1CSShapeSparkRepr::new (src/spartan/ppsnark.rs:117-190 of the reference): row, col, one value vector per matrix, ts_row,
//                  ts_col, every one n field elements.  Entry e of matrix j is storage index e of its CSR arrays (the order of
//                  SparseMatrix::iter, src/r1cs/sparse.rs:332-390), the matrices chained in the order of the handles.
// The masked eq table (MaskedEqPolynomial::evals) needs no kernel of its own: capi.hip runs the eq pass and clears the prefix on the stream.
// Included at the end of fieldvec.hip (after ppsnark_oracles.hpp, whose pps_small and arena helper it uses).  The lane bodies use block-level
// primitives only (LDS, the block barrier, atomics), so tests/host_emul/ppsnark_key_emul.cpp runs them on the CPU (simt.hpp).
//
// Three launches (two when ts_col is not asked for):
//   expand   PpsKeyExpandFn, one lane per i < n.  i < total: the matrix j with off[j] <= i < off[j + 1] by at most 8 compares, e = i - off[j],
//            the row r with indptr[r] <= e < indptr[r + 1] by a binary search of indptr (at most 32 steps: rows < 2^31), the column
//            indices[e] & mask (the coefficient-class bits ride above the mask, spmv_row.hpp).  i >= total: row 0, column n - 1, no value.
//            The lane writes row[i], col[i] and element i of EVERY value vector (the entry's value in matrix j's, zero in the others), so each
//            output element is written exactly once.  The same lane writes ts_row[i] = sum_j (indptr_j[i + 1] - indptr_j[i]) (+ n - total at
//            i = 0): the row histogram is a difference of indptr and needs no atomics.
//   hist     k_pps_key_hist, one block of 256 threads per tile of 2048 entries of the chained entry stream: the column histogram in 32-bit
//            integers, into n zeroed words.  The constant-one column of an R1CS matrix can hold an entry per constraint, so one global atomic
//            per entry would queue a third of all entries on one address.  A block therefore counts in an LDS table of 1024 (column, count)
//            slots first: an entry hashes its column to a slot and probes AT MOST 8 slots for one that holds its column or is empty (claimed
//            by one compare-and-swap); it then adds 1 to the slot's LDS counter.  An entry that finds neither in 8 probes adds 1 to the global
//            counter directly.  After a barrier each occupied slot is flushed with one global atomic.  Per block the heavy column costs one
//            global atomic instead of ~700.
//   finish   PpsKeyTsColFn, one lane per a < n: ts_col[a] = count[a] (+ n - total at a = n - 1) as a field element.
// No loop waits for another lane or block: a failed compare-and-swap moves to the next probe and is never retried.  Trip counts: 8 matrix
// compares, 32 search steps, 8 entries per thread x 8 probes, 4 flush slots per thread -- none depends on the data.  Integer adds are exact
// and commute, so the result does not depend on the order the atomics land in.
//
// Forms.  F = 1 for canonical words, 2^256 for Montgomery words (NMX_SCALARS_MONT); R = 2^261, a (x) b = a b / R.  An integer v < 2^32
// becomes v F by one product, small(v) (x) (F R) (`form`, canonical).  The resident data is x R (spmv_convert_t) whatever form the matrix was
// registered in; x R (x) F (`vscale`, canonical: 1 or 2^256 mod p) = x F.  Both products have a canonical factor and a factor below p, so they
// are below 1.01 p and st() stores the canonical representative.
#pragma once

#include "ppsnark_oracles.hpp"  // pps_small; NMX_DEV / NMX_KERNEL / NMX_LDS (msm_partition.hpp); ld / st (spmv_row.hpp)

namespace nmx {

static constexpr uint32_t kPpsKeyMaxMats = 8;
static constexpr uint32_t kPpsKeyThreads = 256;   // threads per block of the histogram
static constexpr uint32_t kPpsKeyPer = 8;         // entries per thread: a tile is 2048 entries
static constexpr uint32_t kPpsKeyTile = kPpsKeyThreads * kPpsKeyPer;
static constexpr uint32_t kPpsKeySlotBits = 10;   // 1024 (column, count) slots: 8 KiB of LDS
static constexpr uint32_t kPpsKeySlots = 1u << kPpsKeySlotBits;
static constexpr uint32_t kPpsKeyProbes = 8;
static constexpr uint32_t kPpsKeyEmpty = 0xffffffffu;  // no column: masked indices are below 2^31

// compare-and-swap on an LDS word: the old value (the plain read-modify-write where one thread runs at a time)
NMX_HD uint32_t pps_key_cas(uint32_t* p, uint32_t expect, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS(p, expect, v);
#else
  const uint32_t o = *p;
  if (o == expect) *p = v;
  return o;
#endif
}

// the matrices as the kernels see them: entries off[j] .. off[j + 1] of the chained stream are matrix j's
struct PpsKeyMats {
  const uint32_t* indptr[kPpsKeyMaxMats];
  const uint32_t* indices[kPpsKeyMaxMats];
  const uint32_t* data[kPpsKeyMaxMats];
  uint32_t off[kPpsKeyMaxMats + 1];
  uint32_t rows[kPpsKeyMaxMats];
  uint32_t mask[kPpsKeyMaxMats];  // spmv_index_mask(cols)
  uint32_t k, n, total;           // total = off[k] <= n
};

// ---- expand: row, col, the value vectors, ts_row --------------------------------------------------------------------------------------
template <int FID> struct PpsKeyExpandFn {
  PpsKeyMats m;
  uint32_t *row, *col, *ts_row;     // any may be NULL: not computed
  uint32_t* vals[kPpsKeyMaxMats];   // entries j < k may be NULL
  Fp<FID> form;                     // F R, canonical
  Fp<FID> vscale;                   // F, canonical
  NMX_HD void operator()(uint32_t i) const {
    using F = Fp<FID>;
    const uint32_t *ip = nullptr, *ix = nullptr, *dt = nullptr;
    uint32_t jm = kPpsKeyMaxMats, e = 0, rows = 0, mask = 0;
    if (i < m.total) {
#pragma unroll
      for (uint32_t q = 0; q < kPpsKeyMaxMats; q++)
        if (q < m.k && i >= m.off[q]) jm = q, e = i - m.off[q], ip = m.indptr[q], ix = m.indices[q], dt = m.data[q], rows = m.rows[q], mask = m.mask[q];
    }
    uint32_t r = 0, c = m.n - 1u;
    if (jm < kPpsKeyMaxMats) {
      // the last r with indptr[r] <= e: indptr[0] = 0 <= e < nnz = indptr[rows], so indptr[lo] <= e < indptr[hi] throughout
      uint32_t lo = 0, hi = rows;
      for (uint32_t s = 0; s < 32 && hi - lo > 1; s++) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ip[mid] <= e) lo = mid;
        else hi = mid;
      }
      r = lo, c = ix[e] & mask;
    }
    if (row) st<FID>(row, i, pps_small<FID>(r) * form);
    if (col) st<FID>(col, i, pps_small<FID>(c) * form);
#pragma unroll
    for (uint32_t q = 0; q < kPpsKeyMaxMats; q++) {
      if (q >= m.k || !vals[q]) continue;
      if (q == jm) {
        const F x = ld<FID>(dt, e) * vscale;
        x.check_below(1.05, "PpsKeyExpandFn: data * F");
        st<FID>(vals[q], i, x);
      } else {
#pragma unroll
        for (int w = 0; w < 8; w++) vals[q][8 * (size_t)i + w] = 0u;
      }
    }
    if (ts_row) {
      uint32_t cnt = i == 0 ? m.n - m.total : 0u;  // <= n in all: every entry and every padding element counts once
#pragma unroll
      for (uint32_t q = 0; q < kPpsKeyMaxMats; q++)
        if (q < m.k && i < m.rows[q]) cnt += m.indptr[q][i + 1] - m.indptr[q][i];
      st<FID>(ts_row, i, pps_small<FID>(cnt) * form);
    }
  }
};

// ---- hist: the column histogram --------------------------------------------------------------------------------------------------------
struct PpsKeyHistArgs {
  PpsKeyMats m;
  uint32_t* count;  // n words, zero before the launch
};
NMX_DEV uint32_t pps_key_slot(uint32_t col) { return (col * 0x9e3779b1u) >> (32 - kPpsKeySlotBits); }
// grid = ceil(total / kPpsKeyTile) blocks of kPpsKeyThreads threads.  (A template only to get inline linkage, as the kernels of msm_partition.hpp.)
template <int UNUSED> NMX_KERNEL void NMX_LAUNCH_BOUNDS(256) k_pps_key_hist(PpsKeyHistArgs a) {
  NMX_LDS uint32_t key[kPpsKeySlots];
  NMX_LDS uint32_t cnt[kPpsKeySlots];
  const uint32_t t = NMX_TID;
  for (uint32_t s = t; s < kPpsKeySlots; s += kPpsKeyThreads) key[s] = kPpsKeyEmpty, cnt[s] = 0u;
  NMX_SYNC();
  const uint64_t base = (uint64_t)NMX_BID * kPpsKeyTile;
  for (uint32_t u = 0; u < kPpsKeyPer; u++) {
    const uint64_t g64 = base + (uint64_t)u * kPpsKeyThreads + t;
    if (g64 >= a.m.total) continue;
    const uint32_t g = (uint32_t)g64;
    uint32_t col = 0;
#pragma unroll
    for (uint32_t q = 0; q < kPpsKeyMaxMats; q++)
      if (q < a.m.k && g >= a.m.off[q] && g < a.m.off[q + 1]) col = a.m.indices[q][g - a.m.off[q]] & a.m.mask[q];
    const uint32_t h = pps_key_slot(col);
    bool placed = false;
    for (uint32_t pr = 0; pr < kPpsKeyProbes && !placed; pr++) {
      const uint32_t s = (h + pr) & (kPpsKeySlots - 1u);
      uint32_t cur = *(volatile uint32_t*)&key[s];
      if (cur == kPpsKeyEmpty) {
        cur = pps_key_cas(&key[s], kPpsKeyEmpty, col);  // lost to another column: the next probe, never this one again
        if (cur == kPpsKeyEmpty) cur = col;
      }
      if (cur == col) {
        nmx_atomic_add(&cnt[s], 1u);
        placed = true;
      }
    }
    if (!placed) nmx_atomic_add(&a.count[col], 1u);
  }
  NMX_SYNC();
  for (uint32_t s = t; s < kPpsKeySlots; s += kPpsKeyThreads)
    if (key[s] != kPpsKeyEmpty) nmx_atomic_add(&a.count[key[s]], cnt[s]);
}

// ---- finish: the counts as field elements ----------------------------------------------------------------------------------------------
template <int FID> struct PpsKeyTsColFn {
  const uint32_t* count;
  uint32_t* ts_col;
  uint32_t n, total;
  Fp<FID> form;
  NMX_HD void operator()(uint32_t a) const {
    const uint32_t v = count[a] + (a == n - 1u ? n - total : 0u);
    st<FID>(ts_col, a, pps_small<FID>(v) * form);
  }
};

#if defined(__HIPCC__) || defined(__HIP__)
// ---- the host half ---------------------------------------------------------------------------------------------------------------------
// Handles, shapes, n, NULLs and overlaps are the caller's to check (capi.hip); mats[j] / nnz[j]: matrix j and its entry count.
template <int FID>
static void pps_key_t(Ctx& c, const CsrView* mats, const size_t* nnz, size_t k, size_t n, uint32_t flags, void* o_row, void* o_col,
                      void* const* o_vals, void* o_ts_row, void* o_ts_col) {
  using F = Fp<FID>;
  using H = HostFp4<FID>;
  const bool mont = flags & NMX_SCALARS_MONT, dev = flags & NMX_SCALARS_DEVICE;
  size_t n_out = (o_row != nullptr) + (o_col != nullptr) + (o_ts_row != nullptr) + (o_ts_col != nullptr);
  for (size_t j = 0; j < k && o_vals; j++) n_out += o_vals[j] != nullptr;
  if (n_out == 0) return;
  arena_reserve(c, pad256(n * 4) + (dev ? 0 : n_out * pad256(n * 32)) + 256);
  MercuryArena ws{c};
  uint32_t* count = (uint32_t*)ws.take(n * 4);
  std::vector<std::pair<void*, void*>> back;  // (device, host) of the staged outputs
  auto outp = [&](void* p) -> uint32_t* {
    if (!p || dev) return (uint32_t*)p;
    char* d = ws.take(n * 32);
    back.push_back({d, p});
    return (uint32_t*)d;
  };
  PpsKeyMats m{};
  size_t total = 0;
  for (size_t j = 0; j < k; j++) {
    m.indptr[j] = mats[j].indptr, m.indices[j] = mats[j].indices, m.data[j] = mats[j].data;
    m.off[j] = (uint32_t)total, m.rows[j] = (uint32_t)mats[j].rows, m.mask[j] = spmv_index_mask(mats[j].cols);
    total += nnz[j];
  }
  for (size_t j = k; j <= kPpsKeyMaxMats; j++) m.off[j] = (uint32_t)total;
  m.k = (uint32_t)k, m.n = (uint32_t)n, m.total = (uint32_t)total;
  uint32_t fw[8], vw[8];
  H::pow2(mont ? 517 : 261).to_canonical(fw);  // F R
  H::pow2(mont ? 256 : 0).to_canonical(vw);    // F
  PpsKeyExpandFn<FID> ex{};
  ex.m = m, ex.form = F::from_words(fw), ex.vscale = F::from_words(vw);
  ex.row = outp(o_row), ex.col = outp(o_col), ex.ts_row = outp(o_ts_row);
  for (size_t j = 0; j < k; j++) ex.vals[j] = outp(o_vals ? o_vals[j] : nullptr);
  uint32_t* d_ts_col = outp(o_ts_col);
  const bool prof = G.profiling;
  DeviceBackend be(c, false, prof);
  try {
    be.mark("kernel");
    if (n_out > (size_t)(o_ts_col != nullptr)) be.launch(ex, (uint32_t)n);  // (ts_col alone needs no expansion)
    if (d_ts_col) {
      be.memset0(count, n * 4);
      be.launch_kernel(k_pps_key_hist<0>, (uint32_t)((total + kPpsKeyTile - 1) / kPpsKeyTile), kPpsKeyThreads, PpsKeyHistArgs{m, count});
      be.launch(PpsKeyTsColFn<FID>{count, d_ts_col, (uint32_t)n, (uint32_t)total, ex.form}, (uint32_t)n);
    }
    be.mark("end");
    for (auto& b : back) HIPCHK(hipMemcpyAsync(b.second, b.first, n * 32, hipMemcpyDeviceToHost, c.stream));
    stream_wait(c.stream);
  } catch (...) {
    (void)hipStreamSynchronize(c.stream);  // nothing of this call still writes the caller's vectors
    throw;
  }
  if (prof && be.nmarks == 2) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
    prof_store(&ms, 1);
  }
}

void fv_ppsnark_spark_repr(Ctx& c, int field, const CsrView* mats, const size_t* nnz, size_t k, size_t n, uint32_t flags, void* out_row,
                           void* out_col, void* const* out_vals, void* out_ts_row, void* out_ts_col) {
  with_field(field, [&](auto F) { pps_key_t<F()>(c, mats, nnz, k, n, flags, out_row, out_col, out_vals, out_ts_row, out_ts_col); });
}
#endif

}  // namespace nmx
