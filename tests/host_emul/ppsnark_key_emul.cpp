// tests/host_emul/ppsnark_key_emul.cpp -- TEST-ONLY: the kernels of nova_amd/csrc/ppsnark_key.hpp on the CPU, one fiber per thread (simt.hpp),
// limb bounds asserted (NMX_DEBUG_BOUNDS): the expansion pass, the block-level column histogram with its LDS table, barriers and fall-back,
// and the finish pass, with the kernels' own index maps.  The constants of the passes (F R and F) come from the test
// (tests/test_ppsnark_key_abi.py) in big integers, and so do the resident arrays (indices with their class bits, data in the internal form),
// so neither the host half of the call nor the registration is trusted here.
// NOT emulated: the launches, the staging, the concurrency of the atomics (one thread runs at a time).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/msm_pipeline.hpp"
#include "../../nova_amd/csrc/ppsnark_key.hpp"

using namespace nmx;

static PpsKeyMats make_mats(uint32_t k, uint32_t n, const uint32_t* const* indptr, const uint32_t* const* indices, const uint32_t* const* data,
                            const uint32_t* nnz, const uint32_t* rows, const uint32_t* cols) {
  PpsKeyMats m{};
  uint32_t total = 0;
  for (uint32_t j = 0; j < k; j++) {
    m.indptr[j] = indptr[j], m.indices[j] = indices[j], m.data[j] = data ? data[j] : nullptr;
    m.off[j] = total, m.rows[j] = rows[j], m.mask[j] = spmv_index_mask(cols[j]);
    total += nnz[j];
  }
  for (uint32_t j = k; j <= kPpsKeyMaxMats; j++) m.off[j] = total;
  m.k = k, m.n = n, m.total = total;
  return m;
}

// consts: F R then F, 8 words each, canonical
template <int FID>
static void run_expand(const PpsKeyMats& m, const uint32_t* consts, uint32_t* row, uint32_t* col, uint32_t* const* vals, uint32_t* ts_row) {
  PpsKeyExpandFn<FID> f{};
  f.m = m, f.row = row, f.col = col, f.ts_row = ts_row;
  for (uint32_t j = 0; j < m.k; j++) f.vals[j] = vals ? vals[j] : nullptr;
  f.form = Fp<FID>::from_words(consts), f.vscale = Fp<FID>::from_words(consts + 8);
  const uint32_t n = m.n;
  simt::launch((n + 255) / 256, 256, [&] {
    const uint32_t i = simt::bid() * 256u + simt::tid();
    if (i < n) f(i);
  });
}
extern "C" int emul_pps_key_expand(int fid, uint32_t k, uint32_t n, const uint32_t* const* indptr, const uint32_t* const* indices,
                                   const uint32_t* const* data, const uint32_t* nnz, const uint32_t* rows, const uint32_t* cols,
                                   const uint32_t* consts, uint32_t* row, uint32_t* col, uint32_t* const* vals, uint32_t* ts_row) {
  if (!k || k > kPpsKeyMaxMats || !n) return -1;
  const PpsKeyMats m = make_mats(k, n, indptr, indices, data, nnz, rows, cols);
  if (m.total > n) return -1;
  switch (fid) {
    case 0: run_expand<0>(m, consts, row, col, vals, ts_row); break;
    case 1: run_expand<1>(m, consts, row, col, vals, ts_row); break;
    case 2: run_expand<2>(m, consts, row, col, vals, ts_row); break;
    case 3: run_expand<3>(m, consts, row, col, vals, ts_row); break;
    default: return -1;
  }
  return 0;
}

// count: n words, zero on entry
extern "C" int emul_pps_key_hist(uint32_t k, uint32_t n, const uint32_t* const* indptr, const uint32_t* const* indices, const uint32_t* nnz,
                                 const uint32_t* rows, const uint32_t* cols, uint32_t* count) {
  if (!k || k > kPpsKeyMaxMats || !n) return -1;
  const PpsKeyHistArgs a{make_mats(k, n, indptr, indices, nullptr, nnz, rows, cols), count};
  if (a.m.total > n) return -1;
  const uint32_t grid = (a.m.total + kPpsKeyTile - 1) / kPpsKeyTile;
  if (grid) simt::launch(grid, kPpsKeyThreads, [&] { k_pps_key_hist<0>(a); });
  return 0;
}

template <int FID> static void run_ts_col(const uint32_t* count, uint32_t* ts_col, uint32_t n, uint32_t total, const uint32_t* form) {
  const PpsKeyTsColFn<FID> f{count, ts_col, n, total, Fp<FID>::from_words(form)};
  simt::launch((n + 255) / 256, 256, [&] {
    const uint32_t a = simt::bid() * 256u + simt::tid();
    if (a < n) f(a);
  });
}
extern "C" int emul_pps_key_ts_col(int fid, const uint32_t* count, uint32_t* ts_col, uint32_t n, uint32_t total, const uint32_t* form) {
  switch (fid) {
    case 0: run_ts_col<0>(count, ts_col, n, total, form); break;
    case 1: run_ts_col<1>(count, ts_col, n, total, form); break;
    case 2: run_ts_col<2>(count, ts_col, n, total, form); break;
    case 3: run_ts_col<3>(count, ts_col, n, total, form); break;
    default: return -1;
  }
  return 0;
}

// the histogram's geometry and hash, so that a test can tell from its own inputs whether a tile must take the fall-back
extern "C" void emul_pps_key_geometry(uint32_t* out4) { out4[0] = kPpsKeyTile, out4[1] = kPpsKeySlots, out4[2] = kPpsKeyProbes, out4[3] = kPpsKeyThreads; }
extern "C" uint32_t emul_pps_key_slot(uint32_t col) { return pps_key_slot(col); }
