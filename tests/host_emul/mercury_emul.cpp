// tests/host_emul/mercury_emul.cpp -- TEST-ONLY: the lane bodies of Mercury's kernels (nova_amd/csrc/mercury.hpp) on the CPU, one fiber per
// thread (simt.hpp), limb bounds asserted (NMX_DEBUG_BOUNDS).  The internal-form alpha, alpha^seg_rows and eq table come from the test
// (tests/test_mercury_abi.py) in big integers, so the host half of the calls is not trusted here.  The three division passes run with the
// kernels' own thread -> (segment, column) map; of h every lane's canonical partial sum is handed back and the test adds them up.
// NOT emulated: the wave reduction of k_mercury_h (shuffles), its LDS staging of the table, the launches and the host half.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/msm_pipeline.hpp"
#include "../../nova_amd/csrc/mercury.hpp"

using namespace nmx;

template <int FID>
static void run_div(const uint32_t* f, uint32_t n_rows, uint32_t n_cols, uint32_t seg_rows, const uint32_t* alpha, const uint32_t* alpha_seg,
                    uint32_t* q, uint32_t* g, uint32_t* tot) {
  MercuryDivArgs<FID> a;
  a.f = f, a.q = q, a.g = g, a.tot = tot;
  a.alpha = Fp<FID>::from_words(alpha), a.alpha_seg = Fp<FID>::from_words(alpha_seg);
  a.n_rows = n_rows, a.n_cols = n_cols, a.seg_rows = seg_rows, a.segs = (n_rows + seg_rows - 1) / seg_rows;
  const uint32_t cblocks = (n_cols + 255) / 256;
  if (a.segs > 1) {
    simt::launch(cblocks * (a.segs - 1), 256, [&] {
      uint32_t seg, col;
      if (mercury_div_where(simt::bid(), simt::tid(), a.n_cols, 1u, &seg, &col)) mercury_div_total_lane<FID>(a, seg, col);
    });
    simt::launch(cblocks, 256, [&] {
      const uint32_t col = simt::bid() * 256u + simt::tid();
      if (col < a.n_cols) mercury_div_carry_lane<FID>(a, col);
    });
  }
  simt::launch(cblocks * a.segs, 256, [&] {
    uint32_t seg, col;
    if (mercury_div_where(simt::bid(), simt::tid(), a.n_cols, 0u, &seg, &col)) mercury_div_walk_lane<FID>(a, seg, col);
  });
}

template <int FID> static void run_h(const uint32_t* f, uint32_t n_rows, uint32_t n_cols, const uint32_t* eq_internal, uint32_t* lane_sums) {
  simt::launch((n_rows + 3) / 4, 256, [&] {
    const uint32_t lane = simt::tid() & 63u, row = simt::bid() * 4u + (simt::tid() >> 6);
    if (row >= n_rows) return;
    mercury_h_lane<FID>(f, row, n_cols, lane, MercuryEqTable<FID>{eq_internal, n_cols}).to_words(lane_sums + 8 * ((size_t)row * 64 + lane));
  });
}

// q: (n_rows - 1) * n_cols elements, g: n_cols, tot: ceil(n_rows / seg_rows) * n_cols of scratch; alpha, alpha_seg: internal form, 8 words
extern "C" int emul_mercury_div(int fid, const uint32_t* f, uint32_t n_rows, uint32_t n_cols, uint32_t seg_rows, const uint32_t* alpha,
                                const uint32_t* alpha_seg, uint32_t* q, uint32_t* g, uint32_t* tot) {
  if (!n_rows || !n_cols || !seg_rows) return -1;
  switch (fid) {
    case 0: run_div<0>(f, n_rows, n_cols, seg_rows, alpha, alpha_seg, q, g, tot); break;
    case 1: run_div<1>(f, n_rows, n_cols, seg_rows, alpha, alpha_seg, q, g, tot); break;
    case 2: run_div<2>(f, n_rows, n_cols, seg_rows, alpha, alpha_seg, q, g, tot); break;
    case 3: run_div<3>(f, n_rows, n_cols, seg_rows, alpha, alpha_seg, q, g, tot); break;
    default: return -1;
  }
  return 0;
}
// lane_sums: n_rows * 64 elements
extern "C" int emul_mercury_h(int fid, const uint32_t* f, uint32_t n_rows, uint32_t n_cols, const uint32_t* eq_internal, uint32_t* lane_sums) {
  switch (fid) {
    case 0: run_h<0>(f, n_rows, n_cols, eq_internal, lane_sums); break;
    case 1: run_h<1>(f, n_rows, n_cols, eq_internal, lane_sums); break;
    case 2: run_h<2>(f, n_rows, n_cols, eq_internal, lane_sums); break;
    case 3: run_h<3>(f, n_rows, n_cols, eq_internal, lane_sums); break;
    default: return -1;
  }
  return 0;
}
// the prologue's conversion of eq_col (MercuryEqFn), element by element; out: [word][column]
extern "C" int emul_mercury_eq(int fid, const uint32_t* in, uint32_t n, uint32_t mont, uint32_t* out) {
  for (uint32_t i = 0; i < n; i++) switch (fid) {
      case 0: MercuryEqFn<0>{in, out, n, mont}(i); break;
      case 1: MercuryEqFn<1>{in, out, n, mont}(i); break;
      case 2: MercuryEqFn<2>{in, out, n, mont}(i); break;
      case 3: MercuryEqFn<3>{in, out, n, mont}(i); break;
      default: return -1;
    }
  return 0;
}
