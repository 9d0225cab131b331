// tests/host_emul/hyperkzg_emul.cpp -- TEST-ONLY: the lane bodies of the batched multi-point quotient pass (nova_amd/csrc/hyperkzg.hpp) on the
// CPU, one fiber per thread (simt.hpp), limb bounds asserted (NMX_DEBUG_BOUNDS).  The launches are the library's own (lq_run: the heads
// pass, the levels above it, the walk) with its thread -> chunk map; the powers of q and of the points come from the test
// (tests/test_hyperkzg_abi.py) in big integers, so the host half of the call is not trusted here.  Every workspace vector and every
// output carries a guard element behind it, checked after the run.
// NOT emulated: the launches themselves, staging, the arena, the descriptor table in device memory (k > 32 takes `ext`, here host memory).
#include <stdint.h>
#include <string.h>

#include <memory>
#include <vector>

#include "simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/msm_pipeline.hpp"
#include "../../nova_amd/csrc/hyperkzg.hpp"

using namespace nmx;

static constexpr uint32_t kGuard = 0xA5A5A5A5u;

template <int FID>
static int run(uint32_t chunk_opt, int scratch, const uint32_t* const* polys, const uint32_t* lens, uint32_t k, const uint32_t* w, const uint32_t* upow,
               uint32_t m, uint32_t levels, uint32_t* const* outs) {
  uint32_t n_out = 0;
  for (uint32_t i = 0; i < k; i++) n_out = lens[i] > n_out ? lens[i] : n_out;
  if (!n_out) return 0;
  const LqPlan pl = lq_plan(n_out, chunk_opt);
  if (pl.levels != levels) return -2;  // the test's restatement of the plan disagrees
  Fp<FID> up[kLqMaxPts][kLqMaxLevels];
  for (uint32_t j = 0; j < m; j++)
    for (uint32_t l = 0; l < levels; l++) up[j][l] = Fp<FID>::from_words(upow + 8 * ((size_t)j * levels + l));
  auto a = std::make_unique<LqArgs<FID>>();
  memset(a.get(), 0, sizeof(*a));
  std::vector<LqPoly> ext(k);
  for (uint32_t i = 0; i < k; i++) {
    ext[i].f = polys[i], ext[i].len = lens[i], ext[i].pad = 0;
    memcpy(ext[i].w, w + 8 * (size_t)i, 32);
    if (k <= kLqInline) a->tab[i] = ext[i];
  }
  a->ext = k > kLqInline ? ext.data() : nullptr;
  a->k = k, a->m = m;
  std::vector<std::vector<uint32_t>> bufs;  // every vector with one guard element behind it
  auto take = [&](size_t elems) {
    bufs.emplace_back(8 * (elems + 1), 0u);
    for (int q = 0; q < 8; q++) bufs.back()[8 * elems + q] = kGuard;
    return bufs.back().data();
  };
  a->scratch = scratch ? take(n_out) : nullptr;
  for (uint32_t j = 0; j < m; j++) a->out[j] = outs[j];
  lq_run<FID>(pl, *a, up, take, [&](const auto& fn, uint32_t lanes) {
    simt::launch((lanes + 255) / 256, 256, [&] {
      const uint32_t tid = simt::bid() * 256u + simt::tid();
      if (tid < lanes) fn(tid);
    });
  });
  for (const auto& b : bufs)
    for (int q = 0; q < 8; q++)
      if (b[b.size() - 8 + q] != kGuard) return -3;  // a store past the end of a workspace vector
  return 0;
}

// polys: k pointers, lens: k; w: k x 8 words (q^i, internal form); upow: m x levels x 8 words (u_j^(elements of level 0 per element of
// level l), internal form); outs: m vectors of max(lens) elements (the caller appends and checks its own guard)
extern "C" int emul_lincomb_quotients(int fid, uint32_t chunk_opt, int scratch, const uint32_t* const* polys, const uint32_t* lens, uint32_t k,
                                      const uint32_t* w, const uint32_t* upow, uint32_t m, uint32_t levels, uint32_t* const* outs) {
  if (!k || !m || m > kLqMaxPts || levels > kLqMaxLevels) return -1;
  switch (fid) {
    case 0: return run<0>(chunk_opt, scratch, polys, lens, k, w, upow, m, levels, outs);
    case 1: return run<1>(chunk_opt, scratch, polys, lens, k, w, upow, m, levels, outs);
    case 2: return run<2>(chunk_opt, scratch, polys, lens, k, w, upow, m, levels, outs);
    case 3: return run<3>(chunk_opt, scratch, polys, lens, k, w, upow, m, levels, outs);
  }
  return -1;
}
