// tests/host_emul/derive_key_emul.cpp -- TEST-ONLY: the whole chain of nova_amd/csrc/derive_key.hpp (derive_pipeline) on the CPU with a small
// host backend of its own: lane functors as plain loops, std::stable_sort for the pair sort, k_derive_affine on fibers (simt.hpp: LDS product
// tree, barriers, lane 0's inversion), limb bounds asserted (NMX_DEBUG_BOUNDS).  The backend checks what every later index depends on: the
// sorted keys are at most table_size and the sorted values below n; every allocation carries a guard area behind it that must come back
// untouched.  Points go in and come back as the kernels hold them: x || y in the internal form (x * 2^261 mod p), all zero for the identity;
// the test (tests/test_derive_key_abi.py) converts in big integers.
// NOT emulated: the launches, the rocPRIM sort, the quad forms of accumulate and fold, build_key, the key's window tables, the concurrency of
// the atomics.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/msm_pipeline.hpp"
#include "../../nova_amd/csrc/derive_key.hpp"

using namespace nmx;

static constexpr size_t kGuard = 256;
struct DeriveEmulBackend {
  struct Block {
    char* p;
    size_t bytes;
  };
  std::vector<Block> blocks;
  uint32_t n = 0, table_size = 0;
  int bad = 0;  // 1: a sorted key above table_size, 2: a sorted value not below n
  const uint32_t* counters = nullptr;
  uint32_t launches = 0, block_launches = 0, sorts = 0, fold_mask = 0;
  ~DeriveEmulBackend() {
    for (const Block& b : blocks) free(b.p);
  }
  template <class T> T* alloc(size_t count) {
    const size_t bytes = ((count ? count : 1) * sizeof(T) + 255) & ~(size_t)255;  // padded like the device arena
    char* p = (char*)calloc(bytes + kGuard, 1);
    memset(p + bytes, 0xa5, kGuard);
    blocks.push_back({p, bytes});
    return (T*)p;
  }
  bool guards_intact() const {
    for (const Block& b : blocks)
      for (size_t i = 0; i < kGuard; i++)
        if ((unsigned char)b.p[b.bytes + i] != 0xa5) return false;
    return true;
  }
  void memset0(void* p, size_t bytes) { memset(p, 0, bytes); }
  template <class F> void launch(const F& f, uint32_t lanes) {
    launches++;
    for (uint32_t t = 0; t < lanes; t++) f(t);
  }
  template <class A> void launch_kernel(void (*k)(A), uint32_t grid, uint32_t block, const A& a) {
    if (grid == 0) return;
    block_launches++;
    simt::launch(grid, block, [&] { k(a); });
  }
  template <int FID>
  void launch_accum(const AffineW* bases, const uint32_t* vals, const uint32_t* start, const uint32_t* end, const uint32_t* ctr, const TaskRec* extra,
                    XYZZW* buckets, XYZZW* partials, const MsmShape& sh, uint32_t slots, uint64_t) {
    counters = ctr;
    AccumFn<FID> f{bases, vals, start, end, ctr, extra, buckets, partials, sh};
    launch(f, slots);
  }
  template <int FID>
  void launch_fold(const uint32_t* ctr, const HeavyRec* heavy, XYZZW* partials, XYZZW* buckets, uint32_t T, uint32_t cap, uint32_t groups) {
    fold_mask |= T >= 32768 ? 32u : T >= 4096 ? 16u : T >= 512 ? 8u : T >= 64 ? 4u : T > 1 ? 2u : 1u;
    FoldFn<FID> f{ctr, heavy, partials, buckets, T, cap, groups};
    launch(f, groups * T);
  }
  void sort_pairs(uint32_t* k_in, uint32_t* k_out, uint32_t* v_in, uint32_t* v_out, size_t total, uint32_t bits) {
    sorts++;
    std::vector<uint32_t> idx(total);
    std::iota(idx.begin(), idx.end(), 0u);
    const uint32_t mask = bits >= 32 ? 0xffffffffu : ((1u << bits) - 1u);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return (k_in[a] & mask) < (k_in[b] & mask); });
    for (size_t i = 0; i < total; i++) {
      k_out[i] = k_in[idx[i]];
      v_out[i] = v_in[idx[i]];
      if (k_out[i] > table_size || (k_out[i] & mask) != k_out[i]) bad = 1;  // (a key wider than `bits` would be sorted wrongly by a radix sort)
      if (v_out[i] >= n) bad = 2;
    }
  }
  void d2h(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); }
  void sync() {}
};

template <int CID>
static int run(const uint32_t* src16, uint32_t n, const uint64_t* addr64, const uint32_t* addr32, uint32_t table_size, uint32_t clean, uint32_t lmax,
               uint32_t* out16, uint32_t* flags, uint32_t* stats) {
  constexpr int BF = CurveT<CID>::BF;
  DeriveEmulBackend be;
  be.n = n, be.table_size = table_size;
  DeriveArgs a{};
  a.addr64 = addr64, a.addr32 = addr32, a.bases = src16, a.out = (AffineW*)out16;
  a.n = n, a.table_size = table_size, a.bases_clean = clean, a.force_lmax = lmax;
  *flags = 0;
  const MsmShape sh = derive_pipeline<DeriveEmulBackend, BF>(be, a, flags);
  stats[0] = sh.lmax;
  stats[1] = be.counters ? be.counters[0] : 0;  // extra tasks
  stats[2] = be.counters ? be.counters[1] : 0;  // split buckets
  stats[3] = be.counters ? be.counters[3] : 0;  // most tasks in one big bucket
  stats[4] = be.counters ? be.counters[4] : 0;  // big buckets
  stats[5] = be.fold_mask;                      // bit 0: T = 1, 1: the middle pass, 2: T = 64, 3: 512, 4: 4096, 5: 32768
  stats[6] = be.launches + be.block_launches + be.sorts;
  stats[7] = be.block_launches;
  if (be.bad) return be.bad;
  return be.guards_intact() ? 0 : 3;
}

// src16: >= n rows of 16 words (internal form, canonical; all zero = identity); exactly one of addr64 / addr32 when n > 0; out16: table_size
// rows; stats: 8 words.  Returns 0, or 1 / 2 / 3 (see DeriveEmulBackend::bad, 3: a guard area was written), -1 for bad arguments
extern "C" int emul_derive(int cid, const uint32_t* src16, uint32_t n, const uint64_t* addr64, const uint32_t* addr32, uint32_t table_size,
                           uint32_t clean, uint32_t lmax, uint32_t* out16, uint32_t* flags, uint32_t* stats) {
  if (!table_size || (n && !addr64 == !addr32) || (lmax && (lmax < kDeriveLmaxMin || lmax > kDeriveLmaxMax))) return -1;
  switch (cid) {
    case 0: return run<0>(src16, n, addr64, addr32, table_size, clean, lmax, out16, flags, stats);
    case 1: return run<1>(src16, n, addr64, addr32, table_size, clean, lmax, out16, flags, stats);
    case 2: return run<2>(src16, n, addr64, addr32, table_size, clean, lmax, out16, flags, stats);
    case 3: return run<3>(src16, n, addr64, addr32, table_size, clean, lmax, out16, flags, stats);
  }
  return -1;
}

extern "C" void emul_derive_geometry(uint32_t* out4) {
  out4[0] = DK_ERR_ADDRESS, out4[1] = DK_ANY_IDENTITY, out4[2] = kDeriveLmaxMin, out4[3] = kDeriveLmaxMax;
}
extern "C" uint32_t emul_derive_default_lmax(uint32_t n, uint32_t table_size) { return derive_default_lmax(n, table_size); }
