// derive_key.hpp -- derived[j] = sum of ck[i] over all i < n with addresses[i] == j, in HBM: nmx_bases_derive_by_address
// (the reference's CommitmentEngineTrait::ck_derive_by_address, src/traits/commitment.rs:177-194; Pedersen src/provider/pedersen.rs:360-381,
// HyperKZG src/provider/hyperkzg.rs:731-749: a serial acc[addresses[i]] += ck[i]).  Included by runtime.hpp; instantiated by curve_impl.hpp
// (the four curve TUs).  New device code uses lane-level and block-level primitives only (LDS, barriers, one atomic OR), so
// tests/host_emul/derive_key_emul.cpp runs the same bodies on the CPU (simt.hpp) with the limb bounds asserted (NMX_DEBUG_BOUNDS).
//
// It is ONE window of a bucket MSM in which the "digit" of point i is addresses[i], stopped before the bucket reduction, the buckets
// normalised to affine and kept as a key.  derive_pipeline() is the generic-sort branch plus the task branch of msm_pipeline() over the same
// functors (msm_kernels.hpp), with an MsmShape of nbuckets = table_size, total = n:
//   DeriveKeysFn     one lane per source point: key = address narrowed to 32 bits, val = i.  The trash key table_size for an address that
//                    is not below table_size (DK_ERR_ADDRESS is raised: the reference's InvalidIndex) and for a source row that is the
//                    identity encoding (it contributes nothing; skipped when the key is known to hold none)
//   sort_pairs       over ilog2(table_size) + 1 key bits; BoundsFn over table_size + 1 buckets
//   PlanFn, ExpandFn buckets longer than lmax are split into equal tasks.  Skew is the normal case here (padding addresses put a large
//                    share of all points on one index): no lane adds more than lmax points, whatever the distribution
//   launch_accum     one lane (or quad) per bucket | task: gathers ck[vals], mixed additions
//   launch_fold      strided folds T = 32768, 4096, 512, 64, mid, 1 of a split bucket's partial sums: at most 7 dependent additions a pass
//   k_derive_affine  blocks of 256 lanes, one lane per table index: the bucket (XYZZ, canonical at rest) through the block's ONE shared
//                    inversion (fb_block_affine, fixed_base.hpp) to the AffineW row of the new key.  An empty index, or one whose points
//                    cancel, writes the all-zero encoding and raises DK_ANY_IDENTITY
// Every index of every array is a key below table_size + 1 or a position below n that the stages themselves produced: an address is
// compared BEFORE it is narrowed and never used as an index when it is out of range.
//
// lmax (the longest run one lane adds).  The generic path's rule is 4 x the mean bucket, at least 32: a lane per bucket while the
// distribution is flat, tasks only for the outliers.  Here the mean can be the whole input (table_size = 1), so the rule is capped by the
// run that still gives every lane of the chip a task, n / 2^14 (four rounds of 2^16 lanes), and by 1024: min(4 mean, n / 2^14) in
// [32, 1024].  Not tuned by measurement; option derive_lmax (2 .. 1024) overrides it, which is how the tests reach the split and fold passes
// with few points.
//
// Bounds: buckets are XYZZ::load of canonical words (every coordinate < p), inside what fb_block_affine documents (x < 5.3, y < 3.5,
// zz, zzz < 1.2); the additions are the MSM's own functors.
#pragma once

#include "msm_pipeline.hpp"  // MsmShape, the functors, ilog2_u32
#include "fixed_base.hpp"    // fb_block_affine, kFbThreads

namespace nmx {

static constexpr uint32_t kDeriveLmaxMin = 2, kDeriveLmaxMax = 1024;
enum : uint32_t { DK_ERR_ADDRESS = 1u, DK_ANY_IDENTITY = FB_ANY_IDENTITY };  // bits of the flag word (fb_block_affine raises the second)

inline uint32_t derive_default_lmax(uint32_t n, uint32_t table_size) {
  const uint64_t mean4 = 4ull * n / table_size, rounds4 = n >> 14;
  const uint64_t l = mean4 < rounds4 ? mean4 : rounds4;
  return l < 32 ? 32u : l > kDeriveLmaxMax ? kDeriveLmaxMax : (uint32_t)l;
}
inline MsmShape derive_shape(uint32_t n, uint32_t table_size, uint32_t force_lmax) {
  MsmShape sh;
  sh.n = n;
  sh.c = 0;  // no digits: the key of point i is its address
  sh.W = 1;
  sh.WB = 1;
  sh.M = table_size;
  sh.nbuckets = table_size;
  sh.lmax = force_lmax ? force_lmax : derive_default_lmax(n, table_size);
  sh.total = n;
  return sh;
}

struct DeriveKeysFn {
  const uint64_t* addr64;  // n words as the caller holds them in HBM, or null
  const uint32_t* addr32;  // n words narrowed (and checked) by the host, when addr64 is null
  const uint32_t* bases;   // n x 16 words, only to test for the identity encoding; null when the key holds none
  uint32_t* keys;
  uint32_t* vals;
  uint32_t* flags;
  uint32_t table_size;
  NMX_HD void operator()(uint32_t i) const {
    uint32_t key = table_size;
    if (addr64) {
      const uint64_t a = addr64[i];
      if (a < (uint64_t)table_size) key = (uint32_t)a;
    } else {
      const uint32_t a = addr32[i];
      if (a < table_size) key = a;
    }
    if (key == table_size) nmx_atomic_or(flags, DK_ERR_ADDRESS);
    if (bases) {
      uint32_t o = 0;
      const uint32_t* b = bases + 16 * (size_t)i;
#pragma unroll
      for (int j = 0; j < 16; j++) o |= b[j];
      if (o == 0) key = table_size;
    }
    keys[i] = key;
    vals[i] = i;
  }
};

struct DeriveAffineArgs {
  const XYZZW* buckets;  // table_size
  AffineW* out;          // table_size rows of the new key
  uint32_t* flags;
  uint32_t table_size;
};
// grid = ceil(table_size / 256) blocks of 256 threads
template <int BF> NMX_KERNEL void NMX_LAUNCH_BOUNDS(256) k_derive_affine(DeriveAffineArgs a) {
  const uint32_t j = NMX_BID * kFbThreads + NMX_TID;
  const bool active = j < a.table_size;
  XYZZ<BF> acc = XYZZ<BF>::identity();
  if (active) acc = XYZZ<BF>::load(a.buckets[j]);
  fb_block_affine<BF>(acc, active, a.out + (active ? j : 0u), a.flags);
}

struct DeriveArgs {
  const uint64_t* addr64;  // backend-addressable; exactly one of addr64 / addr32 when n > 0
  const uint32_t* addr32;
  const void* bases;       // backend-addressable AffineW[>= n]: internal form, canonical
  AffineW* out;            // backend-addressable AffineW[table_size]
  uint32_t n, table_size;
  uint32_t bases_clean;    // 1: the source holds no identity point: the key stage does not read it
  uint32_t force_lmax;     // 0: derive_default_lmax
};

// Fills a.out.  On return *flags_host holds the flag word (DK_ERR_ADDRESS: a.out is then not to be kept).  Returns the shape used.
template <class BE, int FID> MsmShape derive_pipeline(BE& be, const DeriveArgs& a, uint32_t* flags_host) {
  const MsmShape sh = derive_shape(a.n, a.table_size, a.force_lmax);
  if (a.n == 0) {  // every index is empty: no sort, no accumulate
    be.memset0(a.out, (size_t)a.table_size * sizeof(AffineW));
    *flags_host = DK_ANY_IDENTITY;
    be.sync();
    return sh;
  }
  const size_t total = sh.total;
  const uint32_t heavy_cap = (uint32_t)(total / sh.lmax) + 1;
  const uint32_t extra_cap = 2 * heavy_cap;
  const uint32_t big_cap = (uint32_t)(total / ((size_t)64 * sh.lmax)) + 1;
  // one zeroed block: bucket bounds, then the counters of PlanFn ([0] extra tasks, [1] split buckets, [2] the flag word, [3] most tasks in
  // one bucket, [4] big buckets)
  const size_t nzero = 2 * ((size_t)sh.nbuckets + 1) + 8;
  uint32_t* start = be.template alloc<uint32_t>(nzero);
  uint32_t* end = start + sh.nbuckets + 1;
  uint32_t* counters = end + sh.nbuckets + 1;
  uint32_t* flags = counters + 2;
  HeavyRec* heavy = be.template alloc<HeavyRec>(heavy_cap);
  HeavyRec* big = be.template alloc<HeavyRec>(big_cap);
  TaskRec* extra = be.template alloc<TaskRec>(extra_cap);
  XYZZW* buckets = be.template alloc<XYZZW>(sh.nbuckets);
  XYZZW* partials = be.template alloc<XYZZW>(extra_cap);
  uint32_t* keys0 = be.template alloc<uint32_t>(total);
  uint32_t* vals0 = be.template alloc<uint32_t>(total);
  uint32_t* keys1 = be.template alloc<uint32_t>(total);
  uint32_t* vals1 = be.template alloc<uint32_t>(total);
  be.memset0(start, (nzero * sizeof(uint32_t) + 255) & ~(size_t)255);
  {
    DeriveKeysFn f{a.addr64, a.addr32, a.bases_clean ? nullptr : (const uint32_t*)a.bases, keys0, vals0, flags, a.table_size};
    be.launch(f, a.n);
  }
  be.sort_pairs(keys0, keys1, vals0, vals1, total, ilog2_u32(sh.nbuckets) + 1);  // keys in [0, table_size]
  {
    BoundsFn f{keys1, start, end, (uint32_t)total};
    be.launch(f, (uint32_t)((total + BoundsFn::kPerLane - 1) / BoundsFn::kPerLane));
  }
  const uint32_t hb = heavy_cap < sh.nbuckets ? heavy_cap : sh.nbuckets;  // upper bound on split buckets
  {
    PlanFn f{start, end, counters, heavy, big, sh};
    be.launch(f, (sh.nbuckets + PlanFn::kPerLane - 1) / PlanFn::kPerLane);
    ExpandFn e{start, end, counters, heavy, extra, sh, 64, hb < 16384 ? hb : 16384};
    be.launch(e, e.groups * e.lanes);
  }
  be.template launch_accum<FID>((const AffineW*)a.bases, vals1, start, end, counters, extra, buckets, partials, sh, sh.nbuckets + extra_cap,
                                (uint64_t)sh.nbuckets + total / sh.lmax);
  {
    // the passes of msm_pipeline()'s task branch: every pass shrinks a bucket's partial count by at most 8x; a pass no bucket can need is
    // not launched, one that no bucket does need exits at once
    const uint32_t typical = (uint32_t)(total / ((size_t)sh.nbuckets * sh.lmax));
    const uint32_t mid = typical > 32 ? 8u : 4u;
    const uint32_t Ts[6] = {32768, 4096, 512, 64, mid, 1};
    for (int p = 0; p < 6; p++) {
      const uint32_t T = Ts[p];
      const uint32_t cap = p == 0 ? 0xffffffffu : Ts[p - 1];
      if ((uint64_t)T * sh.lmax > total && T != 1) continue;  // no bucket can have more than T tasks
      const uint32_t bound = T >= 64 ? (big_cap < hb ? big_cap : hb) : hb;
      uint32_t groups = T >= 64 ? (1u << 18) / T : bound;
      if (groups > bound) groups = bound;
      if (groups < 1) groups = 1;
      be.template launch_fold<FID>(counters, T >= 64 ? big : heavy, partials, buckets, T, cap, groups);
    }
  }
  be.launch_kernel(&k_derive_affine<FID>, (a.table_size + kFbThreads - 1) / kFbThreads, kFbThreads,
                   DeriveAffineArgs{buckets, a.out, flags, a.table_size});
  be.d2h(flags_host, flags, sizeof(uint32_t));
  be.sync();
  return sh;
}

}  // namespace nmx
