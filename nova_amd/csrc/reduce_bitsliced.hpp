// reduce_bitsliced.hpp -- the bucket reduction sum_k (k + 1) B_k as bit-sliced sums (host + device).
//
// Write the bucket index in binary:
//     sum_k k B_k  =  sum_l 2^l O_l ,     O_l = sum of the B_k whose index has bit l set.
// Build the plain pair-sum tree N^0_k = B_k, N^(l+1)_j = N^l_2j + N^l_2j+1: O_l is the sum of the ODD nodes of level l, and the
// root is sum_k B_k, the "+ 1" of the weight.  Step s (s = 0 .. L - 1, L = log2 M) halves every array in flight with ONE
// independent addition per output:
//     N^(s+1)_j = N^s_2j + N^s_2j+1 ,     O_l,j <- O_l,2j + O_l,2j+1  for l < s ,     O_s := the odd elements of N^s (no addition).
// After step s there are s + 2 arrays of M / 2^(s+1) elements; after the last one L + 1 single points, combined pairwise
// (weights 2, 4, 16, 256: P_i = O_2i + 2 O_2i+1, then P_2i + 4 P_2i+1, ...), ceil(log2 L) additions and L - 1 doublings deep.
// About 2 M additions and no doublings before the end, one dependent addition per level -- against the pair tree's
// (ReducePairFn, msm_kernels.hpp) 3 M additions + M doublings and two dependent additions per level.
//
// Arrays are FLAT over the WB bucket sets of a fused batch (set w at [w n, (w + 1) n), n a power of two): pairing 2j, 2j + 1 never
// crosses a set.  A launch's arrays sit one behind the other in one allocation, [N, O_0, O_1, ...]; the newest O of a one-step
// launch is a strided VIEW of the previous launch's N (odd elements), not a copy.
//
// This header holds what the host-side test (tests/cpp/reduce_bitsliced_test.cpp) shares with the device: the launch plan, the
// one-step functor and the body of the fused kernel, written over a policy P that says what a "thread group" is (four lanes holding
// one coordinate each on the device, curve_quad.hpp; one fiber holding the whole point on the host).
#pragma once
#include "curve.hpp"

namespace nmx {

static constexpr uint32_t kBsQuads = 128;                 // thread groups per block of the fused kernel (512 threads)
static constexpr uint32_t kBsBuf0 = 256, kBsBuf1 = 192;   // LDS points of the two level buffers (144 B each: 64 512 B)
static constexpr uint32_t kBsMaxLaunches = 40;

struct BsLaunch {
  uint32_t wide;    // 1: one step, one addition per work item of a plain launch (BsStepFn / BsStepQuadFn)
  uint32_t step;    // first step of this launch
  uint32_t levels;  // steps in this launch
  uint32_t S;       // fused: flat inputs of every array per block
  uint32_t n_tot;   // flat elements of every array on entry = WB * (M >> step)
  uint32_t n_cont;  // arrays that sit in the input allocation
  uint32_t view;    // 1: one more array, the odd elements of the PREVIOUS launch's first input array
  uint32_t last;    // the fused launch that ends the tree and combines: one block per bucket set (S = the set's elements)
};

// The launches of one reduction.  A step with more than `wide_above` additions is throughput-bound and gets a launch of its
// own; the others run fused, a block owning S consecutive elements of every live array with at most `cap` additions in its
// first level, as many levels as S allows.  The last launch is one block per bucket set.  false: the shape does not fit the fused
// kernel's LDS or its index range (the caller keeps the pair tree).
inline bool bs_plan(uint32_t M, uint32_t WB, uint32_t cap, uint32_t wide_above, BsLaunch* out, uint32_t* count) {
  uint32_t L = 0;
  while ((1u << L) < M) L++;
  if (L == 0 || (1u << L) != M || L > 31 || WB == 0) return false;
  uint32_t s = 0, n_cont = 1, view = 0, n = 0;
  for (;;) {
    const uint64_t n_tot64 = (uint64_t)WB * (M >> s);
    if (n_tot64 >> 31) return false;
    const uint32_t n_tot = (uint32_t)n_tot64, A = n_cont + view, rem = L - s;
    const uint64_t items = (uint64_t)A * (n_tot / 2);
    if (n == kBsMaxLaunches) return false;
    BsLaunch& l = out[n++];
    l = BsLaunch{0, s, 1, 0, n_tot, n_cont, view, 0};
    if (items > wide_above && rem > 1) {
      if (items >> 30) return false;
      l.wide = 1;
      n_cont = A, view = 1, s += 1;
      continue;
    }
    const uint32_t n_set = M >> s;
    if ((uint64_t)A * (n_set / 2) <= cap || rem == 1) {  // the rest of every set in one block of its own
      l.S = n_set, l.levels = rem, l.last = 1;
      if ((uint64_t)(A + 1) * (n_set / 2) > kBsBuf0) return false;
      if (rem >= 2 && (uint64_t)(A + 2) * (n_set / 4) > kBsBuf1) return false;
      *count = n;
      return true;
    }
    uint32_t S = 2, lg = 1;
    while (2 * S <= (M >> s) && (uint64_t)A * S <= cap) S *= 2, lg++;  // A * (2 S / 2) <= cap
    l.S = S, l.levels = lg < rem - 1 ? lg : rem - 1;
    if ((uint64_t)(A + 1) * (S / 2) > kBsBuf0) return false;
    if (l.levels >= 2 && (uint64_t)(A + 2) * (S / 4) > kBsBuf1) return false;
    s += l.levels, n_cont = s + 1, view = 0;
  }
}
// arrays a launch writes, and elements of each
NMX_HD uint32_t bs_out_arrays(const BsLaunch& l) { return l.wide ? l.n_cont + l.view : l.n_cont + l.view + l.levels; }
NMX_HD uint32_t bs_out_elems(const BsLaunch& l) { return l.n_tot >> l.levels; }

// One step in a launch of its own: work item = (array, output).  `in`: n_cont arrays of 2 * half elements; `view`: the first
// input array of the step before (its odd elements are the newest O) or null; out: the n_cont (+ 1) halved arrays.
struct BsStepArgs {
  const XYZZW* in;
  const XYZZW* view;
  XYZZW* out;
  uint32_t half, n_cont, items;
};
NMX_HD const XYZZW* bs_step_src(const BsStepArgs& a, uint32_t item, uint32_t* gap) {
  const uint32_t arr = item / a.half, j = item - arr * a.half;
  if (arr < a.n_cont) {
    *gap = 1;
    return a.in + ((size_t)arr * 2 * a.half + 2 * (size_t)j);
  }
  *gap = 2;  // element i of the view is element 2 i + 1 of the array it looks at
  return a.view + (4 * (size_t)j + 1);
}
template <int FID> struct BsStepFn {
  BsStepArgs a;
  NMX_HD void operator()(uint32_t item) const {
    if (item >= a.items) return;
    uint32_t gap;
    const XYZZW* src = bs_step_src(a, item, &gap);
    XYZZ<FID> p = XYZZ<FID>::load(src[0]);
    p.template add<kLatTail>(XYZZ<FID>::load(src[gap]));
    p.store(a.out[item]);
  }
};

// The fused launches.  Level k of a launch (k = 1 .. levels) adds pairs of the A = n_cont + view + k - 1 arrays alive there and
// keeps the odd elements of N as the array born at that level; inputs come from memory (k = 1) or the other LDS buffer, outputs go
// to LDS or (the last level of a launch that does not end the tree) to memory, canonical.  In the launch that ends the tree a block
// owns one whole set, leaves its L + 1 points in LDS and combines them.
struct BsTreeArgs {
  const XYZZW* in;
  const XYZZW* view;  // or null
  XYZZW* out;         // last: the WB sums (block w writes set w's), the error word behind them
  uint32_t n_tot, S, levels, n_cont, last, WB;
  const uint32_t* err_src;  // last: the pipeline's error word
  // last, 1: no combine.  Block w leaves its L + 1 points, canonical, at out[w (L + 1) ..]: the root, then O_0 .. O_(L-1); the
  // error word sits behind all WB (L + 1) of them.  The host finishes (host_point4.hpp combine_slices).
  uint32_t slices = 0;
};
// P: V (what a group holds of a point), groups() / group() / block(), load / store (canonical, memory), lds_load / lds_store
// (raw limbs, point index into a buffer of 36-word points), add / dbl / ident, sync() (every thread of the block), lead() (one
// thread of the block), lds() (kBsBuf0 + kBsBuf1 points).
template <class P> NMX_HD void bs_tree_body(P& p, const BsTreeArgs& a) {
  using V = typename P::V;
  const uint32_t qd = p.group(), NQ = p.groups();
  const uint32_t base = p.block() * a.S;
  const uint32_t A_in = a.n_cont + (a.view ? 1u : 0u);
  uint32_t* const buf[2] = {p.lds(), p.lds() + kBsBuf0 * 36u};
  const uint32_t recs = a.slices ? A_in + a.levels : 1u;  // records a set leaves in the last launch: L + 1 slices, or its sum
  if (a.last && a.err_src && p.block() == 0 && p.lead()) *(uint32_t*)(a.out + (size_t)a.WB * recs) = *a.err_src;
  const uint32_t n_out = a.n_tot >> a.levels, base_out = base >> a.levels;
  for (uint32_t k = 1; k <= a.levels; k++) {
    const uint32_t A = A_in + k - 1u, cnt = a.S >> k;
    const bool to_g = k == a.levels && !a.last;
    uint32_t* const rb = buf[k & 1u];
    uint32_t* const wb = buf[(k - 1u) & 1u];
    for (uint32_t item = qd; item < A * cnt; item += NQ) {
      const uint32_t arr = item / cnt, j = item - arr * cnt;
      V x0, x1;
      if (k == 1) {
        if (arr < a.n_cont) {
          const size_t i0 = (size_t)arr * a.n_tot + base + 2 * j;
          x0 = p.load(a.in, i0), x1 = p.load(a.in, i0 + 1);
        } else {
          const size_t i0 = 2 * ((size_t)base + 2 * j) + 1;
          x0 = p.load(a.view, i0), x1 = p.load(a.view, i0 + 2);
        }
      } else {
        x0 = p.lds_load(rb, arr * 2u * cnt + 2u * j), x1 = p.lds_load(rb, arr * 2u * cnt + 2u * j + 1u);
      }
      const V c = p.add(x0, x1);
      if (to_g) {
        p.store(a.out, (size_t)arr * n_out + base_out + j, c);
        if (arr == 0) p.store(a.out, (size_t)A * n_out + base_out + j, x1);
      } else {
        p.lds_store(wb, arr * cnt + j, c);
        if (arr == 0) p.lds_store(wb, A * cnt + j, x1);
      }
    }
    p.sync();
  }
  if (!a.last) return;
  // this block's set: array 0 = the root, array i + 1 = O_i, one element each.  Group i < L takes O_i; pairwise with weights 2, 4,
  // 16, 256: the group of the higher half doubles 2^t times and parks, the group of the lower half adds.
  const uint32_t* const fin = buf[(a.levels - 1u) & 1u];
  uint32_t* const scr = buf[a.levels & 1u];
  const uint32_t L = A_in + a.levels - 1u;  // <= 31
  if (a.slices) {
    if (qd <= L) p.store(a.out, (size_t)p.block() * (L + 1u) + qd, p.lds_load(fin, qd));
    return;
  }
  uint32_t T = 0;
  while ((1u << T) < L) T++;
  // Groups L <= i < 2^T hold ident(): add() and dbl() must treat it as the group identity (the device's is the all-zero coordinate
  // in every lane, which quad_add / quad_dbl test through zz).  No barrier follows the read of a level: level t reads scr at
  // indices = stride mod 2 stride, level t + 1 writes at indices = 2 stride mod 4 stride, i.e. = 0 mod 2 stride -- disjoint sets.
  const uint32_t i = qd;
  V val = p.ident();
  if (i < L) val = p.lds_load(fin, i + 1u);
  if (i == 0) val = p.add(val, p.lds_load(fin, 0));
  for (uint32_t t = 0; t < T; t++) {
    const uint32_t stride = 1u << t, m = i & (2u * stride - 1u);
    if (i < 32u && m == stride) {
      for (uint32_t d = 0; d < stride; d++) val = p.dbl(val);
      p.lds_store(scr, i, val);
    }
    p.sync();
    if (i < 32u && m == 0) val = p.add(val, p.lds_load(scr, i + stride));
  }
  if (i == 0) p.store(a.out, p.block(), val);
}

}  // namespace nmx
