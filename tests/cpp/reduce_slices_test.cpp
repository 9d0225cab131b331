// tests/cpp/reduce_slices_test.cpp -- TEST-ONLY: the bit-sliced bucket reduction ending in SLICES (BsTreeArgs::slices = 1) and the
// host's combine_slices (nova_amd/csrc/host_point4.hpp) behind it, on the host.
//
// As tests/cpp/reduce_bitsliced_test.cpp: the device's launch plan (bs_plan), one-step functor (BsStepFn) and fused body
// (bs_tree_body) run with whole points on fibers of tests/host_emul/simt.hpp -- a policy of its own, LDS bounds checked.  The last
// launch leaves WB x (L + 1) canonical records and the error word behind them; combine_slices turns every set's records into its sum,
// as DeviceBackend::sync() does with the records it copied.  g++ only, built as a shared library by tests/test_reduce_slices.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../host_emul/simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/host_point4.hpp"
#include "../../nova_amd/csrc/reduce_bitsliced.hpp"

using namespace nmx;

static uint32_t g_lds[(kBsBuf0 + kBsBuf1) * 36];

template <int FID> struct SlicePolicy {
  using V = XYZZ<FID>;
  XYZZW* out_lo;  // the last launch's allocation: stores outside it abort
  XYZZW* out_hi;
  uint32_t groups() const { return kBsQuads; }
  uint32_t group() const { return simt::tid(); }
  uint32_t block() const { return simt::bid(); }
  bool lead() const { return simt::tid() == 0; }
  uint32_t* lds() const { return g_lds; }
  static void bounds(const uint32_t* b, uint32_t i) {
    const size_t off = (size_t)(b - g_lds) / 36;
    const size_t cap = off == 0 ? kBsBuf0 : kBsBuf1;
    if ((off != 0 && off != kBsBuf0) || i >= cap) {  // (a fiber cannot throw across its context switch)
      fprintf(stderr, "bs_slices: LDS point %u outside its buffer\n", i);
      abort();
    }
  }
  V load(const XYZZW* p, size_t i) const { return V::load(p[i]); }
  void store(XYZZW* p, size_t i, const V& c) const {
    if (p + i < out_lo || p + i >= out_hi) {
      fprintf(stderr, "bs_slices: record %zu outside the launch's output\n", i);
      abort();
    }
    c.store(p[i]);
  }
  V lds_load(const uint32_t* b, uint32_t i) const {
    bounds(b, i);
    XYZZL m;
    memcpy(m.l, b + 36 * (size_t)i, sizeof m.l);
    return V::load_raw(m);
  }
  void lds_store(uint32_t* b, uint32_t i, const V& c) const {
    bounds(b, i);
    XYZZL m;
    c.store_raw(m);
    memcpy(b + 36 * (size_t)i, m.l, sizeof m.l);
  }
  V add(V x, const V& y) const {
    x.add(y);
    return x;
  }
  V dbl(V x) const {
    x.dbl_in_place();
    return x;
  }
  V ident() const { return V::identity(); }
  void sync() const { simt::syncthreads(); }
};

template <int CID>
static int run(const uint8_t* xy64, uint32_t M, uint32_t WB, uint32_t cap, uint32_t wide_above, uint8_t* out, uint8_t* inf) {
  constexpr int BF = CurveT<CID>::BF;
  const size_t n = (size_t)WB * M;
  std::vector<XYZZW> buckets(n);
  for (size_t i = 0; i < n; i++) {
    Affine<BF> a;
    a.x = fp_from_bytes<BF>(xy64 + 64 * i);
    a.y = fp_from_bytes<BF>(xy64 + 64 * i + 32);
    if (!a.is_identity()) {
      a.x = a.x.to_internal().canon();
      a.y = a.y.to_internal().canon();
    }
    XYZZ<BF>::from_affine(a).store(buckets[i]);
  }
  BsLaunch plan[kBsMaxLaunches];
  uint32_t nl = 0, L = 0;
  while ((1u << L) < M) L++;
  if (!bs_plan(M, WB, cap, wide_above, plan, &nl)) return -1;
  std::vector<std::vector<XYZZW>> keep;  // every launch's output stays alive: views look one launch back
  const XYZZW* in = buckets.data();
  const XYZZW* prev_in = nullptr;
  const uint32_t err_word = 0x5eed0002u;
  const size_t recs = (size_t)WB * (L + 1);
  for (uint32_t i = 0; i < nl; i++) {
    const BsLaunch& l = plan[i];
    const XYZZW* view = l.view ? prev_in : nullptr;
    // the last launch: the records, the record whose first word is the error word, and one of guard words behind it
    keep.emplace_back(l.last ? recs + 2 : (size_t)bs_out_arrays(l) * bs_out_elems(l));
    XYZZW* o = keep.back().data();
    if (l.last) memset(o, 0xa5, sizeof(XYZZW) * (recs + 2));
    if (l.wide) {
      const uint32_t half = l.n_tot / 2, items = (l.n_cont + l.view) * half;
      const BsStepFn<BF> f{BsStepArgs{in, view, o, half, l.n_cont, items}};
      for (uint32_t t = 0; t < ((items + 255u) & ~255u); t++) f(t);  // whole blocks, as the device launches them
    } else {
      BsTreeArgs a{in, view, o, l.n_tot, l.S, l.levels, l.n_cont, l.last, WB, l.last ? &err_word : nullptr};
      a.slices = l.last;
      if (l.n_tot % l.S) return -2;
      simt::launch(l.n_tot / l.S, kBsQuads, [&] {
        SlicePolicy<BF> p{o, o + (l.last ? recs : (size_t)bs_out_arrays(l) * bs_out_elems(l))};
        bs_tree_body(p, a);
      });
    }
    prev_in = in, in = o;
  }
  // the error word lands behind the last slice and nothing is written past it
  const uint8_t* tail = (const uint8_t*)(in + recs);
  uint32_t e;
  memcpy(&e, tail, sizeof e);
  if (e != err_word) return -3;
  for (size_t i = sizeof e; i < 2 * sizeof(XYZZW); i++)
    if (tail[i] != 0xa5) return -4;
  for (size_t i = 0; i < recs; i++)  // every record was written, canonical
    for (int c = 0; c < 4; c++) {
      uint64_t t[4];
      memcpy(t, in[i].w + 8 * c, 32);
      if (HostFp4<BF>::geq(t, HostFp4<BF>::C().p)) return -5;
    }
  for (uint32_t w = 0; w < WB; w++) {
    XYZZW sum;
    combine_slices<BF>(in + (size_t)w * (L + 1), L, &sum);
    xyzz_to_xy64<BF>(XYZZ<BF>::load(sum), out + 64 * w, inf + w);
  }
  return (int)nl;
}

// buckets: WB x M affine points (x || y canonical little-endian, 64 zero bytes = the identity).  Returns the number of launches
// (< 0: the plan does not fit / an internal check failed) and the WB sums in out / inf.
extern "C" int bs_reduce_slices(int cid, const uint8_t* xy64, uint32_t M, uint32_t WB, uint32_t cap, uint32_t wide_above,
                                uint8_t* out, uint8_t* inf) {
  switch (cid) {
    case 0: return run<0>(xy64, M, WB, cap, wide_above, out, inf);
    case 1: return run<1>(xy64, M, WB, cap, wide_above, out, inf);
    case 2: return run<2>(xy64, M, WB, cap, wide_above, out, inf);
    case 3: return run<3>(xy64, M, WB, cap, wide_above, out, inf);
  }
  return -6;
}
