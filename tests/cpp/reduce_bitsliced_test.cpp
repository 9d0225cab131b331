// tests/cpp/reduce_bitsliced_test.cpp -- TEST-ONLY: the bit-sliced bucket reduction (nova_amd/csrc/reduce_bitsliced.hpp) on the host.
//
// Runs the SAME launch plan (bs_plan), the same one-step functor (BsStepFn) and the same body of the fused kernel (bs_tree_body)
// as the device, with XYZZ::add / dbl_in_place on whole points: a "thread group" is one fiber of tests/host_emul/simt.hpp holding
// the point (the device's is four lanes holding a coordinate each), LDS is a static array, barriers are real.  It checks the
// identity sum_k (k + 1) B_k = root + sum_l 2^l O_l, the plan, the indexing and the barrier placement; tests compare it with the
// oracle.  g++ only, built as a shared library by tests/test_reduce_bitsliced.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../host_emul/simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/reduce_bitsliced.hpp"

using namespace nmx;

static uint32_t g_lds[(kBsBuf0 + kBsBuf1) * 36];

template <int FID> struct HostPolicy {
  using V = XYZZ<FID>;
  uint32_t groups() const { return kBsQuads; }
  uint32_t group() const { return simt::tid(); }
  uint32_t block() const { return simt::bid(); }
  bool lead() const { return simt::tid() == 0; }
  uint32_t* lds() const { return g_lds; }
  static void bounds(const uint32_t* b, uint32_t i) {  // a point outside the buffer it was addressed in
    const size_t off = (size_t)(b - g_lds) / 36;
    const size_t cap = off == 0 ? kBsBuf0 : kBsBuf1;
    if ((off != 0 && off != kBsBuf0) || i >= cap) {  // (a fiber cannot throw across its context switch)
      fprintf(stderr, "bs_reduce: LDS point %u outside its buffer\n", i);
      abort();
    }
  }
  V load(const XYZZW* p, size_t i) const { return V::load(p[i]); }
  void store(XYZZW* p, size_t i, const V& c) const { c.store(p[i]); }
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
static int run(const uint8_t* xy64, uint32_t M, uint32_t WB, uint32_t cap, uint32_t wide_above, uint8_t* out, uint8_t* inf,
               uint32_t* desc /* kBsMaxLaunches x 3: wide, levels, blocks */) {
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
  uint32_t nl = 0;
  if (!bs_plan(M, WB, cap, wide_above, plan, &nl)) return -1;
  std::vector<std::vector<XYZZW>> keep;  // every launch's output stays alive: views look one launch back
  const XYZZW* in = buckets.data();
  const XYZZW* prev_in = nullptr;
  const uint32_t err_word = 0x5eed0001u;
  for (uint32_t i = 0; i < nl; i++) {
    const BsLaunch& l = plan[i];
    const XYZZW* view = l.view ? prev_in : nullptr;
    keep.emplace_back(l.last ? (size_t)WB + 1 : (size_t)bs_out_arrays(l) * bs_out_elems(l));
    XYZZW* o = keep.back().data();
    desc[3 * i] = l.wide, desc[3 * i + 1] = l.levels, desc[3 * i + 2] = l.wide ? 0 : l.n_tot / l.S;
    if (l.wide) {
      const uint32_t half = l.n_tot / 2, items = (l.n_cont + l.view) * half;
      const BsStepFn<BF> f{BsStepArgs{in, view, o, half, l.n_cont, items}};
      for (uint32_t t = 0; t < ((items + 255u) & ~255u); t++) f(t);  // whole blocks, as the device launches them
    } else {
      const BsTreeArgs a{in, view, o, l.n_tot, l.S, l.levels, l.n_cont, l.last, WB, l.last ? &err_word : nullptr};
      if (l.n_tot % l.S) return -2;
      simt::launch(l.n_tot / l.S, kBsQuads, [&] {
        HostPolicy<BF> p;
        bs_tree_body(p, a);
      });
    }
    prev_in = in, in = o;
  }
  uint32_t e;
  memcpy(&e, in + WB, sizeof e);
  if (e != err_word) return -3;  // the error word rides behind the sums
  for (uint32_t w = 0; w < WB; w++) xyzz_to_xy64<BF>(XYZZ<BF>::load(in[w]), out + 64 * w, inf + w);
  return (int)nl;
}

// buckets: WB x M affine points (x || y canonical little-endian, 64 zero bytes = the identity).  Returns the number of launches
// (< 0: the plan does not fit / an internal check failed), the WB sums in out / inf, the launches in desc.
extern "C" int bs_reduce(int cid, const uint8_t* xy64, uint32_t M, uint32_t WB, uint32_t cap, uint32_t wide_above, uint8_t* out,
                         uint8_t* inf, uint32_t* desc) {
  try {
    switch (cid) {
      case 0: return run<0>(xy64, M, WB, cap, wide_above, out, inf, desc);
      case 1: return run<1>(xy64, M, WB, cap, wide_above, out, inf, desc);
      case 2: return run<2>(xy64, M, WB, cap, wide_above, out, inf, desc);
      case 3: return run<3>(xy64, M, WB, cap, wide_above, out, inf, desc);
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "bs_reduce: %s\n", e.what());
    return -4;
  }
  return -5;
}
