// tests/cpp/host_point4_test.cpp -- TEST-ONLY: the host point arithmetic on 4 x 64-bit limbs (nova_amd/csrc/host_point4.hpp) against
// XYZZ<FID> (curve.hpp) compiled for the host, and combine_slices against the weighted sum it stands for.
//
// Points come in as affine bytes (x || y canonical little-endian, 64 zero bytes = the identity) with a scaling factor lambda each:
// the helper builds the representative (lambda^2 x, lambda^3 y, lambda^2, lambda^3), stores it as the device does (XYZZW) and runs
// the operation on HostPoint4 (load, operate, store) and on XYZZ; both answers go back as affine bytes.  g++ only: a shared
// library for tests/test_host_point4.py, or -- with -DHP4_MAIN -- a stand-alone program that checks itself on multiples of the
// generators (the form the sanitizer build runs) and times combine_slices.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/host_point4.hpp"

using namespace nmx;

template <int BF> static XYZZW scaled(const uint8_t* xy64, const uint8_t* lambda32) {
  Affine<BF> a;
  a.x = fp_from_bytes<BF>(xy64);
  a.y = fp_from_bytes<BF>(xy64 + 32);
  XYZZW w;
  if (a.is_identity()) {
    XYZZ<BF>::identity().store(w);
    return w;
  }
  const Fp<BF> lam = fp_from_bytes<BF>(lambda32).to_internal();
  const Fp<BF> l2 = lam * lam, l3 = l2 * lam;
  XYZZ<BF> p;
  p.x = a.x.to_internal() * l2;
  p.y = a.y.to_internal() * l3;
  p.zz = l2;
  p.zzz = l3;
  p.store(w);
  return w;
}
template <int BF> static void to_bytes(const XYZZW& w, uint8_t* out, uint8_t* inf) {
  xyzz_to_xy64<BF>(XYZZ<BF>::load(w), out, inf);
}

// op 0: P + Q, op 1: 2 P.  out / inf: [0] HostPoint4, [1] XYZZ.
template <int CID>
static int op_run(int op, const uint8_t* p64, const uint8_t* lp, const uint8_t* q64, const uint8_t* lq, uint8_t* out, uint8_t* inf) {
  constexpr int BF = CurveT<CID>::BF;
  const XYZZW pw = scaled<BF>(p64, lp), qw = scaled<BF>(q64, lq);
  HostPoint4<BF> h = HostPoint4<BF>::load(pw);
  XYZZ<BF> x = XYZZ<BF>::load(pw);
  if (op == 0) {
    h.add(HostPoint4<BF>::load(qw));
    x.add(XYZZ<BF>::load(qw));
  } else {
    h.dbl_in_place();
    x.dbl_in_place();
  }
  XYZZW hw, xw;
  h.store(hw);
  x.store(xw);
  for (int c = 0; c < 4; c++) {  // at rest every coordinate is canonical
    uint64_t t[4];
    memcpy(t, hw.w + 8 * c, 32);
    if (HostFp4<BF>::geq(t, HostFp4<BF>::C().p)) return -2;
  }
  if (h.is_identity() != x.is_identity()) return -3;
  to_bytes<BF>(hw, out, inf);
  to_bytes<BF>(xw, out + 64, inf + 1);
  return 0;
}
extern "C" int hp4_op(int cid, int op, const uint8_t* p64, const uint8_t* lp, const uint8_t* q64, const uint8_t* lq, uint8_t* out,
                      uint8_t* inf) {
  switch (cid) {
    case 0: return op_run<0>(op, p64, lp, q64, lq, out, inf);
    case 1: return op_run<1>(op, p64, lp, q64, lq, out, inf);
    case 2: return op_run<2>(op, p64, lp, q64, lq, out, inf);
    case 3: return op_run<3>(op, p64, lp, q64, lq, out, inf);
  }
  return -1;
}

// pts: L + 1 affine points (the root, then O_0 .. O_(L-1)), lambdas: as many scaling factors.  out: root + sum_l 2^l O_l.
template <int CID> static int combine_run(const uint8_t* pts, const uint8_t* lambdas, uint32_t L, uint8_t* out, uint8_t* inf) {
  constexpr int BF = CurveT<CID>::BF;
  std::vector<XYZZW> s(L + 1);
  for (uint32_t i = 0; i <= L; i++) s[i] = scaled<BF>(pts + 64 * i, lambdas + 32 * i);
  XYZZW r;
  combine_slices<BF>(s.data(), L, &r);
  to_bytes<BF>(r, out, inf);
  return 0;
}
extern "C" int hp4_combine(int cid, const uint8_t* pts, const uint8_t* lambdas, uint32_t L, uint8_t* out, uint8_t* inf) {
  switch (cid) {
    case 0: return combine_run<0>(pts, lambdas, L, out, inf);
    case 1: return combine_run<1>(pts, lambdas, L, out, inf);
    case 2: return combine_run<2>(pts, lambdas, L, out, inf);
    case 3: return combine_run<3>(pts, lambdas, L, out, inf);
  }
  return -1;
}

#ifdef HP4_MAIN
template <int CID> static void gen_multiple(uint64_t k, uint8_t* xy64) {
  constexpr int BF = CurveT<CID>::BF;
  Affine<BF> g;
  g.x = Fp<BF>::from_words(CurveT<CID>::GX).to_internal().canon();
  g.y = Fp<BF>::from_words(CurveT<CID>::GY).to_internal().canon();
  const uint32_t kw[8] = {(uint32_t)k, (uint32_t)(k >> 32), 0, 0, 0, 0, 0, 0};
  uint8_t inf;
  xyzz_to_xy64<BF>(scalar_mul<BF>(XYZZ<BF>::from_affine(g), kw), xy64, &inf);
}
static void lambda_of(uint64_t seed, uint8_t* l32) {
  memset(l32, 0, 32);
  uint64_t x = seed * 0x9e3779b97f4a7c15ull + 1;
  for (int i = 0; i < 3; i++) {  // 192 bits: below every modulus
    x ^= x >> 29, x *= 0xbf58476d1ce4e5b9ull, x ^= x >> 32;
    memcpy(l32 + 8 * i, &x, 8);
  }
  l32[0] |= 1;
}
static int g_bad = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "host_point4: line %d: %s\n", __LINE__, #cond); \
      g_bad++;                                                        \
    }                                                                 \
  } while (0)

template <int CID> static void self_check() {
  constexpr int BF = CurveT<CID>::BF;
  uint8_t P[64], Q[64], N[64], Z[64] = {0}, lp[32], lq[32], out[128], inf[2];
  gen_multiple<CID>(12345, P);
  gen_multiple<CID>(67890, Q);
  memcpy(N, P, 64);  // -P
  {
    Affine<BF> a;
    a.x = fp_from_bytes<BF>(P).to_internal().canon();
    a.y = fp_from_bytes<BF>(P + 32).to_internal().canon();
    const XYZZ<BF> n = XYZZ<BF>::from_affine(a).neg();
    uint8_t f;
    xyzz_to_xy64<BF>(n, N, &f);
  }
  lambda_of(7 + CID, lp), lambda_of(99 + CID, lq);
  const uint8_t* lhs[] = {P, Z, P, Z, P, P};
  const uint8_t* rhs[] = {Q, Q, Z, Z, P, N};
  for (int i = 0; i < 6; i++) {
    CHECK(hp4_op(CID, 0, lhs[i], lp, rhs[i], lq, out, inf) == 0);
    CHECK(memcmp(out, out + 64, 64) == 0 && inf[0] == inf[1]);
    if (i == 3 || i == 5) CHECK(inf[0] == 1);
  }
  CHECK(hp4_op(CID, 1, P, lp, P, lp, out, inf) == 0 && memcmp(out, out + 64, 64) == 0 && inf[0] == 0);
  CHECK(hp4_op(CID, 1, Z, lp, Z, lp, out, inf) == 0 && inf[0] == 1 && inf[1] == 1);
  for (uint32_t L : {1u, 2u, 7u, 16u, 19u}) {  // combine_slices against the definition on XYZZ
    std::vector<uint8_t> pts(64 * (L + 1)), lam(32 * (L + 1));
    XYZZ<BF> want = XYZZ<BF>::identity();
    for (uint32_t i = 0; i <= L; i++) {
      if (i % 5 == 3) memset(&pts[64 * i], 0, 64);
      else gen_multiple<CID>(1000 + 17 * i, &pts[64 * i]);
      lambda_of(i + 1, &lam[32 * i]);
      XYZZ<BF> t = XYZZ<BF>::load(scaled<BF>(&pts[64 * i], &lam[32 * i]));
      for (uint32_t d = 1; d < i; d++) t.dbl_in_place();  // weights 1, 1, 2, 4, ...
      want.add(t);
    }
    uint8_t got[64], gi, exp[64], ei;
    CHECK(hp4_combine(CID, pts.data(), lam.data(), L, got, &gi) == 0);
    xyzz_to_xy64<BF>(want, exp, &ei);
    CHECK(memcmp(got, exp, 64) == 0 && gi == ei);
  }
}
template <int CID> static double time_combine(uint32_t L, int reps) {
  constexpr int BF = CurveT<CID>::BF;
  std::vector<XYZZW> s(L + 1);
  for (uint32_t i = 0; i <= L; i++) {
    uint8_t p[64], l[32];
    gen_multiple<CID>(555 + i, p);
    lambda_of(i + 3, l);
    s[i] = scaled<BF>(p, l);
  }
  XYZZW r;
  uint32_t sink = 0;
  for (int i = 0; i < 200; i++) combine_slices<BF>(s.data(), L, &r), sink += r.w[0];
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < reps; i++) {
    s[0].w[0] ^= sink & 1u;  // every call depends on the one before (the formulas never test the curve equation)
    combine_slices<BF>(s.data(), L, &r);
    sink += r.w[0];
  }
  const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
  if (sink == 0x12345678u) printf(" ");
  return us;
}
int main(int argc, char** argv) {
  self_check<0>();
  self_check<1>();
  self_check<2>();
  self_check<3>();
  if (g_bad) {
    fprintf(stderr, "host_point4: %d checks failed\n", g_bad);
    return 1;
  }
  printf("host_point4 self-check ok (4 curves)\n");
  if (argc > 1) {
    const int reps = atoi(argv[1]);
    for (uint32_t L : {7u, 14u, 16u, 19u})
      printf("combine_slices L = %2u: %.2f us (BN254 G1), %.2f us (Pallas)\n", L, time_combine<0>(L, reps), time_combine<2>(L, reps));
  }
  return 0;
}
#endif
