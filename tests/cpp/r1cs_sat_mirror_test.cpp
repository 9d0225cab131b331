// tests/cpp/r1cs_sat_mirror_test.cpp -- nova::resident::r1cs_is_sat / r1cs_is_sat_relaxed (include/nova_mi355x.hpp) on a three-constraint
// circuit over the BN254 scalar field, host operands (a proof received from a peer), expected commitments from the oracle
// (libnova_ref.so).  R1CSShape::is_sat / is_sat_relaxed: src/r1cs/mod.rs:474-574.  Exit code 0 = pass, 3 = no GPU (NMX_E_NO_DEVICE), else fail.
//
//   z = [w0 w1 w2 w3 | u | x0] = [2 3 6 5 | u | 7]         row 0: w0 * w1 = w2          row 1: (w0 + w1) * u = w3
//                                                          row 2: x0 * w0 = 14 u
// strict (u = 1): satisfied.  relaxed with u = 3: E = Az o Bz - u Cz = (6 - 18, 15 - 15, 14 - 126) = (-12, 0, -112).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/nova_mi355x.hpp"

extern "C" {
int ref_commit(int curve, const uint8_t* v, const uint8_t* ck, size_t n, const uint8_t* h, const uint8_t* r, uint8_t* out,
               uint8_t* inf);
int ref_sequential_bases(int curve, const uint8_t* gen, uint64_t k0, size_t n, uint8_t* out);
}
using namespace nova::provider;
namespace res = nova::resident;

static Scalar small(uint64_t v) {
  Scalar s{};
  memcpy(s.data(), &v, 8);
  return s;
}
// r - v for the BN254 scalar modulus r (v < 2^32)
static Scalar neg_small(uint32_t v) {
  static const uint8_t r_le[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                                   0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};
  Scalar s{};
  int64_t borrow = v;
  for (int i = 0; i < 32; i++) {
    int64_t d = (int64_t)r_le[i] - (borrow & 0xff);
    borrow >>= 8;
    if (d < 0) d += 256, borrow += 1;
    s[i] = (uint8_t)d;
  }
  return s;
}
static Point oracle_commit(const std::vector<Scalar>& v, const std::vector<Affine>& ck, const Affine& h, const Scalar& r) {
  Point p;
  uint8_t inf = 0;
  ref_commit(NMX_BN254_G1, v[0].data(), ck[0].data(), v.size(), h.data(), r.data(), p.xy.data(), &inf);
  p.is_inf = inf != 0;
  return p;
}
#define EXPECT(cond)                                                 \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
      return 1;                                                      \
    }                                                                \
  } while (0)

static int run() {
  uint8_t gen[64] = {0};
  gen[0] = 1, gen[32] = 2;  // BN254 G1 generator (1, 2)
  const size_t n = 4;
  std::vector<Affine> pts(n + 1);
  ref_sequential_bases(NMX_BN254_G1, gen, 99, n + 1, pts[0].data());
  const std::vector<Affine> bases(pts.begin(), pts.begin() + n);
  CommitmentKey ck(NMX_BN254_G1, bases, pts[n]);  // (the first call that needs the device: NMX_E_NO_DEVICE surfaces here)

  // CSR, columns 0..3 = W, 4 = the constant / u, 5 = x0
  const uint64_t ipA[4] = {0, 1, 3, 4}, ixA[4] = {0, 0, 1, 5};
  const uint64_t ipB[4] = {0, 1, 2, 3}, ixB[3] = {1, 4, 0};
  const uint64_t ipC[4] = {0, 1, 2, 3}, ixC[3] = {2, 3, 4};
  const std::vector<Scalar> dA(4, small(1)), dB(3, small(1)), dC{small(1), small(1), small(14)};
  uint64_t mats[3] = {0, 0, 0};
  check(nmx_spmv_register(NMX_F_BN254_FR, ipA, ixA, dA[0].data(), 3, 6, 0, &mats[0]));
  check(nmx_spmv_register(NMX_F_BN254_FR, ipB, ixB, dB[0].data(), 3, 6, 0, &mats[1]));
  check(nmx_spmv_register(NMX_F_BN254_FR, ipC, ixC, dC[0].data(), 3, 6, 0, &mats[2]));

  std::vector<Scalar> W{small(2), small(3), small(6), small(5)};
  const std::vector<Scalar> X{small(7)};
  const Scalar rW = small(1234567), rE = small(7654321), u = small(3);
  const std::vector<Scalar> E{neg_small(12), small(0), neg_small(112)};
  const Point cW = oracle_commit(W, bases, pts[n], rW);
  const Point cE = oracle_commit(E, bases, pts[n], rE);

  // strict
  res::SatResult s = res::r1cs_is_sat(mats, &ck, W.data(), W.size(), X, cW, rW, /*device=*/false);
  EXPECT(s.ok() && s.bad_rows == 0 && s.first_bad_row == ~0ull);
  s = res::r1cs_is_sat(mats, nullptr, W.data(), W.size(), X, Point{}, Scalar{}, false);  // the equation only
  EXPECT(s.ok());
  s = res::r1cs_is_sat(mats, &ck, W.data(), W.size(), X, cE, rW, false);  // somebody else's commitment
  EXPECT(s.verdict == NMX_UNSAT_COMM_W && s.eq_ok() && !s.comm_W_ok());
  // relaxed
  s = res::r1cs_is_sat_relaxed(mats, &ck, W.data(), W.size(), E.data(), E.size(), u, X, cW, cE, rW, rE, false);
  EXPECT(s.ok() && s.bad_rows == 0);
  s = res::r1cs_is_sat_relaxed(mats, &ck, W.data(), W.size(), E.data(), E.size(), small(4), X, cW, cE, rW, rE, false);  // wrong u: rows 0 and 2 (row 1 is (w0 + w1) u = u w3 for every u)
  EXPECT(s.verdict == NMX_UNSAT_EQ && s.bad_rows == 2 && s.first_bad_row == 0);
  s = res::r1cs_is_sat_relaxed(mats, &ck, W.data(), W.size(), E.data(), E.size(), u, X, cW, cW, rW, rE, false);
  EXPECT(s.verdict == NMX_UNSAT_COMM_E);
  // a changed witness element: w3 only enters row 1 (as C z), and the commitment no longer matches
  W[3] = small(6);
  s = res::r1cs_is_sat(mats, &ck, W.data(), W.size(), X, cW, rW, false);
  EXPECT(s.verdict == (NMX_UNSAT_EQ | NMX_UNSAT_COMM_W) && s.bad_rows == 1 && s.first_bad_row == 1);
  // the reference's length checks
  try {
    res::r1cs_is_sat(mats, &ck, W.data(), W.size() - 1, X, cW, rW, false);
    return 1;
  } catch (const Error& e) {
    EXPECT(e.code == NMX_E_ARG);
  }
  for (uint64_t m : mats) check(nmx_spmv_unregister(m));
  return 0;
}

int main() {
  try {
    if (run()) return 1;
  } catch (const Error& e) {
    fprintf(stderr, "%s\n", e.what());
    return e.code == NMX_E_NO_DEVICE ? 3 : 2;
  }
  printf("r1cs_sat mirror ok\n");
  return 0;
}
