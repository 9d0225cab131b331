// tests/cpp/r1cs_eval_mirror_test.cpp -- nova::resident::r1cs_evaluate (include/nova_mi355x.hpp) on the three-constraint circuit of
// r1cs_sat_mirror_test.cpp over the BN254 scalar field.  RelaxedR1CSSNARK::verify's multi_evaluate: src/spartan/snark.rs:325-353.
// Exit code 0 = pass, 3 = no GPU (NMX_E_NO_DEVICE), else fail.
//
//   columns 0..3 = W, 4 = the constant / u, 5 = x0          A: (0,0) (1,0) (1,1) (2,5), all 1     B: (0,1) (1,4) (2,0), all 1
//                                                           C: (0,2) 1, (1,3) 1, (2,4) 14
//   r_x = (2, 3):     T_x = [(1-2)(1-3), (1-2) 3, 2 (1-3), 6] = [2, -3, -4, 6]
//   r_y = (1, 0, 3):  T_y = 0 except T_y[4] = 1 (1-0) (1-3) = -2 and T_y[5] = 1 (1-0) 3 = 3
//   A~ = T_x[2] T_y[5] = -12        B~ = T_x[1] T_y[4] = 6        C~ = 14 T_x[2] T_y[4] = 112
//   r_x = (0, 1), r_y = (1, 0, 0): eq collapses to row 1 and column 4 -- the entries themselves: (0, 1, 0)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/nova_mi355x.hpp"

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
#define EXPECT(cond)                                                 \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
      return 1;                                                      \
    }                                                                \
  } while (0)

static int run() {
  const uint64_t ipA[4] = {0, 1, 3, 4}, ixA[4] = {0, 0, 1, 5};
  const uint64_t ipB[4] = {0, 1, 2, 3}, ixB[3] = {1, 4, 0};
  const uint64_t ipC[4] = {0, 1, 2, 3}, ixC[3] = {2, 3, 4};
  const std::vector<Scalar> dA(4, small(1)), dB(3, small(1)), dC{small(1), small(1), small(14)};
  uint64_t mats[3] = {0, 0, 0};
  check(nmx_spmv_register(NMX_F_BN254_FR, ipA, ixA, dA[0].data(), 3, 6, 0, &mats[0]));  // (the first call that needs the device)
  check(nmx_spmv_register(NMX_F_BN254_FR, ipB, ixB, dB[0].data(), 3, 6, 0, &mats[1]));
  check(nmx_spmv_register(NMX_F_BN254_FR, ipC, ixC, dC[0].data(), 3, 6, 0, &mats[2]));

  std::vector<Scalar> e = res::r1cs_evaluate(mats, 3, {small(2), small(3)}, {small(1), small(0), small(3)});
  EXPECT(e.size() == 3 && e[0] == neg_small(12) && e[1] == small(6) && e[2] == small(112));
  e = res::r1cs_evaluate(mats, 3, {small(0), small(1)}, {small(1), small(0), small(0)});
  EXPECT(e[0] == small(0) && e[1] == small(1) && e[2] == small(0));
  e = res::r1cs_evaluate(mats + 2, 1, {small(2), small(3)}, {small(1), small(0), small(3)});  // one matrix
  EXPECT(e.size() == 1 && e[0] == small(112));
  // variables beyond what the shape needs: the extra top variable of r_x at 0 changes nothing, at 1 it selects rows that do not exist
  e = res::r1cs_evaluate(mats, 3, {small(0), small(2), small(3)}, {small(1), small(0), small(3)});
  EXPECT(e[0] == neg_small(12) && e[1] == small(6) && e[2] == small(112));
  e = res::r1cs_evaluate(mats, 3, {small(1), small(2), small(3)}, {small(1), small(0), small(3)});
  EXPECT(e[0] == small(0) && e[1] == small(0) && e[2] == small(0));
  // the shape rule: 3 rows need ell_x >= 2, 6 columns need ell_y >= 3
  for (int which = 0; which < 2; which++) {
    try {
      if (which == 0) res::r1cs_evaluate(mats, 3, {small(2)}, {small(1), small(0), small(3)});
      else res::r1cs_evaluate(mats, 3, {small(2), small(3)}, {small(1), small(0)});
      return 1;
    } catch (const Error& err) {
      EXPECT(err.code == NMX_E_ARG);
    }
  }
  try {
    const uint64_t bad[1] = {0xdeadbeefull};
    res::r1cs_evaluate(bad, 1, {small(2), small(3)}, {small(1), small(0), small(3)});
    return 1;
  } catch (const Error& err) {
    EXPECT(err.code == NMX_E_HANDLE);
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
  printf("r1cs_eval mirror ok\n");
  return 0;
}
