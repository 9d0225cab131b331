// tests/cpp/mercury_mirror_test.cpp -- the host-side plan of nmx_mercury_divide_by_binomial (nova_amd/csrc/mercury.hpp: mercury_plan,
// mercury_alpha_pow) as a stand-alone g++ program: no library, no device.  tests/test_mercury_abi.py compares every line with Python.
//   mercury_mirror_test plan  n_rows n_cols option          -> "seg_rows segs last_rows"
//   mercury_mirror_test pow   field_id alpha_hex exponent   -> alpha^exponent as 64 hex digits (alpha canonical, below p)
//   mercury_mirror_test self                                -> a few fixed cases, "mercury mirror ok" (the form a sanitizer build runs)
// divide_by_binomial: src/provider/mercury.rs:319-356 of the reference.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../host_emul/simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/msm_pipeline.hpp"
#include "../../nova_amd/csrc/mercury.hpp"

using namespace nmx;

// canonical integer (64 hex digits, most significant first) -> alpha^e, canonical integer, through the internal form as the call does
template <int FID> static void pow_hex(const char* hex, uint64_t e, char* out65) {
  uint32_t w[8] = {0};
  for (int i = 0; i < 64; i++) {
    const char ch = hex[63 - i];
    const uint32_t d = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
    w[i / 8] |= d << (4 * (i % 8));
  }
  const Fp<FID> a = Fp<FID>::from_words(w).to_internal().canon();
  mercury_alpha_pow<FID>(a, e).to_canonical().to_words(w);
  for (int i = 0; i < 64; i++) out65[63 - i] = "0123456789abcdef"[(w[i / 8] >> (4 * (i % 8))) & 15u];
  out65[64] = 0;
}
static int pow_any(int fid, const char* hex, uint64_t e, char* out65) {
  if (strlen(hex) != 64) return 1;
  switch (fid) {
    case 0: pow_hex<0>(hex, e, out65); return 0;
    case 1: pow_hex<1>(hex, e, out65); return 0;
    case 2: pow_hex<2>(hex, e, out65); return 0;
    case 3: pow_hex<3>(hex, e, out65); return 0;
  }
  return 1;
}
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

static int self_test() {
  MercuryPlan p = mercury_plan(1024, 1024, 0);
  EXPECT(p.seg_rows == 16 && p.segs == 64 && p.last_rows == 16);
  p = mercury_plan(512, 1024, 0);
  EXPECT(p.seg_rows == 8 && p.segs == 64 && p.last_rows == 8);
  p = mercury_plan(17, 65, 0);
  EXPECT(p.seg_rows == 4 && p.segs == 5 && p.last_rows == 1);
  p = mercury_plan(3, 5, 0);
  EXPECT(p.seg_rows == 3 && p.segs == 1 && p.last_rows == 3);
  p = mercury_plan(9, 65, 4);
  EXPECT(p.seg_rows == 4 && p.segs == 3 && p.last_rows == 1);
  p = mercury_plan(9, 65, 100);
  EXPECT(p.seg_rows == 9 && p.segs == 1 && p.last_rows == 9);
  p = mercury_plan((size_t)1 << 20, 1, 1);  // a tiny option on a tall shape: the grid cap
  EXPECT(p.segs <= kMercuryGridSegs && (size_t)(p.segs - 1) * p.seg_rows + p.last_rows == ((size_t)1 << 20) && p.last_rows >= 1 && p.last_rows <= p.seg_rows);
  char out[65];
  const char* two = "0000000000000000000000000000000000000000000000000000000000000002";
  EXPECT(pow_any(1, two, 10, out) == 0 && strcmp(out, "0000000000000000000000000000000000000000000000000000000000000400") == 0);
  EXPECT(pow_any(2, two, 0, out) == 0 && strcmp(out, "0000000000000000000000000000000000000000000000000000000000000001") == 0);
  printf("mercury mirror ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "self")) return self_test();
  if (argc == 5 && !strcmp(argv[1], "plan")) {
    const MercuryPlan p = mercury_plan(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), (uint32_t)strtoul(argv[4], nullptr, 10));
    printf("%u %u %u\n", p.seg_rows, p.segs, p.last_rows);
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "pow")) {
    char out[65];
    if (pow_any(atoi(argv[2]), argv[3], strtoull(argv[4], nullptr, 10), out)) return 2;
    printf("%s\n", out);
    return 0;
  }
  fprintf(stderr, "usage: mercury_mirror_test plan n_rows n_cols option | pow field_id alpha_hex exponent | self\n");
  return 2;
}
