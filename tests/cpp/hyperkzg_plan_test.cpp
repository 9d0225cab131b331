// tests/cpp/hyperkzg_plan_test.cpp -- the host-side plan of nmx_poly_lincomb_quotients (nova_amd/csrc/hyperkzg.hpp: lq_plan, lq_point_powers,
// lq_q_powers) as a stand-alone g++ program: no library, no device.  tests/test_hyperkzg_abi.py compares every line with Python.
//   hyperkzg_plan_test plan   n_out option                 -> "chunk levels n_0 n_1 ..."
//   hyperkzg_plan_test upow   field_id u_hex n_out option  -> one line per level: u^(elements of level 0 per element of that level)
//   hyperkzg_plan_test qpow   field_id q_hex k             -> one line per power q^0 .. q^(k-1)
//   hyperkzg_plan_test self                                -> a few fixed cases, "hyperkzg plan ok" (the form a sanitizer build runs)
// Values are canonical integers of 64 hex digits, most significant first; they go through the internal form as the call takes them.
// kzg_open_batch: src/provider/hyperkzg.rs:1007-1072 of the reference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../host_emul/simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/msm_pipeline.hpp"
#include "../../nova_amd/csrc/hyperkzg.hpp"

using namespace nmx;

static bool parse_hex(const char* hex, uint32_t w[8]) {
  if (strlen(hex) != 64) return false;
  memset(w, 0, 32);
  for (int i = 0; i < 64; i++) {
    const char ch = hex[63 - i];
    const uint32_t d = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
    w[i / 8] |= d << (4 * (i % 8));
  }
  return true;
}
// an internal-form residue -> the canonical integer, printed
template <int FID> static void print_internal(const Fp<FID>& x) {
  uint32_t w[8];
  x.to_canonical().to_words(w);
  char out[65];
  for (int i = 0; i < 64; i++) out[63 - i] = "0123456789abcdef"[(w[i / 8] >> (4 * (i % 8))) & 15u];
  out[64] = 0;
  printf("%s\n", out);
}
template <int FID> static int upow(const char* hex, size_t n_out, uint32_t opt) {
  uint32_t w[8];
  if (!parse_hex(hex, w)) return 2;
  const LqPlan pl = lq_plan(n_out, opt);
  std::vector<Fp<FID>> out(pl.levels);
  lq_point_powers<FID>(HostFp4<FID>::from_canonical(w), pl, out.data());
  for (uint32_t l = 0; l < pl.levels; l++) print_internal<FID>(out[l]);
  return 0;
}
template <int FID> static int qpow(const char* hex, size_t k) {
  uint32_t w[8];
  if (!parse_hex(hex, w)) return 2;
  std::vector<uint32_t> pw(8 * (k ? k : 1));
  lq_q_powers<FID>(HostFp4<FID>::from_canonical(w), k, pw.data());
  for (size_t i = 0; i < k; i++) print_internal<FID>(Fp<FID>::from_words(pw.data() + 8 * i));
  return 0;
}
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

static int self_test() {
  LqPlan p = lq_plan(1, 0);
  EXPECT(p.chunk == 4 && p.levels == 1 && p.n[0] == 1);
  p = lq_plan(8, 8);
  EXPECT(p.chunk == 8 && p.levels == 1);
  p = lq_plan(9, 8);
  EXPECT(p.levels == 2 && p.n[1] == 2);
  p = lq_plan(129, 8);
  EXPECT(p.levels == 3 && p.n[1] == 17 && p.n[2] == 2);
  p = lq_plan((size_t)1 << 20, 8);
  EXPECT(p.levels == 6 && p.n[1] == (1u << 17) && p.n[2] == (1u << 13) && p.n[3] == (1u << 9) && p.n[4] == 32 && p.n[5] == 2);
  p = lq_plan((size_t)1 << 20, 0);
  EXPECT(p.chunk == 4 && p.levels == 6 && p.n[1] == (1u << 18) && p.n[5] == 4);
  p = lq_plan(((size_t)1 << 31) - 1, 4);
  EXPECT(p.chunk == 4 && p.levels <= kLqMaxLevels && p.n[p.levels - 1] <= kLqUpChunk);
  p = lq_plan(5, 4);
  EXPECT(p.chunk == 4 && p.levels == 2 && p.n[1] == 2);
  const char* two = "0000000000000000000000000000000000000000000000000000000000000002";
  EXPECT(upow<1>(two, 129, 8) == 0);  // 2, 2^8, 2^128
  EXPECT(qpow<2>(two, 3) == 0);       // 1, 2, 4
  printf("hyperkzg plan ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "self")) return self_test();
  if (argc == 4 && !strcmp(argv[1], "plan")) {
    const LqPlan p = lq_plan(strtoull(argv[2], nullptr, 10), (uint32_t)strtoul(argv[3], nullptr, 10));
    printf("%u %u", p.chunk, p.levels);
    for (uint32_t l = 0; l < p.levels; l++) printf(" %u", p.n[l]);
    printf("\n");
    return 0;
  }
  if (argc == 6 && !strcmp(argv[1], "upow")) {
    const size_t n = strtoull(argv[4], nullptr, 10);
    const uint32_t opt = (uint32_t)strtoul(argv[5], nullptr, 10);
    switch (atoi(argv[2])) {
      case 0: return upow<0>(argv[3], n, opt);
      case 1: return upow<1>(argv[3], n, opt);
      case 2: return upow<2>(argv[3], n, opt);
      case 3: return upow<3>(argv[3], n, opt);
    }
    return 2;
  }
  if (argc == 5 && !strcmp(argv[1], "qpow")) {
    const size_t k = strtoull(argv[4], nullptr, 10);
    switch (atoi(argv[2])) {
      case 0: return qpow<0>(argv[3], k);
      case 1: return qpow<1>(argv[3], k);
      case 2: return qpow<2>(argv[3], k);
      case 3: return qpow<3>(argv[3], k);
    }
    return 2;
  }
  fprintf(stderr, "usage: hyperkzg_plan_test plan n_out option | upow field_id u_hex n_out option | qpow field_id q_hex k | self\n");
  return 2;
}
