// tests/cpp/sc_ppsnark_host_test.cpp -- g++-only harness around sc_tail_rounds_ppsnark (nova_amd/csrc/sc_host.hpp): the host tail of
// nmx_sumcheck_prove_ppsnark run from round 1 as a complete prover over sixteen host tables, so that tests/test_sumcheck_ppsnark_abi.py can
// put it through tests/ppsnark_sc_common.py without a GPU.  Test scaffolding: the product reaches this code only through
// nova_amd/csrc/sumcheck_ppsnark.hpp.  With main() (-DSCP_MAIN) it is a stand-alone program for a sanitizer build.
#include <stdio.h>

#include "../../nova_amd/csrc/sc_host.hpp"

using namespace nmx;

namespace {
template <int FID>
int prove(int mont, size_t nr, const uint8_t* const* tables, const uint8_t* rhos, const uint8_t* r_outer, const uint8_t* claims2, const uint8_t* coeffs9,
          TranscriptFn cb, void* ctx, uint8_t* out_polys, uint8_t* out_r, uint8_t* out_finals) {
  using H = HostFp4<FID>;
  try {
    ScAlg<FID> alg(mont != 0);
    ScPps<FID> st;
    st.init(alg, rhos, r_outer, claims2, coeffs9, (uint32_t)nr);
    const size_t n = (size_t)1 << nr;
    std::vector<H> T[ScPps<FID>::kTables];
    for (uint32_t t = 0; t < ScPps<FID>::kTables; t++) {
      T[t].resize(n);
      for (size_t x = 0; x < n; x++) T[t][x] = alg.in(tables[t] + 32 * x);
    }
    sc_tail_rounds_ppsnark<FID>(alg, st, (uint32_t)nr, 1, T, cb, ctx, out_polys, out_r);
    for (uint32_t t = 0; t < ScPps<FID>::kTables; t++) alg.out(T[t][0], out_finals + 32 * t);
    return 0;
  } catch (const ScFail& f) {
    fprintf(stderr, "sc_ppsnark_host_test: %s\n", f.msg.c_str());
    return -f.code;
  }
}
}  // namespace

extern "C" int hscp_prove_ppsnark(int field, int mont, size_t nr, const uint8_t* const* tables, const uint8_t* rhos, const uint8_t* r_outer,
                                  const uint8_t* claims2, const uint8_t* coeffs9, TranscriptFn cb, void* ctx, uint8_t* out_polys, uint8_t* out_r,
                                  uint8_t* out_finals) {
  switch (field) {
    case 0: return prove<0>(mont, nr, tables, rhos, r_outer, claims2, coeffs9, cb, ctx, out_polys, out_r, out_finals);
    case 1: return prove<1>(mont, nr, tables, rhos, r_outer, claims2, coeffs9, cb, ctx, out_polys, out_r, out_finals);
    case 2: return prove<2>(mont, nr, tables, rhos, r_outer, claims2, coeffs9, cb, ctx, out_polys, out_r, out_finals);
    case 3: return prove<3>(mont, nr, tables, rhos, r_outer, claims2, coeffs9, cb, ctx, out_polys, out_r, out_finals);
    default: return -100;
  }
}

#ifdef SCP_MAIN
// A proof over small-integer tables with a fixed-challenge transcript, every field, a zero rho / r_outer included.  The instance is not
// a true one (the derived claims start from a false zero), so what is checked is what holds for any tables: one callback per round and
// every final value its table's multilinear extension at the challenges.  For -fsanitize=address,undefined builds.
namespace {
int tr_cb(void* ctx, const uint8_t*, size_t n, uint8_t* ch) {
  if (n != 4) return 1;
  memset(ch, 0, 32);
  ch[0] = 5, ch[9] = 0x77;
  ++*(int*)ctx;
  return 0;
}
template <int FID> int one(int zero_tau) {
  using H = HostFp4<FID>;
  const size_t nr = 4, n = 16;
  ScAlg<FID> alg(false);
  std::vector<std::vector<uint8_t>> tab(16, std::vector<uint8_t>(32 * n, 0));
  for (size_t t = 0; t < 16; t++)
    for (size_t x = 0; x < n; x++) tab[t][32 * x] = (uint8_t)(1 + 7 * t + 3 * x), tab[t][32 * x + 1] = (uint8_t)(t * x);
  uint8_t rhos[32 * 4] = {0}, ro[32 * 4] = {0}, claims2[64] = {0}, coeffs[32 * 9] = {0};
  for (size_t j = 0; j < nr; j++) rhos[32 * j] = (uint8_t)(2 + j), ro[32 * j] = (uint8_t)(11 + j);
  if (zero_tau) rhos[32 * 1] = 0, ro[32 * 2] = 0;
  claims2[0] = 9, claims2[32] = 4;
  for (size_t i = 0; i < 9; i++) coeffs[32 * i] = (uint8_t)(3 + i);
  const uint8_t* ptr[16];
  for (size_t t = 0; t < 16; t++) ptr[t] = tab[t].data();
  uint8_t polys[128 * 4], r[32 * 4], fin[32 * 16];
  int calls = 0;
  if (hscp_prove_ppsnark(FID, 0, nr, ptr, rhos, ro, claims2, coeffs, tr_cb, &calls, polys, r, fin) != 0 || calls != (int)nr) return 1;
  for (size_t t = 0; t < 16; t++) {  // the finals: bind_poly_var_top four times
    std::vector<H> z(n);
    for (size_t x = 0; x < n; x++) z[x] = alg.in(&tab[t][32 * x]);
    for (size_t j = 0; j < nr; j++) ScAlg<FID>::bind_top(z, alg.in(r + 32 * j));
    uint8_t got[32];
    alg.out(z[0], got);
    if (memcmp(got, fin + 32 * t, 32)) return 2;
  }
  return 0;
}
}  // namespace
int main() {
  for (int zero_tau = 0; zero_tau < 2; zero_tau++) {
    const int rc[4] = {one<0>(zero_tau), one<1>(zero_tau), one<2>(zero_tau), one<3>(zero_tau)};
    for (int f = 0; f < 4; f++)
      if (rc[f]) {
        fprintf(stderr, "sc_ppsnark_host_test: field %d zero_tau %d: %d\n", f, zero_tau, rc[f]);
        return 1;
      }
  }
  printf("sc_ppsnark host tail ok\n");
  return 0;
}
#endif
