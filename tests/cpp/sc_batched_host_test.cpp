// tests/cpp/sc_batched_host_test.cpp -- g++-only harness around sc_tail_rounds_batched (nova_amd/csrc/sc_host.hpp): the host tail of
// nmx_sumcheck_prove_batched_cubic run from round 1 as a complete prover over host tables, so that tests/test_sumcheck_batched_abi.py can
// put it through check_batched_cubic without a GPU.  Test scaffolding: the product reaches this code only through
// nova_amd/csrc/sumcheck_batched.hpp.  With main() (-DSCB_MAIN) it is a stand-alone program for a sanitizer build.
#include <stdio.h>

#include "../../nova_amd/csrc/sc_host.hpp"

using namespace nmx;

namespace {
template <int FID>
int prove(int mont, const uint8_t* claim, const uint8_t* taus, size_t nr, const uint8_t* const* As, const uint8_t* const* Bs, const uint8_t* const* Cs,
          const uint8_t* alphas, size_t k, TranscriptFn cb, void* ctx, uint8_t* out_polys, uint8_t* out_r, uint8_t* out_claims) {
  using H = HostFp4<FID>;
  if (k == 0) return -3;  // InvalidNumInstances
  try {
    ScAlg<FID> alg(mont != 0);
    typename ScAlg<FID>::Eq eq;
    eq.init(alg, taus, (uint32_t)nr);
    const size_t n = (size_t)1 << nr;
    std::vector<std::vector<H>> A(k), B(k), C(k);
    std::vector<H> al(k);
    for (size_t i = 0; i < k; i++) {
      A[i].resize(n), B[i].resize(n), C[i].resize(n);
      for (size_t x = 0; x < n; x++) A[i][x] = alg.in(As[i] + 32 * x), B[i][x] = alg.in(Bs[i] + 32 * x), C[i][x] = alg.in(Cs[i] + 32 * x);
      al[i] = alg.in(alphas + 32 * i);
    }
    H cl = alg.in(claim);
    sc_tail_rounds_batched<FID>(alg, &eq, (uint32_t)nr, 1, cl, A, B, C, al, cb, ctx, out_polys, out_r);
    for (size_t i = 0; i < k; i++) alg.out(A[i][0], out_claims + 96 * i), alg.out(B[i][0], out_claims + 96 * i + 32), alg.out(C[i][0], out_claims + 96 * i + 64);
    return 0;
  } catch (const ScFail& f) {
    fprintf(stderr, "sc_batched_host_test: %s\n", f.msg.c_str());
    return -f.code;
  }
}
}  // namespace

extern "C" int hscb_prove_batched_cubic(int field, int mont, const uint8_t* claim, const uint8_t* taus, size_t nr, const uint8_t* const* As,
                                        const uint8_t* const* Bs, const uint8_t* const* Cs, const uint8_t* alphas, size_t k, TranscriptFn cb,
                                        void* ctx, uint8_t* out_polys, uint8_t* out_r, uint8_t* out_claims) {
  switch (field) {
    case 0: return prove<0>(mont, claim, taus, nr, As, Bs, Cs, alphas, k, cb, ctx, out_polys, out_r, out_claims);
    case 1: return prove<1>(mont, claim, taus, nr, As, Bs, Cs, alphas, k, cb, ctx, out_polys, out_r, out_claims);
    case 2: return prove<2>(mont, claim, taus, nr, As, Bs, Cs, alphas, k, cb, ctx, out_polys, out_r, out_claims);
    case 3: return prove<3>(mont, claim, taus, nr, As, Bs, Cs, alphas, k, cb, ctx, out_polys, out_r, out_claims);
    default: return -100;
  }
}

#ifdef SCB_MAIN
// A proof over small-integer tables with a fixed-challenge transcript, every field, a tau of zero included: each round polynomial must
// satisfy p(0) + p(1) == the running claim (SumcheckProof::verify, sumcheck.rs:87-129).  For -fsanitize=address,undefined builds.
namespace {
struct Tr {
  int field, bad = 0;
  uint8_t claim[32];
};
template <int FID> void round_check(Tr* t, const uint8_t* co, uint8_t* ch) {
  using H = HostFp4<FID>;
  ScAlg<FID> alg(false);
  H c[4];
  for (int i = 0; i < 4; i++) c[i] = alg.in(co + 32 * i);
  const H at0 = c[0], at1 = c[0] + c[1] + c[2] + c[3];
  uint8_t got[32];
  alg.out(at0 + at1, got);
  if (memcmp(got, t->claim, 32)) t->bad++;
  memset(ch, 0, 32);
  ch[0] = 5, ch[9] = 0x77;
  alg.out(ScAlg<FID>::poly_eval(c, 4, alg.in(ch)), t->claim);
}
int tr_cb(void* ctx, const uint8_t* co, size_t n, uint8_t* ch) {
  Tr* t = (Tr*)ctx;
  if (n != 4) return 1;
  switch (t->field) {
    case 0: round_check<0>(t, co, ch); break;
    case 1: round_check<1>(t, co, ch); break;
    case 2: round_check<2>(t, co, ch); break;
    default: round_check<3>(t, co, ch); break;
  }
  return 0;
}
}  // namespace
int main() {
  const size_t nr = 4, n = 16, k = 3;
  for (int field = 0; field < 4; field++)
    for (int zero_tau = 0; zero_tau < 2; zero_tau++) {
      std::vector<std::vector<uint8_t>> tab(3 * k, std::vector<uint8_t>(32 * n, 0));
      for (size_t t = 0; t < 3 * k; t++)
        for (size_t x = 0; x < n; x++) tab[t][32 * x] = (uint8_t)(1 + 7 * t + 3 * x), tab[t][32 * x + 1] = (uint8_t)(t * x);
      uint8_t taus[32 * 4] = {0}, alphas[32 * 3] = {0};
      for (size_t j = 0; j < nr; j++) taus[32 * j] = (uint8_t)(2 + j);
      if (zero_tau) taus[32 * 1] = 0;
      for (size_t i = 0; i < k; i++) alphas[32 * i] = (uint8_t)(3 + i);
      // the claim by brute force in host arithmetic: eq(tau, x) over the hypercube, most significant variable first
      auto claim_of = [&](auto F) {
        constexpr int FID = decltype(F)::value;
        using H = HostFp4<FID>;
        ScAlg<FID> alg(false);
        H sum = H::zero();
        for (size_t x = 0; x < n; x++) {
          H e = H::one();
          for (size_t j = 0; j < nr; j++) {
            const H tau = alg.in(taus + 32 * j);
            e = e * (((x >> (nr - 1 - j)) & 1) ? tau : H::one() - tau);
          }
          H inner = H::zero();
          for (size_t i = 0; i < k; i++)
            inner = inner + alg.in(alphas + 32 * i) * (alg.in(&tab[i][32 * x]) * alg.in(&tab[k + i][32 * x]) - alg.in(&tab[2 * k + i][32 * x]));
          sum = sum + e * inner;
        }
        Tr t;
        t.field = FID;
        alg.out(sum, t.claim);
        return t;
      };
      Tr t = field == 0 ? claim_of(std::integral_constant<int, 0>{}) : field == 1 ? claim_of(std::integral_constant<int, 1>{})
           : field == 2 ? claim_of(std::integral_constant<int, 2>{}) : claim_of(std::integral_constant<int, 3>{});
      const uint8_t *As[3], *Bs[3], *Cs[3];
      for (size_t i = 0; i < k; i++) As[i] = tab[i].data(), Bs[i] = tab[k + i].data(), Cs[i] = tab[2 * k + i].data();
      uint8_t claim0[32], polys[128 * 4], r[32 * 4], claims[96 * 3];
      memcpy(claim0, t.claim, 32);
      const int rc = hscb_prove_batched_cubic(field, 0, claim0, taus, nr, As, Bs, Cs, alphas, k, tr_cb, &t, polys, r, claims);
      if (rc != 0 || t.bad) {
        fprintf(stderr, "sc_batched_host_test: field %d zero_tau %d: rc %d, %d rounds with p(0) + p(1) != claim\n", field, zero_tau, rc, t.bad);
        return 1;
      }
    }
  printf("sc_batched host tail ok\n");
  return 0;
}
#endif
