// tests/cpp/ipa_verify_mirror_test.cpp -- nova::ipa::verify (include/nova_mi355x.hpp) on a four-element instance over Grumpkin: the proof
// comes from the oracle's key-folding prover (libnova_ref.so) under fixed small challenges, comm_a from the oracle's MSM.
// InnerProductArgument::verify: src/provider/ipa_pc.rs:286-390.  Exit code 0 = pass, 3 = no GPU (NMX_E_NO_DEVICE), else fail.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/nova_mi355x.hpp"

extern "C" {
typedef int (*ref_ipa_transcript_fn)(void* ctx, const uint8_t* L, int L_inf, const uint8_t* R, int R_inf, uint8_t* r32);
int ref_msm(int curve, const uint8_t* scalars_le32, const uint8_t* bases_xy64, size_t n, uint8_t* out, uint8_t* is_inf);
int ref_sequential_bases(int curve, const uint8_t* gen, uint64_t k0, size_t n, uint8_t* out);
int ref_ipa_prove(int curve, const uint8_t* ck_xy64, const uint8_t* ck_c_xy64, const uint8_t* a_le32, const uint8_t* b_le32, size_t n,
                  ref_ipa_transcript_fn cb, void* ctx, uint8_t* out_L, uint8_t* out_R, uint8_t* out_inf, uint8_t* out_a_hat);
}
using namespace nova::provider;
namespace ipa = nova::ipa;

static Scalar small(uint64_t v) {
  Scalar s{};
  memcpy(s.data(), &v, 8);
  return s;
}
struct Fixed {  // the stand-in transcript: challenge 5, 6, ...
  std::vector<Scalar> rs;
};
static int fixed_cb(void* ctx, const uint8_t*, int, const uint8_t*, int, uint8_t* out) {
  Fixed* f = static_cast<Fixed*>(ctx);
  f->rs.push_back(small(5 + f->rs.size()));
  memcpy(out, f->rs.back().data(), 32);
  return 0;
}
#define EXPECT(cond)                                                 \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
      return 1;                                                      \
    }                                                                \
  } while (0)

static int run() {
  // Grumpkin's generator (1, sqrt(-16)): bn256_grumpkin.rs:84-92
  static const uint8_t gy[32] = {0x2c, 0x27, 0x3f, 0x82, 0x8d, 0xc4, 0x3f, 0x83, 0x94, 0x12, 0x18, 0xf1, 0x45, 0x0d, 0x27, 0x2d,
                                 0x63, 0x5d, 0xa4, 0x06, 0x75, 0x5e, 0x13, 0xcf, 0x02, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00};
  uint8_t gen[64] = {0};
  gen[0] = 1;
  memcpy(gen + 32, gy, 32);
  const size_t n = 4;
  std::vector<Affine> pts(n + 1);
  EXPECT(ref_sequential_bases(NMX_GRUMPKIN, gen, 321, n + 1, pts[0].data()) == 0);
  const std::vector<Affine> bases(pts.begin(), pts.begin() + n);
  CommitmentKey ck(NMX_GRUMPKIN, bases, pts[n]);  // (the first call that needs the device: NMX_E_NO_DEVICE surfaces here)
  const Affine ck_c = pts[n];

  const std::vector<Scalar> a{small(2), small(3), small(5), small(7)}, b{small(1), small(4), small(9), small(16)};
  const Scalar c = small(2 * 1 + 3 * 4 + 5 * 9 + 7 * 16);
  Point comm_a;
  uint8_t inf = 0;
  EXPECT(ref_msm(NMX_GRUMPKIN, a[0].data(), bases[0].data(), n, comm_a.xy.data(), &inf) == 0 && !inf);
  comm_a.is_inf = false;  // (a default Point is the identity)

  Fixed tr;
  uint8_t L[128], R[128], infs[4];
  ipa::InnerProductArgument proof;
  EXPECT(ref_ipa_prove(NMX_GRUMPKIN, bases[0].data(), ck_c.data(), a[0].data(), b[0].data(), n, &fixed_cb, &tr, L, R, infs,
                       proof.a_hat.data()) == 0);
  proof.L_vec.resize(2), proof.R_vec.resize(2);
  for (size_t k = 0; k < 2; k++) {
    memcpy(proof.L_vec[k].xy.data(), L + 64 * k, 64), memcpy(proof.R_vec[k].xy.data(), R + 64 * k, 64);
    proof.L_vec[k].is_inf = infs[2 * k] != 0, proof.R_vec[k].is_inf = infs[2 * k + 1] != 0;
  }
  EXPECT(ipa::verify(ck, ck_c, comm_a, c, b, proof, tr.rs));
  // each single change is refused
  ipa::InnerProductArgument bad = proof;
  bad.a_hat[0] ^= 1;
  EXPECT(!ipa::verify(ck, ck_c, comm_a, c, b, bad, tr.rs));
  bad = proof;
  std::swap(bad.L_vec[1], bad.R_vec[1]);
  EXPECT(!ipa::verify(ck, ck_c, comm_a, c, b, bad, tr.rs));
  EXPECT(!ipa::verify(ck, ck_c, comm_a, small(172), b, proof, tr.rs));
  std::vector<Scalar> b2 = b;
  b2[3] = small(17);
  EXPECT(!ipa::verify(ck, ck_c, comm_a, c, b2, proof, tr.rs));
  std::vector<Scalar> rs2 = tr.rs;
  rs2[0] = small(9);
  EXPECT(!ipa::verify(ck, ck_c, comm_a, c, b, proof, rs2));
  // the reference's length rule (:297-303) and a zero challenge (`batch_invert(&r)?`, :328)
  try {
    ipa::verify(ck, ck_c, comm_a, c, std::vector<Scalar>(b.begin(), b.begin() + 3), proof, tr.rs);
    return 1;
  } catch (const std::invalid_argument&) {
  }
  rs2[0] = small(0);
  try {
    ipa::verify(ck, ck_c, comm_a, c, b, proof, rs2);
    return 1;
  } catch (const Error& e) {
    EXPECT(e.code == NMX_E_ZERO);
  }
  return 0;
}

int main() {
  try {
    if (run()) return 1;
  } catch (const Error& e) {
    fprintf(stderr, "%s\n", e.what());
    return e.code == NMX_E_NO_DEVICE ? 3 : 2;
  }
  printf("ipa_verify mirror ok\n");
  return 0;
}
