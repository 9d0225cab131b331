// tests/cpp/mercury_host_test.cpp -- the host-side algebra of nmx_mercury_prove's batch opening (nova_amd/csrc/mercury_host.hpp:
// generate_batch_evaluate_arg, src/provider/mercury.rs:567-770 of the reference) as a stand-alone g++ program: no library, no device.
// tests/test_mercury_prove_abi.py compares every line with the restatement in Python integers (tests/mercury_prove_common.py).
//   mercury_host_test open field_id b mont     stdin: g (b values), h (b), s (b - 1), zeta, alpha, beta, z
//        -> "degenerate" when two opening points coincide, else the eight evaluations (g_zeta, g_zeta_inv, h_zeta, h_zeta_inv, h_alpha,
//           s_zeta, s_zeta_inv, d_zeta), "W", the b - 1 coefficients of W, "Wp", the b - 1 coefficients of W', one value per line;
//           "remainder" in place of a polynomial whose division left one
//   mercury_host_test self                     -> one fixed case, "mercury host ok" (the form a sanitizer build runs)
// Values are 64 hex digits, most significant first: canonical integers, or Montgomery limbs (x 2^256 mod p) with mont = 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../nova_amd/csrc/mercury_host.hpp"

using namespace nmx;

static bool parse_hex(const char* hex, uint8_t b[32]) {
  if (strlen(hex) != 64) return false;
  memset(b, 0, 32);
  for (int i = 0; i < 64; i++) {
    const char ch = hex[63 - i];
    const uint32_t d = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
    b[i / 2] |= (uint8_t)(d << (4 * (i % 2)));
  }
  return true;
}
static void print_bytes(const uint8_t b[32]) {
  char out[65];
  for (int i = 0; i < 64; i++) out[63 - i] = "0123456789abcdef"[(b[i / 2] >> (4 * (i % 2))) & 15u];
  out[64] = 0;
  printf("%s\n", out);
}
static bool read_values(std::vector<uint8_t>& v, size_t count) {
  v.assign(32 * (count ? count : 1), 0);
  char tok[128];
  for (size_t i = 0; i < count; i++)
    if (scanf("%127s", tok) != 1 || !parse_hex(tok, v.data() + 32 * i)) return false;
  return true;
}

template <int FID> static int open_case(size_t b, bool mont) {
  using O = MercuryOpening<FID>;
  using H = typename O::H;
  std::vector<uint8_t> g, h, s, ch;
  if (!read_values(g, b) || !read_values(h, b) || !read_values(s, b - 1) || !read_values(ch, 4)) return 2;
  auto get = [&](const uint8_t* w) { return mont ? H::from_mont256(w) : H::from_canonical(w); };
  auto put = [&](const H& x) {
    uint8_t w[32];
    if (mont) x.to_mont256(w);
    else x.to_canonical(w);
    print_bytes(w);
  };
  O op;
  if (!op.set_points(get(ch.data()), get(ch.data() + 32))) {
    printf("degenerate\n");
    return 0;
  }
  op.load(g.data(), h.data(), s.data(), b, mont);
  op.eval_all();
  for (const H& e : {op.g_zeta, op.g_zeta_inv, op.h_zeta, op.h_zeta_inv, op.h_alpha, op.s_zeta, op.s_zeta_inv, op.d_zeta}) put(e);
  printf("W\n");
  if (!op.make_w(get(ch.data() + 64))) {
    printf("remainder\n");
    return 0;
  }
  for (const H& e : op.W) put(e);
  printf("Wp\n");
  typename O::Poly wp;
  if (!op.make_w_prime(get(ch.data() + 96), wp)) {
    printf("remainder\n");
    return 0;
  }
  for (const H& e : wp) put(e);
  return 0;
}

// a fixed case over BN254 Fr: b = 4, small coefficients; the divisions leave no remainder and W, W' have b - 1 coefficients; wrong
// evaluations leave one; coinciding points are refused
static int self_test() {
  using O = MercuryOpening<1>;
  using H = O::H;
  O op;
  const size_t b = 4;
  std::vector<uint8_t> g(32 * b, 0), h(32 * b, 0), s(32 * (b - 1), 0);
  for (size_t i = 0; i < b; i++) g[32 * i] = (uint8_t)(3 + i), h[32 * i] = (uint8_t)(11 * i + 1);
  for (size_t i = 0; i + 1 < b; i++) s[32 * i] = (uint8_t)(7 - i);
  if (op.set_points(H::zero(), H::from_u64(5)) || op.set_points(H::one(), H::from_u64(5)) || op.set_points(H::zero() - H::one(), H::from_u64(5)) ||
      op.set_points(H::from_u64(9), H::from_u64(9)) || op.set_points(H::from_u64(9), H::from_u64(9).inv()))
    return 1;
  if (!op.set_points(H::from_u64(9), H::zero())) return 1;  // alpha = 0 is legal
  if (!op.set_points(H::from_u64(9), H::from_u64(5))) return 1;
  op.load(g.data(), h.data(), s.data(), b, false);
  op.eval_all();
  O::Poly wp;
  for (uint64_t beta : {0ull, 1ull, 77ull}) {
    if (!op.make_w(H::from_u64(beta)) || op.W.size() != b - 1) return 1;
    for (const H& z : {H::from_u64(123), H::from_u64(9), H::from_u64(5), H::from_u64(9).inv(), H::zero()})
      if (!op.make_w_prime(z, wp) || wp.size() != b - 1) return 1;
  }
  op.set_evals(op.g_zeta + H::one(), op.g_zeta_inv, op.h_zeta, op.h_zeta_inv, op.h_alpha, op.s_zeta, op.s_zeta_inv, op.d_zeta);
  if (op.make_w(H::from_u64(77))) return 1;  // a wrong evaluation: m(X) does not vanish on T
  printf("mercury host ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "self")) return self_test();
  if (argc == 5 && !strcmp(argv[1], "open")) {
    const size_t b = strtoull(argv[3], nullptr, 10);
    const bool mont = atoi(argv[4]) != 0;
    if (b < 2) return 2;
    switch (atoi(argv[2])) {
      case 0: return open_case<0>(b, mont);
      case 1: return open_case<1>(b, mont);
      case 2: return open_case<2>(b, mont);
      case 3: return open_case<3>(b, mont);
    }
  }
  fprintf(stderr, "usage: mercury_host_test open field_id b mont < values | self\n");
  return 2;
}
