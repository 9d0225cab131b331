// tests/cpp/fixed_base_mirror_test.cpp -- nova::provider::CommitmentKey::from_scalars / setup_from_tau of include/nova_mi355x.hpp as a
// stand-alone g++ program against the product library.  Everything here is decided before a device is leased, so the program runs the same
// with and without a GPU: the wrappers' refusals as nova::provider::Error with the library's code, and that a well-formed call is stopped
// by nothing but the missing device.  tests/test_fixed_base_abi.py builds and runs it; "fixed base mirror ok" and exit 0 on success.
#include <cstdio>
#include <vector>

#include "../../include/nova_mi355x.hpp"

#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

template <class Fn> static int code_of(Fn&& fn) {
  try {
    fn();
  } catch (const nova::provider::Error& e) {
    return e.code;
  }
  return NMX_OK;
}

int main() {
  using namespace nova::provider;
  Scalar three{}, ones;
  three[0] = 3;
  ones.fill(0xff);
  const Affine h{};
  Affine g{}, off{};  // BN254 G1: G = (1, 2); (1, 3) is not on the curve
  g[0] = 1, g[32] = 2;
  off[0] = 1, off[32] = 3;
  const std::vector<Scalar> good{three, three}, high{three, ones}, none;
  const int curve = NMX_BN254_G1;
  EXPECT(code_of([&] { CommitmentKey::from_scalars(curve, none, nullptr, h); }) == NMX_E_ARG);                 // n == 0
  EXPECT(code_of([&] { CommitmentKey::from_scalars(9, good, nullptr, h); }) == NMX_E_ARG);                     // unknown curve
  EXPECT(code_of([&] { CommitmentKey::from_scalars(curve, high, nullptr, h); }) == NMX_E_SCALAR_RANGE);
  EXPECT(code_of([&] { CommitmentKey::from_scalars(curve, high, nullptr, h, true); }) == NMX_E_SCALAR_RANGE);  // Montgomery words are range-checked too
  EXPECT(code_of([&] { CommitmentKey::from_scalars(curve, good, &off, h); }) == NMX_E_POINT);
  EXPECT(code_of([&] { CommitmentKey::from_scalars(curve, good, &h, h); }) == NMX_E_POINT);                    // the identity as the base
  EXPECT(code_of([&] { CommitmentKey::from_scalars(curve, good, &g, h, true); }) == NMX_E_POINT);              // canonical bytes named Montgomery
  EXPECT(code_of([&] { CommitmentKey::setup_from_tau(9, 4, three, h); }) == NMX_E_ARG);
  EXPECT(code_of([&] { CommitmentKey::setup_from_tau(curve, 4, ones, h); }) == NMX_E_SCALAR_RANGE);
  EXPECT(code_of([&] { CommitmentKey::setup_from_tau(curve, (size_t)1 << 31, three, h); }) == NMX_E_ARG);      // n >= 2^31
  if (nmx_device_count() <= 0) {
    EXPECT(code_of([&] { CommitmentKey::from_scalars(curve, good, &g, h); }) == NMX_E_NO_DEVICE);
    EXPECT(code_of([&] { CommitmentKey::setup_from_tau(curve, 3, three, h); }) == NMX_E_NO_DEVICE);
    EXPECT(code_of([&] { CommitmentKey::setup_from_tau(curve, 0, three, h, true, false); }) == NMX_E_NO_DEVICE);  // n = 0 rounds to 1, as next_power_of_two does
  }
  printf("fixed base mirror ok\n");
  return 0;
}
