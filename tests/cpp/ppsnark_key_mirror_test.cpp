// tests/cpp/ppsnark_key_mirror_test.cpp -- nova::resident::ppsnark_spark_size / ppsnark_spark_repr / masked_eq_evals of include/nova_mi355x.hpp
// as a stand-alone g++ program against the product library.  Everything here is decided before a device is leased, so the program runs the
// same with and without a GPU: the size formula (src/spartan/ppsnark.rs:118-121 of the reference), and the wrappers' refusals as nova::Error
// with the library's code.  tests/test_ppsnark_key_abi.py builds and runs it; "ppsnark key mirror ok" and exit 0 on success.
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
  } catch (const std::invalid_argument&) {
    return -1000;
  }
  return NMX_OK;
}

int main() {
  using namespace nova;
  EXPECT(resident::ppsnark_spark_size({0, 0, 0}, 0, 0) == 1);
  EXPECT(resident::ppsnark_spark_size({192, 192, 192}, 64, 64) == 1024);
  EXPECT(resident::ppsnark_spark_size({64, 64, 64}, 128, 64) == 256);
  EXPECT(resident::ppsnark_spark_size({100, 100, 56}, 64, 64) == 256);
  EXPECT(resident::ppsnark_spark_size({100, 100, 57}, 64, 64) == 512);
  EXPECT(resident::ppsnark_spark_size({5}, 1, 1000) == 1024);
  // the wrapper passes NMX_SCALARS_DEVICE; none of these calls reaches a device or touches its (bogus, never dereferenced) pointers
  std::vector<uint8_t> buf(8 * 4 * 32);
  auto at = [&](size_t j) { return (void*)(buf.data() + 32 * 4 * j); };
  const std::vector<uint64_t> unknown{(1ull << 62) + 1, (1ull << 62) + 2, (1ull << 62) + 3};
  EXPECT(code_of([&] { resident::ppsnark_spark_repr(unknown, 4, at(0), at(1), {at(2), at(3), at(4)}, at(5), at(6)); }) == NMX_E_HANDLE);
  EXPECT(code_of([&] { resident::ppsnark_spark_repr(unknown, 4, nullptr, nullptr, {}, nullptr, at(6), true); }) == NMX_E_HANDLE);
  EXPECT(code_of([&] { resident::ppsnark_spark_repr(unknown, 6, at(0), at(1), {}, at(5), at(6)); }) == NMX_E_ARG);          // no power of two
  EXPECT(code_of([&] { resident::ppsnark_spark_repr(unknown, 4, at(0), at(0), {}, at(5), at(6)); }) == NMX_E_ARG);          // row and col overlap
  EXPECT(code_of([&] { resident::ppsnark_spark_repr({}, 4, at(0), at(1), {}, at(5), at(6)); }) == NMX_E_ARG);               // k == 0
  EXPECT(code_of([&] { resident::ppsnark_spark_repr(unknown, 4, at(0), at(1), {at(2)}, at(5), at(6)); }) == -1000);         // one value vector for three matrices
  nova::provider::Scalar three{};
  three[0] = 3;
  nova::provider::Scalar ones;
  ones.fill(0xff);
  const std::vector<nova::provider::Scalar> good{three, three}, high{three, ones};
  EXPECT(code_of([&] { resident::masked_eq_evals(NMX_F_BN254_FR, good, 3, at(0)); }) == NMX_E_ARG);                // num_masked_vars > ell
  EXPECT(code_of([&] { resident::masked_eq_evals(NMX_F_BN254_FR, high, 1, at(0)); }) == NMX_E_SCALAR_RANGE);
  EXPECT(code_of([&] { resident::masked_eq_evals(9, good, 1, at(0)); }) == NMX_E_ARG);
  for (uint8_t b : buf) EXPECT(b == 0);
  printf("ppsnark key mirror ok\n");
  return 0;
}
