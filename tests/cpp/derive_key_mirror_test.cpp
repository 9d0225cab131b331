// tests/cpp/derive_key_mirror_test.cpp -- nova::provider::CommitmentKey::derive_by_address and nova::resident::derive_by_address of
// include/nova_mi355x.hpp as a stand-alone g++ program against the product library.  A CommitmentKey object cannot exist without a device
// (every constructor registers a key), so without one the program checks the wrappers' types and the refusals of the C call they make, all
// decided before a device is leased; with one it derives from a generated key P_i = (1 + i) G and compares points of the derived key with
// points of the source (G + 3G = 4G needs no oracle), and the wrappers' errors as nova::provider::Error with the library's code.
// tests/test_derive_key_abi.py builds and runs it; "derive key mirror ok" and exit 0 on success.
#include <cstdio>
#include <type_traits>
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

using nova::provider::Affine;
using nova::provider::CommitmentKey;
static_assert(std::is_same<decltype(&CommitmentKey::derive_by_address),
                           CommitmentKey (CommitmentKey::*)(const uint64_t*, size_t, size_t, bool) const>::value,
              "CommitmentKey::derive_by_address(const uint64_t*, size_t, size_t, bool) const");
static_assert(std::is_same<decltype(&nova::resident::derive_by_address), CommitmentKey (*)(const CommitmentKey&, const uint64_t*, size_t, size_t, bool)>::value,
              "nova::resident::derive_by_address(const CommitmentKey&, const uint64_t*, size_t, size_t, bool)");

static Affine point_of(const CommitmentKey& k, size_t i) {
  Affine a{};
  nova::provider::check(nmx_bases_read(k.handle(), i, 1, a.data()));
  return a;
}

int main() {
  const uint64_t kSentinel = 0x5eedface0badf00dull;
  const uint64_t addr[4] = {0, 1, 0, 2}, bad[4] = {0, 1, 0, 3};
  uint64_t h = kSentinel;
  // decided on the host, whatever the handle names
  EXPECT(nmx_bases_derive_by_address(77, addr, 4, 3, 0, nullptr) == NMX_E_ARG);
  EXPECT(nmx_bases_derive_by_address(77, nullptr, 4, 3, 0, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_derive_by_address(77, addr, 4, 0, 0, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_derive_by_address(77, addr, 4, (size_t)1 << 31, 0, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_derive_by_address(77, addr, 4, 3, NMX_SCALARS_MONT, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_derive_by_address(77, bad, 4, 3, 0, &h) == NMX_E_ARG);
  EXPECT(h == kSentinel);
  if (nmx_device_count() > 0) {
    CommitmentKey ck = CommitmentKey::generate(NMX_BN254_G1, 8);  // G, 2G, ... 8G and h = 9G: nine registered points
    CommitmentKey d = ck.derive_by_address(addr, 4, 3);
    EXPECT(d.len() == 3 && d.curve() == ck.curve() && d.h() == ck.h() && d.mont() == ck.mont() && d.handle() != ck.handle());
    EXPECT(point_of(d, 0) == point_of(ck, 3));  // G + 3G
    EXPECT(point_of(d, 1) == point_of(ck, 1));
    EXPECT(point_of(d, 2) == point_of(ck, 3));
    CommitmentKey e = ck.derive_by_address(addr, 2, 4, false);  // indices 2 and 3 stay empty
    EXPECT(point_of(e, 0) == point_of(ck, 0) && point_of(e, 1) == point_of(ck, 1) && point_of(e, 2) == Affine{} && point_of(e, 3) == Affine{});
    CommitmentKey f = e.derive_by_address(addr, 4, 3);  // from a derived key with identity rows: e[0] + e[2], e[1], e[3]
    EXPECT(point_of(f, 0) == point_of(ck, 0) && point_of(f, 1) == point_of(ck, 1) && point_of(f, 2) == Affine{});
    EXPECT(code_of([&] { ck.derive_by_address(bad, 4, 3); }) == NMX_E_ARG);
    const std::vector<uint64_t> zeros(10, 0);
    EXPECT(code_of([&] { ck.derive_by_address(zeros.data(), 10, 3); }) == NMX_E_HANDLE);  // one more than the nine points
    EXPECT(code_of([&] { ck.derive_by_address(addr, 4, 0); }) == NMX_E_ARG);
  }
  printf("derive key mirror ok\n");
  return 0;
}
