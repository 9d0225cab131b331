// tests/cpp/key_ext_mirror_test.cpp -- nova::provider::CommitmentKey::split_at / combine / concat / fold / scale of include/nova_mi355x.hpp as
// a stand-alone g++ program against the product library.  A CommitmentKey object cannot exist without a device (every constructor registers
// a key), so without one the program checks the wrappers' types and the refusals of the C calls they make, all decided before a device is
// leased; with one it works on a generated key P_i = (1 + i) G and compares points of the results with points of the source (1 * P_0 +
// 1 * P_2 = G + 3G = P_3, 2 * P_1 = 4G = P_3: no oracle needed), and the wrappers' errors as nova::provider::Error with the library's code.
// tests/test_key_ext_abi.py builds and runs it; "key ext mirror ok" and exit 0 on success.
#include <cstdio>
#include <type_traits>
#include <utility>
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
using nova::provider::Scalar;
static_assert(std::is_same<decltype(&CommitmentKey::split_at), std::pair<CommitmentKey, CommitmentKey> (CommitmentKey::*)(size_t) const>::value,
              "CommitmentKey::split_at(size_t) const");
static_assert(std::is_same<decltype(&CommitmentKey::combine), CommitmentKey (CommitmentKey::*)(const CommitmentKey&) const>::value,
              "CommitmentKey::combine(const CommitmentKey&) const");
static_assert(std::is_same<decltype(&CommitmentKey::concat), CommitmentKey (CommitmentKey::*)(const std::vector<CommitmentKey::Part>&, bool) const>::value,
              "CommitmentKey::concat(const std::vector<Part>&, bool) const");
static_assert(std::is_same<decltype(&CommitmentKey::fold), CommitmentKey (CommitmentKey::*)(const Scalar&, const Scalar&, bool, bool) const>::value,
              "CommitmentKey::fold(const Scalar&, const Scalar&, bool, bool) const");
static_assert(std::is_same<decltype(&CommitmentKey::scale), CommitmentKey (CommitmentKey::*)(const Scalar&, bool, bool) const>::value,
              "CommitmentKey::scale(const Scalar&, bool, bool) const");

static Affine point_of(const CommitmentKey& k, size_t i) {
  Affine a{};
  nova::provider::check(nmx_bases_read(k.handle(), i, 1, a.data()));
  return a;
}
static Scalar small(uint8_t v) {
  Scalar s{};
  s[0] = v;
  return s;
}

int main() {
  const uint64_t kSentinel = 0x5eedface0badf00dull;
  uint64_t h = kSentinel;
  const uint64_t hs[2] = {77, 78};
  const size_t lens[2] = {2, 1}, zero[2] = {0, 0}, big[2] = {(size_t)1 << 30, (size_t)1 << 30};
  const Scalar one = small(1);
  // decided on the host, whatever the handles name
  EXPECT(nmx_bases_concat(hs, nullptr, lens, 2, 0, nullptr) == NMX_E_ARG);
  EXPECT(nmx_bases_concat(nullptr, nullptr, lens, 2, 0, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_concat(hs, nullptr, lens, 0, 0, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_concat(hs, nullptr, lens, 9, 0, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_concat(hs, nullptr, zero, 2, 0, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_concat(hs, nullptr, big, 2, 0, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_concat(hs, nullptr, lens, 2, NMX_SCALARS_MONT, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_concat(hs, nullptr, lens, 2, 0, &h) == NMX_E_HANDLE);
  EXPECT(nmx_bases_fold(77, 0, 4, one.data(), one.data(), 0, nullptr) == NMX_E_ARG);
  EXPECT(nmx_bases_fold(77, 0, 4, nullptr, one.data(), 0, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_fold(77, 0, 4, one.data(), nullptr, 0, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_fold(77, 0, 1, one.data(), one.data(), 0, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_fold(77, 0, 4, one.data(), one.data(), NMX_ASYNC, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_fold(77, 0, 4, one.data(), one.data(), NMX_SCALARS_MONT, &h) == NMX_E_HANDLE);
  EXPECT(nmx_bases_scale(77, 0, 4, nullptr, 0, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_scale(77, 0, 0, one.data(), 0, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_scale(77, 0, (size_t)1 << 31, one.data(), 0, &h) == NMX_E_ARG);
  EXPECT(nmx_bases_scale(77, 0, 4, one.data(), NMX_BASES_PRECOMPUTE, &h) == NMX_E_HANDLE);
  EXPECT(h == kSentinel);
  if (nmx_device_count() > 0) {
    CommitmentKey ck = CommitmentKey::generate(NMX_BN254_G1, 8);  // G, 2G, ... 8G and h = 9G: nine registered points
    auto halves = ck.split_at(3);
    const CommitmentKey &lo = halves.first, &hi = halves.second;
    EXPECT(lo.len() == 3 && hi.len() == 5 && lo.h() == ck.h() && hi.curve() == ck.curve() && lo.handle() != ck.handle());
    EXPECT(point_of(lo, 2) == point_of(ck, 2) && point_of(hi, 0) == point_of(ck, 3) && point_of(hi, 4) == point_of(ck, 7));
    CommitmentKey back = lo.combine(hi);
    EXPECT(back.len() == 8);
    for (size_t i = 0; i < 8; i++) EXPECT(point_of(back, i) == point_of(ck, i));
    CommitmentKey pick = ck.concat({{&ck, 4, 2}, {&lo, 0, 1}});  // 5G, 6G, G
    EXPECT(pick.len() == 3 && point_of(pick, 0) == point_of(ck, 4) && point_of(pick, 1) == point_of(ck, 5) && point_of(pick, 2) == point_of(ck, 0));
    CommitmentKey f = ck.fold(one, one);  // (1 + i) G + (5 + i) G = (6 + 2 i) G: 6G, 8G in range of the source
    EXPECT(f.len() == 4 && f.h() == ck.h() && f.mont() == ck.mont());
    EXPECT(point_of(f, 0) == point_of(ck, 5) && point_of(f, 1) == point_of(ck, 7));
    CommitmentKey s = ck.scale(small(2));  // 2 (1 + i) G
    EXPECT(s.len() == 8 && point_of(s, 0) == point_of(ck, 1) && point_of(s, 1) == point_of(ck, 3) && point_of(s, 3) == point_of(ck, 7));
    CommitmentKey z = ck.scale(small(0));  // identities
    EXPECT(point_of(z, 0) == Affine{} && point_of(z, 7) == Affine{});
    CommitmentKey ff = f.fold(one, small(0));  // a fold of a fold: its first half
    EXPECT(ff.len() == 2 && point_of(ff, 0) == point_of(f, 0) && point_of(ff, 1) == point_of(f, 1));
    Scalar ones;
    ones.fill(0xff);
    EXPECT(code_of([&] { ck.scale(ones); }) == NMX_E_SCALAR_RANGE);
    EXPECT(code_of([&] { ck.fold(one, ones); }) == NMX_E_SCALAR_RANGE);
    EXPECT(code_of([&] { ck.concat({{&ck, 8, 2}}); }) == NMX_E_HANDLE);  // one past the nine registered points
    EXPECT(code_of([&] { ck.split_at(9); }) == NMX_E_HANDLE);
    EXPECT(code_of([&] { lo.split_at(0); }) == NMX_E_ARG);  // an empty half is no key
  }
  printf("key ext mirror ok\n");
  return 0;
}
