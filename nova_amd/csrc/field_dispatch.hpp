// field_dispatch.hpp -- the one place a run-time field id (NMX_F_*) becomes a template argument, with the error type every layer
// throws.  Plain C++17, no HIP: the g++ builds under tests/ include it as it is.
#pragma once
#include <string>
#include <type_traits>
#include <utility>

#include "../../include/nova_mi355x.h"

namespace nmx {

struct Fail {
  int code;
  std::string msg;
};

// fn(std::integral_constant<int, N>{}) for value == N in Lo .. Hi, returning what fn returns; anything else: NMX_E_ARG with `message`
template <int Lo, int Hi, class Fn> decltype(auto) with_index(int value, const char* message, Fn&& fn) {
  if constexpr (Lo < Hi) {
    if (value != Lo) return with_index<Lo + 1, Hi>(value, message, std::forward<Fn>(fn));
  } else {
    if (value != Lo) throw Fail{NMX_E_ARG, message};
  }
  return fn(std::integral_constant<int, Lo>{});
}

// the four scalar / base fields: with_field(field, [&](auto F) { horner_t<F()>(c, f, n, u, flags, out); });
template <class Fn> decltype(auto) with_field(int field, Fn&& fn) {
  return with_index<0, 3>(field, "bad field id", std::forward<Fn>(fn));
}

}  // namespace nmx
