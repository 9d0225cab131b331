// g++ -std=c++17: nova_amd/csrc/field_dispatch.hpp (with_field / with_index) and spmv_index_mask of spmv_row.hpp on the host; prints
// one line per probe, tests/test_field_dispatch.py asserts on them.
#include <limits.h>
#include <stdio.h>

#include "../../nova_amd/csrc/field_dispatch.hpp"
#include "../../nova_amd/csrc/spmv_row.hpp"

template <int FID> static int tagged(int x) { return 1000 * FID + x; }

int main() {
  for (int field = 0; field < 4; field++) {
    int calls = 0, seen = -1;
    const int ret = nmx::with_field(field, [&](auto F) {
      calls++;
      seen = F();
      return tagged<F()>(7);
    });
    int side = 0;
    nmx::with_field(field, [&](auto F) { side = tagged<F()>(1); });  // a lambda that returns nothing
    printf("field=%d seen=%d ret=%d calls=%d side=%d\n", field, seen, ret, calls, side);
  }
  const int bad[3] = {-1, 4, INT_MAX};
  for (int field : bad) {
    int calls = 0;
    try {
      (void)nmx::with_field(field, [&](auto F) {
        calls++;
        return (int)F();
      });
      printf("bad=%d threw=0 calls=%d\n", field, calls);
    } catch (const nmx::Fail& f) {
      printf("bad=%d threw=1 calls=%d code=%d msg=%s\n", field, calls, f.code, f.msg.c_str());
    }
  }
  for (int mode = 0; mode <= 4; mode++) {  // the nested form: its own range and its own message
    try {
      const int got = nmx::with_index<1, 3>(mode, "bad sum-check mode", [&](auto M) { return tagged<M()>(0); });
      printf("mode=%d threw=0 ret=%d\n", mode, got);
    } catch (const nmx::Fail& f) {
      printf("mode=%d threw=1 code=%d msg=%s\n", mode, f.code, f.msg.c_str());
    }
  }
  const size_t extents[3] = {1, (size_t)1 << 28, ((size_t)1 << 28) + 1};
  for (size_t ext : extents) printf("extent=%zu mask=%u\n", ext, nmx::spmv_index_mask(ext));
  printf("e_arg=%d\n", (int)NMX_E_ARG);
  return 0;
}
