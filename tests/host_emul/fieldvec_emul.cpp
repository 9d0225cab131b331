// tests/host_emul/fieldvec_emul.cpp -- TEST-ONLY: the map functors of the dense field-vector calls (nova_amd/csrc/fieldvec_maps.hpp) and
// the lane bodies of the three sum passes (nova_amd/csrc/sumcheck_sums.hpp) on the CPU, lane by lane, limb bounds asserted
// (NMX_DEBUG_BOUNDS).  The challenge-derived constants (r 2^261, p - u, 2^522 or 2^266, nk) arrive as canonical residues made by the test
// with big integers (tests/test_fieldvec_edges.py), so the host half of a call is not trusted here.  The sum passes hand back every
// lane's canonical sums; the test compares each with the big-integer sum over that lane's indices.  NOT emulated: the block reductions
// (block_sum, block_sum_waves), k_sum_partials_n, the staging of host operands, the host-side form constants and k_fold_chain's LDS
// hand-over -- those run in tests/test_gpu_fieldvec_edges.py only.
#include <stdint.h>

#include <type_traits>

#include "../../nova_amd/csrc/fieldvec_maps.hpp"
#include "../../nova_amd/csrc/sumcheck_sums.hpp"

using namespace nmx;

namespace {
template <int FID> Fp<FID> W(const uint32_t* w) { return w ? Fp<FID>::from_words(w) : Fp<FID>::zero(); }

template <class Fn> void each(const Fn& f, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) f(i);
}

// op: 0 axpy, 1 axpy2, 2 cross_term, 3 cross_term2, 4 vec_add, 5 bind (in[0] = lo, in[1] = hi, aux = stride), 6 fold_pair (in = w1, w2, e1, t;
// aux = n_w; out = w, out2 = e)
template <int FID>
int run_map(int op, const uint32_t* const* in, const uint32_t* c0, const uint32_t* c1, uint32_t n, uint32_t aux, uint32_t* out, uint32_t* out2) {
  switch (op) {
    case 0: each(AxpyFn<FID>{in[0], in[1], out, W<FID>(c0)}, n); break;
    case 1: each(Axpy2Fn<FID>{in[0], in[1], in[2], out, W<FID>(c0), W<FID>(c1)}, n); break;
    case 2: each(CrossTermFn<FID>{in[0], in[1], in[2], in[3], out, W<FID>(c0), W<FID>(c1)}, n); break;
    case 3: each(CrossTerm2Fn<FID>{in[0], in[1], in[2], in[3], in[4], out, W<FID>(c0), W<FID>(c1)}, n); break;
    case 4: each(VecAddFn<FID>{in[0], in[1], out}, n); break;
    case 5: each(BindTopFn<FID>{in[0], in[1], out, W<FID>(c0), aux}, n); break;
    case 6: each(FoldPairFn<FID>{in[0], in[1], in[2], in[3], out, out2, aux, W<FID>(c0)}, n); break;
    default: return -1;
  }
  return 0;
}

template <int FID, int MODE>
void run_eq(const uint32_t* A, const uint32_t* B, const uint32_t* C, const uint32_t* eqL, const uint32_t* eqR, uint32_t shift, uint32_t h,
            const uint32_t* nk, uint32_t grid, int rows, uint32_t* lane_sums) {
  const Fp<FID> k = W<FID>(nk);
  const uint32_t mask = shift >= 32 ? 0xffffffffu : ((1u << shift) - 1u);
  for (uint32_t b = 0; b < grid; b++)
    for (uint32_t t = 0; t < 256; t++) {
      Fp<FID> s0, s1;
      if (rows) eq_rows_lane<FID, MODE>(A, B, C, eqL, eqR, shift, h, k, t, b, grid, s0, s1);
      else eq_sums_lane<FID, MODE>(A, B, C, eqL, eqR, shift, mask, h, k, b * 256u + t, grid * 256u, s0, s1);
      s0.to_words(lane_sums + 16 * (size_t)(b * 256u + t));
      s1.to_words(lane_sums + 16 * (size_t)(b * 256u + t) + 8);
    }
}
template <int FID, int MODE>
void run_bind(const uint32_t* A, const uint32_t* B, const uint32_t* C, uint32_t* oA, uint32_t* oB, uint32_t* oC, const uint32_t* r,
              const uint32_t* eqL, const uint32_t* eqR, uint32_t shift, uint32_t hq, const uint32_t* nk, uint32_t grid, uint32_t* lane_sums) {
  const Fp<FID> k = W<FID>(nk), ri = W<FID>(r);
  const uint32_t mask = shift >= 32 ? 0xffffffffu : ((1u << shift) - 1u);
  for (uint32_t l = 0; l < grid * 256u; l++) {
    Fp<FID> s0, s1;
    bind_eq_sums_lane<FID, MODE>(A, B, C, oA, oB, oC, ri, eqL, eqR, shift, mask, hq, k, l, grid * 256u, s0, s1);
    s0.to_words(lane_sums + 16 * (size_t)l);
    s1.to_words(lane_sums + 16 * (size_t)l + 8);
  }
}
template <int FID, int KIND>
void run_plain(const uint32_t* A, const uint32_t* B, const uint32_t* C, uint32_t h, uint32_t grid, uint32_t* lane_sums) {
  for (uint32_t l = 0; l < grid * 256u; l++) {
    Fp<FID> s0, s1, s2;
    plain_sums_lane<FID, KIND>(A, B, C, h, l, grid * 256u, s0, s1, s2);
    s0.to_words(lane_sums + 24 * (size_t)l);
    s1.to_words(lane_sums + 24 * (size_t)l + 8);
    s2.to_words(lane_sums + 24 * (size_t)l + 16);
  }
}

template <class Fn> int with_fid(int fid, Fn&& fn) {
  switch (fid) {
    case 0: return fn(std::integral_constant<int, 0>{});
    case 1: return fn(std::integral_constant<int, 1>{});
    case 2: return fn(std::integral_constant<int, 2>{});
    case 3: return fn(std::integral_constant<int, 3>{});
    default: return -1;
  }
}
template <int LO, int HI, class Fn> int with_int(int v, Fn&& fn) {
  if constexpr (LO > HI) {
    return -1;
  } else {
    if (v == LO) return fn(std::integral_constant<int, LO>{});
    return with_int<LO + 1, HI>(v, fn);
  }
}
}  // namespace

// every vector 8 words per element; c0, c1: 8 words each (canonical residues) or null
extern "C" int emul_fv_map(int fid, int op, const uint32_t* const* in, const uint32_t* c0, const uint32_t* c1, uint32_t n, uint32_t aux,
                           uint32_t* out, uint32_t* out2) {
  return with_fid(fid, [&](auto F) { return run_map<F()>(op, in, c0, c1, n, aux, out, out2); });
}

// vecs: k host addresses; lens: k element counts; w: k x 8 words (s^j 2^261 mod p)
extern "C" int emul_fv_lincomb(int fid, const uint64_t* vecs, const uint64_t* lens, const uint32_t* w, uint32_t k, uint32_t n, uint32_t* out) {
  return with_fid(fid, [&](auto F) {
    each(LinCombFn<F()>{vecs, lens, w, out, k}, n);
    return 0;
  });
}

// lane_sums: grid x 256 x 2 elements.  rows != 0: k_eq_rows' body (eqL required, shift < 31), else k_eq_sums'
extern "C" int emul_eq_sums(int fid, int mode, const uint32_t* A, const uint32_t* B, const uint32_t* C, const uint32_t* eqL, const uint32_t* eqR,
                            uint32_t shift, uint32_t h, const uint32_t* nk, uint32_t grid, int rows, uint32_t* lane_sums) {
  if (grid < 1 || (rows && (!eqL || shift >= 31))) return -1;
  return with_fid(fid, [&](auto F) {
    return with_int<1, 3>(mode, [&](auto M) {
      run_eq<F(), M()>(A, B, C, eqL, eqR, shift, h, nk, grid, rows, lane_sums);
      return 0;
    });
  });
}

extern "C" int emul_bind_eq_sums(int fid, int mode, const uint32_t* A, const uint32_t* B, const uint32_t* C, uint32_t* oA, uint32_t* oB, uint32_t* oC,
                                 const uint32_t* r, const uint32_t* eqL, const uint32_t* eqR, uint32_t shift, uint32_t hq, const uint32_t* nk,
                                 uint32_t grid, uint32_t* lane_sums) {
  if (grid < 1) return -1;
  return with_fid(fid, [&](auto F) {
    return with_int<1, 3>(mode, [&](auto M) {
      run_bind<F(), M()>(A, B, C, oA, oB, oC, r, eqL, eqR, shift, hq, nk, grid, lane_sums);
      return 0;
    });
  });
}

// lane_sums: grid x 256 x 3 elements
extern "C" int emul_plain_sums(int fid, int kind, const uint32_t* A, const uint32_t* B, const uint32_t* C, uint32_t h, uint32_t grid,
                               uint32_t* lane_sums) {
  if (grid < 1) return -1;
  return with_fid(fid, [&](auto F) {
    return with_int<1, 4>(kind, [&](auto K) {
      run_plain<F(), K()>(A, B, C, h, grid, lane_sums);
      return 0;
    });
  });
}
