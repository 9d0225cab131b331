// tests/host_emul/eval_emul.cpp -- TEST-ONLY: the functors of the eq tables, the two passes of batch_invert and the lane body of
// k_eval_multi (nova_amd/csrc/fieldvec_eval.hpp) on the CPU, lane by lane, limb bounds asserted (NMX_DEBUG_BOUNDS).  Every constant a
// call derives on the host (r 2^261, (1 - r) 2^261, ONE in the vectors' form, the internal ONE of the split form's left table, the
// chunk inverses of batch_invert's upper level, the points and power tables of the evaluation) arrives as a canonical residue made by
// the test with big integers (tests/test_eval_edges.py), so the host half of a call is not trusted here.  NOT emulated: k_launch's
// bounds, the choice of form by ell, the staging, block_sum and the pw4096 loop of k_eval_multi, k_eval_finish, the host level of
// batch_invert, k_sc_small / k_eq_rows of the evaluations -- those run in tests/test_gpu_eval_edges.py only.
#include <stdint.h>

#include <type_traits>

#include "../../nova_amd/csrc/fieldvec_eval.hpp"

using namespace nmx;

namespace {
template <int FID> Fp<FID> W(const uint32_t* w) { return Fp<FID>::from_words(w); }

template <class Fn> void each(const Fn& f, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) f(i);
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

// r, nr: count x 8 words; unused entries zero, as the library leaves them
template <int FID, uint32_t CAP> void fill(Fp<FID> (&r)[CAP], Fp<FID> (&nr)[CAP], const uint32_t* rw, const uint32_t* nrw, uint32_t count) {
  for (uint32_t i = 0; i < CAP; i++) r[i] = nr[i] = Fp<FID>::zero();
  for (uint32_t i = 0; i < count; i++) r[i] = W<FID>(rw + 8 * i), nr[i] = W<FID>(nrw + 8 * i);
}
}  // namespace

// EqDirectFn: out = 2^ell elements
extern "C" int emul_eq_direct(int fid, uint32_t ell, const uint32_t* r, const uint32_t* nr, const uint32_t* one, uint32_t* out) {
  return with_fid(fid, [&](auto F) {
    constexpr int FID = decltype(F)::value;
    if (ell > EqDirectFn<FID>::kMaxEll) return -1;
    EqDirectFn<FID> f;
    f.out = out, f.ell = ell, f.one = W<FID>(one);
    fill<FID>(f.r, f.nr, r, nr, ell);
    each(f, 1u << ell);
    return 0;
  });
}

// EqDirect2Fn: r, nr hold the ellL left challenges, then the ellR right ones
extern "C" int emul_eq_direct2(int fid, uint32_t ellL, uint32_t ellR, const uint32_t* r, const uint32_t* nr, const uint32_t* one, uint32_t* outL,
                               uint32_t* outR) {
  return with_fid(fid, [&](auto F) {
    constexpr int FID = decltype(F)::value;
    if (ellL > EqDirectFn<FID>::kMaxEll || ellR > EqDirectFn<FID>::kMaxEll) return -1;
    EqDirect2Fn<FID> f;
    f.outL = outL, f.outR = outR, f.ellL = ellL, f.ellR = ellR, f.one = W<FID>(one);
    fill<FID>(f.r, f.nr, r, nr, ellL + ellR);
    each(f, (1u << ellL) + (1u << ellR));
    return 0;
  });
}

// EqSplit2Fn, then EqProductFn over the two tables it left: out = 2^(ellL + ellR) elements
extern "C" int emul_eq_split(int fid, uint32_t ellL, uint32_t ellR, const uint32_t* r, const uint32_t* nr, const uint32_t* oneL, const uint32_t* oneR,
                             uint32_t* outL, uint32_t* outR, uint32_t* out) {
  return with_fid(fid, [&](auto F) {
    constexpr int FID = decltype(F)::value;
    if (ellL > EqDirectFn<FID>::kMaxEll || ellR > EqDirectFn<FID>::kMaxEll) return -1;
    EqSplit2Fn<FID> f;
    f.outL = outL, f.outR = outR, f.ellL = ellL, f.ellR = ellR, f.oneL = W<FID>(oneL), f.oneR = W<FID>(oneR);
    fill<FID>(f.r, f.nr, r, nr, ellL + ellR);
    each(f, (1u << ellL) + (1u << ellR));
    each(EqProductFn<FID>{outL, outR, out, ellR, (1u << ellR) - 1u}, 1u << (ellL + ellR));
    return 0;
  });
}

// EqStepFn chained as eq_evals_t chains it: buf[0] = one, then one doubling step per challenge, the LAST challenge first
extern "C" int emul_eq_steps(int fid, uint32_t ell, const uint32_t* r, const uint32_t* one, uint32_t* buf) {
  return with_fid(fid, [&](auto F) {
    constexpr int FID = decltype(F)::value;
    for (int j = 0; j < 8; j++) buf[j] = one[j];
    uint32_t size = 1;
    for (int j = (int)ell - 1; j >= 0; j--) {
      each(EqStepFn<FID>{buf, W<FID>(r + 8 * j), size}, size);
      size *= 2;
    }
    return 0;
  });
}

// one level of batch_invert: T lanes, lane c owns {c, c + T, ...} below n, at most K of them
extern "C" int emul_binv_fwd(int fid, const uint32_t* v, uint32_t n, uint32_t T, uint32_t K, uint32_t* prefix, uint32_t* chunk_prod) {
  return with_fid(fid, [&](auto F) {
    each(BatchInvFwdFn<decltype(F)::value>{v, prefix, chunk_prod, n, T, K}, T);
    return 0;
  });
}
extern "C" int emul_binv_bwd(int fid, const uint32_t* v, const uint32_t* chunk_inv, uint32_t* prefix, uint32_t n, uint32_t T, uint32_t K) {
  return with_fid(fid, [&](auto F) {
    each(BatchInvBwdFn<decltype(F)::value>{v, chunk_inv, prefix, n, T, K}, T);
    return 0;
  });
}

// eval_multi_lane for lane t of a block: out = m x 8 words
extern "C" int emul_eval_lane(int fid, const uint32_t* f, uint32_t lo, uint32_t hi, uint32_t m, const uint32_t* pts, const uint32_t* pw16, uint32_t t,
                              uint32_t* out) {
  return with_fid(fid, [&](auto F) {
    constexpr int FID = decltype(F)::value;
    if (m > kEvalMaxPts || t >= 256 || hi - lo > kEvalChunk) return -1;
    Fp<FID> h[kEvalMaxPts];
    for (uint32_t j = 0; j < kEvalMaxPts; j++) h[j] = Fp<FID>::zero();
    eval_multi_lane<FID>(f, lo, hi, m, pts, pw16, t, h);
    for (uint32_t j = 0; j < m; j++) h[j].to_words(out + 8 * j);
    return 0;
  });
}
