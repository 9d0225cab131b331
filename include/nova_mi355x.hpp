// nova_mi355x.hpp -- header-only C++ host mirror of the reference's provider interface for the commitment / MSM
// path, on top of the C ABI (nova_mi355x.h).  Same names, argument meaning and error behaviour as the reference:
//   DlogGroupExt            /root/reference/src/provider/traits.rs:77-117
//   CommitmentEngineTrait   /root/reference/src/traits/commitment.rs:52-195
//   Pedersen / HyperKZG CE  /root/reference/src/provider/pedersen.rs:240-305, src/provider/hyperkzg.rs:584-645
// No group arithmetic here: every operation is a call into libnova_mi355x.so.  Precondition violations that are
// `assert!` panics in the reference throw std::invalid_argument; library errors throw nova::provider::Error.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "nova_mi355x.h"

namespace nova {
namespace provider {

using Scalar = std::array<uint8_t, 32>;  // canonical little-endian (`to_repr()`), or raw Montgomery with mont = true
using Affine = std::array<uint8_t, 64>;  // x || y, identity = all zero (`to_coordinates()`, traits.rs:303-312)

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error("nmx error " + std::to_string(c) + ": " + m), code(c) {}
};
inline void check(int rc) {
  if (rc != NMX_OK) throw Error(rc, nmx_last_error());
}

// One host process, k GPUs (nmx_init_devices): keys of >= 2^20 points registered afterwards are sharded over the devices by
// the library; every MSM / commit below stays one synchronous call (the reference decomposes in-process too:
// /root/reference/src/provider/msm.rs:564-574).  Returns the number of devices in use.  count = 0: all visible GPUs.
inline int init_devices(int count = 0, bool oversubscribe = false) {
  check(nmx_init_devices(count, oversubscribe ? NMX_DEVICES_OVERSUBSCRIBE : 0u));
  return nmx_devices_in_use();
}

struct Point {  // result of an MSM / commit, as `to_coordinates()` returns it
  Affine xy{};
  bool is_inf = true;
  bool operator==(const Point& o) const { return xy == o.xy && is_inf == o.is_inf; }
};

// A commitment key resident in HBM (`CommitmentKey { ck, h }`, pedersen.rs:33-45 / hyperkzg.rs:84-100).
class CommitmentKey {
 public:
  CommitmentKey(int curve, const std::vector<Affine>& ck, const Affine& h, bool mont = false, bool precompute = true)
      : curve_(curve), n_(ck.size()), h_(h), mont_(mont) {
    uint32_t flags = (mont ? NMX_BASES_MONT : 0u) | (precompute ? NMX_BASES_PRECOMPUTE : 0u);
    check(nmx_bases_register(curve, ck.data(), ck.size(), flags, &handle_));
  }
  // `CommitmentEngineTrait::load_setup` (src/traits/commitment.rs:64-76).  HyperKZG (hyperkzg.rs:658-674): the first
  // n.next_power_of_two() tauG1 points of a .ptau file; `h` is derived from the label on the reference side and tau_H
  // (G2) stays with the host, so the caller supplies h.  Pedersen (pedersen.rs:318-340): "PEDERSEN_KEY" | h | ck.
  // The G1 points are validated as `read_points` does (ptau.rs:372-391: canonical coordinates, on the curve); errors throw
  // Error with NMX_E_IO / _FORMAT / _POINT.  The two G2 points of section 3 (tau_H) are NOT read or validated here: pairings
  // are outside this library, the caller that needs tau_H reads and checks it as the reference does.
  static CommitmentKey load_ptau(int curve, const std::string& path, size_t n, const Affine& h, bool precompute = true) {
    CommitmentKey k(curve, next_power_of_two(n), h);
    check(nmx_bases_register_ptau(curve, path.c_str(), k.n_, 2, precompute ? NMX_BASES_PRECOMPUTE : 0u, &k.handle_));
    return k;
  }
  static CommitmentKey load_keyfile(int curve, const std::string& path, size_t n, bool precompute = true) {
    CommitmentKey k(curve, next_power_of_two(n), Affine{});
    check(nmx_bases_register_keyfile(curve, path.c_str(), k.n_, precompute ? NMX_BASES_PRECOMPUTE : 0u, &k.handle_,
                                     k.h_.data()));
    return k;
  }
  // synthetic key P_i = (k0 + i) G built on the device, h = P_n (benchmarks and replays: nmx_bases_generate)
  static CommitmentKey generate(int curve, size_t n, uint64_t k0 = 1, bool precompute = true) {
    CommitmentKey k(curve, n, Affine{});
    check(nmx_bases_generate(curve, k0, n + 1, precompute ? NMX_BASES_PRECOMPUTE : 0u, &k.handle_));
    check(nmx_bases_read(k.handle_, n, 1, k.h_.data()));
    return k;
  }
  // key[i] = scalars[i] * base made in HBM (nmx_bases_from_scalars); base == nullptr: the curve's generator.  mont names the form of the
  // scalars, of *base and of h.
  static CommitmentKey from_scalars(int curve, const std::vector<Scalar>& scalars, const Affine* base, const Affine& h, bool mont = false,
                                    bool precompute = true) {
    CommitmentKey k(curve, scalars.size(), h);
    k.mont_ = mont;
    const uint32_t flags = (mont ? (NMX_SCALARS_MONT | NMX_BASES_MONT) : 0u) | (precompute ? NMX_BASES_PRECOMPUTE : 0u);
    check(nmx_bases_from_scalars(curve, base ? base->data() : nullptr, scalars.data(), scalars.size(), flags, &k.handle_));
    return k;
  }
  // HyperKZG's key from a known tau (CommitmentKey::setup_from_rng, hyperkzg.rs:357-410): ck[i] = tau^i * G for n.next_power_of_two()
  // points made in HBM (nmx_bases_setup_from_tau).  h (from_label) and tau_H (G2) stay the caller's.
  static CommitmentKey setup_from_tau(int curve, size_t n, const Scalar& tau, const Affine& h, bool mont = false, bool precompute = true) {
    CommitmentKey k(curve, next_power_of_two(n), h);
    k.mont_ = mont;
    const uint32_t flags = (mont ? NMX_SCALARS_MONT : 0u) | (precompute ? NMX_BASES_PRECOMPUTE : 0u);
    check(nmx_bases_setup_from_tau(curve, tau.data(), k.n_, flags, &k.handle_));
    return k;
  }
  // `ck_derive_by_address` (src/traits/commitment.rs:177-194; pedersen.rs:360-381, hyperkzg.rs:731-749), in HBM
  // (nmx_bases_derive_by_address): derived[j] = sum of ck[i] over i < n with addresses[i] == j, the identity where nothing matches.
  // addresses: host.  The result keeps this key's h and mont, as the reference keeps h.  InvalidIndex -> Error(NMX_E_ARG),
  // InvalidCommitmentKeyLength -> Error(NMX_E_HANDLE).
  CommitmentKey derive_by_address(const uint64_t* addresses, size_t n, size_t table_size, bool precompute = true) const {
    return derive(addresses, n, table_size, precompute ? NMX_BASES_PRECOMPUTE : 0u);
  }
  // the same with `addresses` in HBM (nova::resident::derive_by_address)
  CommitmentKey derive_by_device_address(const uint64_t* d_addresses, size_t n, size_t table_size, bool precompute = true) const {
    return derive(d_addresses, n, table_size, NMX_SCALARS_DEVICE | (precompute ? NMX_BASES_PRECOMPUTE : 0u));
  }
  // `CommitmentKeyExtTrait` (src/provider/pedersen.rs:430-529), in HBM (nmx_bases_concat / _fold / _scale).  Every result keeps this key's
  // h and mont, as the reference keeps h; the default is NO window tables: a folded key is used for two MSMs and folded again.
  // (reinterpret_commitments_as_ck, pedersen.rs:515-528, is the registering constructor over the commitments' coordinates.)
  struct Part {  // rows [offset, offset + len) of *key
    const CommitmentKey* key;
    size_t offset, len;
  };
  // the rows of 1 to 8 parts, copied device to device; h and mont come from this key, which need not be among the parts
  CommitmentKey concat(const std::vector<Part>& parts, bool precompute = false) const {
    std::vector<uint64_t> hs;
    std::vector<size_t> offs, lens;
    size_t total = 0;
    for (const Part& p : parts) {
      hs.push_back(p.key->handle_), offs.push_back(p.offset), lens.push_back(p.len);
      total += p.len;
    }
    CommitmentKey k(curve_, total, h_);
    k.mont_ = mont_;
    check(nmx_bases_concat(hs.data(), offs.data(), lens.data(), parts.size(), precompute ? NMX_BASES_PRECOMPUTE : 0u, &k.handle_));
    return k;
  }
  // `split_at` (pedersen.rs:461-472): (ck[..n], ck[n..]), two keys of their own
  std::pair<CommitmentKey, CommitmentKey> split_at(size_t n) const {
    if (n > n_) throw Error(NMX_E_HANDLE, "split_at: n beyond the key");
    return {concat({Part{this, 0, n}}), concat({Part{this, n, n_ - n}})};
  }
  // `combine` (pedersen.rs:474-481): this key's points, then other's
  CommitmentKey combine(const CommitmentKey& other) const { return concat({Part{this, 0, n_}, Part{&other, 0, other.n_}}); }
  // `fold` (pedersen.rs:484-497): with h = len() / 2, out[i] = w1 * ck[i] + w2 * ck[h + i]; for an odd length the last point is ignored.
  // mont names the form of w1 and w2.
  CommitmentKey fold(const Scalar& w1, const Scalar& w2, bool mont = false, bool precompute = false) const {
    CommitmentKey k(curve_, n_ / 2, h_);
    k.mont_ = mont_;
    const uint32_t flags = (mont ? NMX_SCALARS_MONT : 0u) | (precompute ? NMX_BASES_PRECOMPUTE : 0u);
    check(nmx_bases_fold(handle_, 0, n_, w1.data(), w2.data(), flags, &k.handle_));
    return k;
  }
  // `scale` (pedersen.rs:500-512): out[i] = r * ck[i].  mont names the form of r.
  CommitmentKey scale(const Scalar& r, bool mont = false, bool precompute = false) const {
    CommitmentKey k(curve_, n_, h_);
    k.mont_ = mont_;
    const uint32_t flags = (mont ? NMX_SCALARS_MONT : 0u) | (precompute ? NMX_BASES_PRECOMPUTE : 0u);
    check(nmx_bases_scale(handle_, 0, n_, r.data(), flags, &k.handle_));
    return k;
  }
  CommitmentKey(CommitmentKey&& o) noexcept : curve_(o.curve_), n_(o.n_), h_(o.h_), mont_(o.mont_), handle_(o.handle_) {
    o.handle_ = 0;
  }
  CommitmentKey(const CommitmentKey&) = delete;
  CommitmentKey& operator=(const CommitmentKey&) = delete;
  ~CommitmentKey() {
    if (handle_) nmx_bases_unregister(handle_);
  }
  size_t len() const { return n_; }
  int curve() const { return curve_; }
  uint64_t handle() const { return handle_; }
  const Affine& h() const { return h_; }
  bool mont() const { return mont_; }

 private:
  CommitmentKey(int curve, size_t n, const Affine& h) : curve_(curve), n_(n), h_(h), mont_(false) {}
  CommitmentKey derive(const uint64_t* addresses, size_t n, size_t table_size, uint32_t flags) const {
    CommitmentKey k(curve_, table_size, h_);
    k.mont_ = mont_;
    check(nmx_bases_derive_by_address(handle_, addresses, n, table_size, flags, &k.handle_));
    return k;
  }
  static size_t next_power_of_two(size_t n) {
    size_t p = 1;
    while (p < n) p <<= 1;
    return p;
  }
  int curve_;
  size_t n_;
  Affine h_;
  bool mont_;
  uint64_t handle_ = 0;
};

// `DlogGroupExt` for one curve id (NMX_BN254_G1 / NMX_GRUMPKIN / NMX_PALLAS / NMX_VESTA).
template <int CURVE> struct DlogGroupExt {
  // Smallest n worth sending to the GPU; below it the shim keeps the CPU msm() (pedersen.rs:484-497, msm.rs:233)
  static size_t min_gpu_n() { return nmx_min_gpu_n(CURVE); }
  // traits.rs:79 == msm() (msm.rs:225): assert_eq!(coeffs.len(), bases.len()).  Slice form: the library's slice cache
  // keeps `bases` resident (window tables included) keyed by bases.data(); a prefix of the same vector hits it.
  static Point vartime_multiscalar_mul(const std::vector<Scalar>& scalars, const std::vector<Affine>& bases,
                                       bool mont = false) {
    if (scalars.size() != bases.size()) throw std::invalid_argument("assert_eq!(coeffs.len(), bases.len())");
    Point p;
    uint8_t inf = 0;
    uint32_t flags = mont ? (NMX_SCALARS_MONT | NMX_BASES_MONT) : 0u;
    check(nmx_msm(CURVE, scalars.data(), bases.data(), scalars.size(), flags, p.xy.data(), &inf));
    p.is_inf = inf != 0;
    return p;
  }
  // same over a registered key prefix (`&ck.ck[..v.len()]`)
  static Point vartime_multiscalar_mul(const std::vector<Scalar>& scalars, const CommitmentKey& ck, bool mont = false) {
    if (scalars.size() > ck.len()) throw std::invalid_argument("assert!(ck.ck.len() >= v.len())");
    Point p;
    uint8_t inf = 0;
    check(nmx_msm_handle(ck.handle(), 0, scalars.data(), scalars.size(), mont ? NMX_SCALARS_MONT : 0u,
                         p.xy.data(), &inf));
    p.is_inf = inf != 0;
    return p;
  }
  // traits.rs:82-90: the j-th vector uses bases[..len_j]
  static std::vector<Point> batch_vartime_multiscalar_mul(const std::vector<std::vector<Scalar>>& scalars,
                                                          const CommitmentKey& ck, bool mont = false) {
    std::vector<const void*> ptrs;
    std::vector<size_t> lens;
    for (auto& v : scalars) {
      ptrs.push_back(v.data());
      lens.push_back(v.size());
    }
    std::vector<uint8_t> out(64 * scalars.size() + 1), inf(scalars.size() + 1);
    check(nmx_msm_batch_handle(ck.handle(), ptrs.data(), lens.data(), scalars.size(), mont ? NMX_SCALARS_MONT : 0u,
                               out.data(), inf.data()));
    std::vector<Point> r(scalars.size());
    for (size_t j = 0; j < scalars.size(); j++) {
      std::copy(out.begin() + 64 * j, out.begin() + 64 * j + 64, r[j].xy.begin());
      r[j].is_inf = inf[j] != 0;
    }
    return r;
  }
  // traits.rs:93-106 (`T: Into<u64>`: widen to u64 before the call)
  static Point vartime_multiscalar_mul_small(const std::vector<uint64_t>& scalars, const CommitmentKey& ck) {
    return vartime_multiscalar_mul_small_with_max_num_bits(scalars, ck, NMX_BITS_AUTO);
  }
  static Point vartime_multiscalar_mul_small_with_max_num_bits(const std::vector<uint64_t>& scalars,
                                                               const CommitmentKey& ck, uint32_t max_num_bits) {
    if (scalars.size() > ck.len()) throw std::invalid_argument("assert_eq!(bases.len(), scalars.len())");
    Point p;
    uint8_t inf = 0;
    check(nmx_msm_u64_handle(ck.handle(), 0, scalars.data(), scalars.size(), max_num_bits, 0, p.xy.data(), &inf));
    p.is_inf = inf != 0;
    return p;
  }
  // traits.rs:109-117: batch_vartime_multiscalar_mul_small -- the j-th vector uses bases[..len_j]
  static std::vector<Point> batch_vartime_multiscalar_mul_small(const std::vector<std::vector<uint64_t>>& scalars,
                                                                const CommitmentKey& ck, uint32_t max_num_bits = NMX_BITS_AUTO) {
    std::vector<const uint64_t*> ptrs;
    std::vector<size_t> lens;
    for (auto& v : scalars) {
      ptrs.push_back(v.data());
      lens.push_back(v.size());
    }
    std::vector<uint8_t> out(64 * scalars.size() + 1), inf(scalars.size() + 1);
    check(nmx_msm_u64_batch_handle(ck.handle(), ptrs.data(), lens.data(), scalars.size(), max_num_bits, 0u, out.data(), inf.data()));
    std::vector<Point> r(scalars.size());
    for (size_t j = 0; j < scalars.size(); j++) {
      std::copy(out.begin() + 64 * j, out.begin() + 64 * j + 64, r[j].xy.begin());
      r[j].is_inf = inf[j] != 0;
    }
    return r;
  }
};

// `CommitmentEngineTrait` restricted to the hot path.
template <int CURVE> struct CommitmentEngine {
  // pedersen.rs:263-270 / hyperkzg.rs:584-591:  msm(v, ck[..len v]) + h * r
  static Point commit(const CommitmentKey& ck, const std::vector<Scalar>& v, const Scalar& r, bool mont = false) {
    if (ck.len() < v.size()) throw std::invalid_argument("assert!(ck.ck.len() >= v.len())");
    Point p;
    uint8_t inf = 0;
    uint32_t flags = (mont ? NMX_SCALARS_MONT : 0u) | (ck.mont() ? NMX_BASES_MONT : 0u);
    check(nmx_commit(ck.handle(), v.data(), v.size(), ck.h().data(), r.data(), flags, p.xy.data(), &inf));
    p.is_inf = inf != 0;
    return p;
  }
  // The same commitment begun now and collected later (nmx_commit_begin / nmx_commit_finish): `W.commit(ck)` beside the cross
  // term + commit(T) that does not read it (src/r1cs/mod.rs:590-622, src/nova/nifs.rs:53-63).  `v` must outlive finish().
  class Pending {
    uint64_t ticket_ = 0;

   public:
    explicit Pending(uint64_t t) : ticket_(t) {}
    Pending(Pending&& o) noexcept : ticket_(o.ticket_) { o.ticket_ = 0; }
    Pending(const Pending&) = delete;
    Pending& operator=(const Pending&) = delete;
    ~Pending() {  // never leave a ticket behind: wait, drop the result
      uint8_t xy[128], inf;
      if (ticket_) (void)nmx_commit_finish(ticket_, xy, &inf);
    }
    Point finish() {
      Point p;
      uint8_t inf = 0;
      const uint64_t t = ticket_;
      ticket_ = 0;
      check(nmx_commit_finish(t, p.xy.data(), &inf));
      p.is_inf = inf != 0;
      return p;
    }
  };
  static Pending commit_begin(const CommitmentKey& ck, const std::vector<Scalar>& v, const Scalar& r, bool mont = false) {
    if (ck.len() < v.size()) throw std::invalid_argument("assert!(ck.ck.len() >= v.len())");
    uint64_t t = 0;
    uint32_t flags = (mont ? NMX_SCALARS_MONT : 0u) | (ck.mont() ? NMX_BASES_MONT : 0u);
    check(nmx_commit_begin(ck.handle(), v.data(), v.size(), ck.h().data(), r.data(), flags, &t));
    return Pending(t);
  }
  // hyperkzg.rs:593-612 with r_i = 0 (the HyperKZG prover's use)
  static std::vector<Point> batch_commit(const CommitmentKey& ck, const std::vector<std::vector<Scalar>>& v) {
    return DlogGroupExt<CURVE>::batch_vartime_multiscalar_mul(v, ck);
  }
};

}  // namespace provider

// Spartan's sum-check provers (src/spartan/sumcheck.rs) over the C ABI's one-call-per-prover entry points.  `Transcript` is the
// caller's: any type with `Scalar round(const std::vector<Scalar>& unipoly_coeffs)` -- what the reference writes as
// `transcript.absorb(b"p", &poly); transcript.squeeze(b"c")` (sumcheck.rs:224-227, 481-484, 315-318).  Tables are host vectors here
// (uploaded for the call; hosts that keep their vectors in HBM call the C entry points with NMX_SCALARS_DEVICE).
namespace spartan {
using provider::Scalar;
using provider::check;

struct SumcheckProof {                              // what SumcheckProof::new(compressed_polys) is built from, plus r and the claims
  std::vector<std::vector<Scalar>> polys;           // per round: UniPoly coefficients, constant term first
  std::vector<Scalar> r;                            // the challenges
  std::vector<Scalar> claims;                       // final evaluations (poly_A[0], ...)
};
namespace detail {
template <class Transcript> int round_cb(void* ctx, const uint8_t* coeffs32, size_t n, uint8_t* out) {
  try {
    std::vector<Scalar> co(n);
    for (size_t i = 0; i < n; i++) std::copy(coeffs32 + 32 * i, coeffs32 + 32 * i + 32, co[i].begin());
    const Scalar r = static_cast<Transcript*>(ctx)->round(co);
    std::copy(r.begin(), r.end(), out);
    return 0;
  } catch (...) {
    return 1;  // never let an exception cross the C frame: the call fails with NMX_E_ARG
  }
}
inline SumcheckProof unpack(size_t rounds, size_t nco, size_t nclaims, const std::vector<uint8_t>& p, const std::vector<uint8_t>& r,
                            const std::vector<uint8_t>& c) {
  SumcheckProof out;
  out.polys.assign(rounds, std::vector<Scalar>(nco));
  out.r.resize(rounds), out.claims.resize(nclaims);
  for (size_t j = 0; j < rounds; j++) {
    for (size_t i = 0; i < nco; i++) std::copy(p.begin() + 32 * (nco * j + i), p.begin() + 32 * (nco * j + i) + 32, out.polys[j][i].begin());
    std::copy(r.begin() + 32 * j, r.begin() + 32 * j + 32, out.r[j].begin());
  }
  for (size_t i = 0; i < nclaims; i++) std::copy(c.begin() + 32 * i, c.begin() + 32 * i + 32, out.claims[i].begin());
  return out;
}
}  // namespace detail

template <int FIELD> struct Sumcheck {
  // SumcheckProof::prove_cubic_with_three_inputs (sumcheck.rs:446-507)
  template <class Transcript>
  static SumcheckProof prove_cubic_with_three_inputs(const Scalar& claim, const std::vector<Scalar>& taus, const std::vector<Scalar>& A,
                                                     const std::vector<Scalar>& B, const std::vector<Scalar>& C, Transcript& tr, bool mont = false) {
    const size_t l = taus.size();
    if (A.size() != (size_t)1 << l || B.size() != A.size() || C.size() != A.size()) throw std::invalid_argument("tables must hold 2^taus.len() elements");
    std::vector<uint8_t> p(128 * l + 1), r(32 * l + 1), c(96);
    check(nmx_sumcheck_prove_cubic_with_three_inputs(FIELD, claim.data(), taus.data(), l, const_cast<Scalar*>(A.data()), const_cast<Scalar*>(B.data()),
                                                     const_cast<Scalar*>(C.data()), mont ? NMX_SCALARS_MONT : 0u, &detail::round_cb<Transcript>, &tr,
                                                     p.data(), r.data(), c.data()));
    return detail::unpack(l, 4, 3, p, r, c);
  }
  // SumcheckProof::prove_quad_prod (sumcheck.rs:199-249)
  template <class Transcript>
  static SumcheckProof prove_quad_prod(const Scalar& claim, size_t num_rounds, const std::vector<Scalar>& A, const std::vector<Scalar>& B,
                                       Transcript& tr, bool mont = false) {
    if (A.size() != (size_t)1 << num_rounds || B.size() != A.size()) throw std::invalid_argument("tables must hold 2^num_rounds elements");
    std::vector<uint8_t> p(96 * num_rounds + 1), r(32 * num_rounds + 1), c(64);
    check(nmx_sumcheck_prove_quad_prod(FIELD, claim.data(), num_rounds, const_cast<Scalar*>(A.data()), const_cast<Scalar*>(B.data()),
                                       mont ? NMX_SCALARS_MONT : 0u, &detail::round_cb<Transcript>, &tr, p.data(), r.data(), c.data()));
    return detail::unpack(num_rounds, 3, 2, p, r, c);
  }
  // SumcheckProof::prove_batch_eval (sumcheck.rs:251-353)
  template <class Transcript>
  static SumcheckProof prove_batch_eval(const std::vector<Scalar>& claims, const std::vector<std::vector<Scalar>>& polys,
                                        const std::vector<std::vector<Scalar>>& eq_points, const std::vector<Scalar>& coeffs, Transcript& tr,
                                        bool mont = false) {
    const size_t k = polys.size();
    if (claims.size() != k || eq_points.size() != k || coeffs.size() != k || k == 0) throw std::invalid_argument("one claim, point and coefficient per polynomial");
    std::vector<size_t> nr(k);
    std::vector<void*> pp(k);
    std::vector<const void*> qp(k);
    size_t nmax = 0;
    for (size_t i = 0; i < k; i++) {
      nr[i] = eq_points[i].size();
      if (polys[i].size() != (size_t)1 << nr[i]) throw std::invalid_argument("poly size mismatch");
      pp[i] = const_cast<Scalar*>(polys[i].data()), qp[i] = eq_points[i].data();
      nmax = nr[i] > nmax ? nr[i] : nmax;
    }
    std::vector<uint8_t> p(96 * nmax + 1), r(32 * nmax + 1), f(32 * k);
    check(nmx_sumcheck_prove_batch_eval(FIELD, claims.data(), nr.data(), pp.data(), qp.data(), coeffs.data(), k, mont ? NMX_SCALARS_MONT : 0u,
                                        &detail::round_cb<Transcript>, &tr, p.data(), r.data(), f.data()));
    return detail::unpack(nmax, 3, k, p, r, f);
  }
  // SumcheckProof::prove_batched_cubic (sumcheck.rs:509-577): k <= 16 triples under one sum-check; claims = [A_0(r), B_0(r), C_0(r), A_1(r), ...]
  template <class Transcript>
  static SumcheckProof prove_batched_cubic(const Scalar& claim, const std::vector<Scalar>& taus, const std::vector<std::vector<Scalar>>& As,
                                           const std::vector<std::vector<Scalar>>& Bs, const std::vector<std::vector<Scalar>>& Cs,
                                           const std::vector<Scalar>& alphas, Transcript& tr, bool mont = false) {
    const size_t l = taus.size(), k = As.size();
    if (k == 0 || Bs.size() != k || Cs.size() != k || alphas.size() != k) throw std::invalid_argument("one B, C and alpha per A, at least one");
    std::vector<void*> pa(k), pb(k), pc(k);
    for (size_t i = 0; i < k; i++) {
      if (As[i].size() != (size_t)1 << l || Bs[i].size() != As[i].size() || Cs[i].size() != As[i].size()) throw std::invalid_argument("tables must hold 2^taus.len() elements");
      pa[i] = const_cast<Scalar*>(As[i].data()), pb[i] = const_cast<Scalar*>(Bs[i].data()), pc[i] = const_cast<Scalar*>(Cs[i].data());
    }
    std::vector<uint8_t> p(128 * l + 1), r(32 * l + 1), c(96 * k);
    check(nmx_sumcheck_prove_batched_cubic(FIELD, claim.data(), taus.data(), l, pa.data(), pb.data(), pc.data(), alphas.data(), k,
                                           mont ? NMX_SCALARS_MONT : 0u, &detail::round_cb<Transcript>, &tr, p.data(), r.data(), c.data()));
    return detail::unpack(l, 4, 3 * k, p, r, c);
  }
  // RelaxedR1CSSNARK::prove_helper (ppsnark.rs:886-983): the batched inner sum-check of the pre-processing SNARK over its sixteen tables in
  // the order NMX_PPS_* (copies: they are bound in place); claims = the sixteen tables at r, in table order
  template <class Transcript>
  static SumcheckProof prove_ppsnark(const std::vector<std::vector<Scalar>>& tables, const std::vector<Scalar>& rhos, const std::vector<Scalar>& r_outer,
                                     const std::array<Scalar, 2>& claims2, const std::array<Scalar, 9>& coeffs, Transcript& tr, bool mont = false) {
    const size_t l = rhos.size();
    if (tables.size() != NMX_PPS_TABLES || r_outer.size() != l) throw std::invalid_argument("sixteen tables, one r_outer per rho");
    std::vector<void*> pt(NMX_PPS_TABLES);
    for (size_t t = 0; t < NMX_PPS_TABLES; t++) {
      if (tables[t].size() != (size_t)1 << l) throw std::invalid_argument("tables must hold 2^rhos.len() elements");
      pt[t] = const_cast<Scalar*>(tables[t].data());
    }
    std::vector<uint8_t> p(128 * l + 1), r(32 * l + 1), c(32 * NMX_PPS_TABLES);
    check(nmx_sumcheck_prove_ppsnark(FIELD, l, pt.data(), rhos.data(), r_outer.data(), claims2.data(), coeffs.data(), mont ? NMX_SCALARS_MONT : 0u,
                                     &detail::round_cb<Transcript>, &tr, p.data(), r.data(), c.data()));
    return detail::unpack(l, 4, NMX_PPS_TABLES, p, r, c);
  }
};
}  // namespace spartan

// The inner-product argument (src/provider/ipa_pc.rs:174-281) over the C ABI's one call.  `Transcript` is the caller's: any type with
// `Scalar round(const Point& L, const Point& R)` -- `transcript.absorb(b"L", &L); transcript.absorb(b"R", &R); transcript.squeeze(b"r")`
// (:231-234).  Host vectors here (uploaded for the call); `ck_c` is the already scaled one-point key (`ck_c.scale(&r)`, :190-191).
namespace ipa {
using provider::Affine;
using provider::check;
using provider::CommitmentKey;
using provider::Point;
using provider::Scalar;

struct InnerProductArgument {  // L_vec, R_vec, a_hat (:157-162)
  std::vector<Point> L_vec, R_vec;
  Scalar a_hat{};
};
namespace detail {
template <class Transcript> int round_cb(void* ctx, const uint8_t* L, int L_inf, const uint8_t* R, int R_inf, uint8_t* out) {
  try {
    Point l, r;
    std::copy(L, L + 64, l.xy.begin()), std::copy(R, R + 64, r.xy.begin());
    l.is_inf = L_inf != 0, r.is_inf = R_inf != 0;
    const Scalar c = static_cast<Transcript*>(ctx)->round(l, r);
    std::copy(c.begin(), c.end(), out);
    return 0;
  } catch (...) {
    return 1;  // never let an exception cross the C frame: the call fails with NMX_E_ARG
  }
}
}  // namespace detail
template <class Transcript>
InnerProductArgument prove(const CommitmentKey& ck, const Affine& ck_c, const std::vector<Scalar>& a_vec, const std::vector<Scalar>& b_vec,
                           Transcript& tr, bool mont = false) {
  if (a_vec.size() != b_vec.size() || a_vec.empty()) throw std::invalid_argument("InvalidInputLength (ipa_pc.rs:185-187)");
  const size_t n = a_vec.size();
  size_t rounds = 0;
  while (((size_t)1 << rounds) < n) rounds++;
  std::vector<uint8_t> L(64 * rounds + 1), R(64 * rounds + 1), inf(2 * rounds + 1);
  InnerProductArgument out;
  check(nmx_ipa_prove(ck.handle(), ck_c.data(), a_vec.data(), b_vec.data(), n, mont ? NMX_SCALARS_MONT : 0u, &detail::round_cb<Transcript>, &tr,
                      L.data(), R.data(), inf.data(), out.a_hat.data()));
  out.L_vec.resize(rounds), out.R_vec.resize(rounds);
  for (size_t k = 0; k < rounds; k++) {
    std::copy(L.begin() + 64 * k, L.begin() + 64 * k + 64, out.L_vec[k].xy.begin());
    std::copy(R.begin() + 64 * k, R.begin() + 64 * k + 64, out.R_vec[k].xy.begin());
    out.L_vec[k].is_inf = inf[2 * k] != 0, out.R_vec[k].is_inf = inf[2 * k + 1] != 0;
  }
  return out;
}
// InnerProductArgument::verify (src/provider/ipa_pc.rs:286-390) from the point where the caller's transcript has produced `rs` (it absorbs
// L_vec[i], R_vec[i] and squeezes, :315-321; round 0 first).  `b`: U.b_vec (n elements), or with b_is_point the evaluation point of
// EvaluationEngine::verify (:80-99; log2(n) elements, the eq table is never built).  true: accepted; false: NovaError::InvalidPCS.
namespace detail {
inline bool verify_call(const CommitmentKey& ck, const Affine& ck_c, const Point& comm_a, const Scalar& c, const void* b, size_t n,
                        const InnerProductArgument& proof, const std::vector<Scalar>& rs, uint32_t flags) {
  const size_t rounds = proof.L_vec.size();
  if (proof.R_vec.size() != rounds || rs.size() != rounds || n != ((size_t)1 << rounds))
    throw std::invalid_argument("InvalidInputLength (ipa_pc.rs:297-303)");
  std::vector<uint8_t> L(64 * rounds + 1), R(64 * rounds + 1), inf(2 * rounds + 1);
  for (size_t k = 0; k < rounds; k++) {
    std::copy(proof.L_vec[k].xy.begin(), proof.L_vec[k].xy.end(), L.begin() + 64 * k);
    std::copy(proof.R_vec[k].xy.begin(), proof.R_vec[k].xy.end(), R.begin() + 64 * k);
    inf[2 * k] = proof.L_vec[k].is_inf, inf[2 * k + 1] = proof.R_vec[k].is_inf;
  }
  uint32_t verdict = 0;
  check(nmx_ipa_verify(ck.handle(), ck_c.data(), comm_a.xy.data(), comm_a.is_inf ? 1 : 0, c.data(), b, n, L.data(), R.data(), inf.data(),
                       proof.a_hat.data(), rs.data(), flags | (ck.mont() ? NMX_BASES_MONT : 0u), &verdict, nullptr, nullptr, nullptr));
  return verdict == 0;
}
}  // namespace detail
inline bool verify(const CommitmentKey& ck, const Affine& ck_c, const Point& comm_a, const Scalar& c, const std::vector<Scalar>& b,
                   const InnerProductArgument& proof, const std::vector<Scalar>& rs, bool mont = false, bool b_is_point = false) {
  const size_t n = b_is_point ? (size_t)1 << b.size() : b.size();
  if (b.empty() && !b_is_point) throw std::invalid_argument("InvalidInputLength (ipa_pc.rs:297-303)");
  const Scalar none{};
  return detail::verify_call(ck, ck_c, comm_a, c, b.empty() ? none.data() : b.data()->data(), n, proof, rs,
                             (mont ? NMX_SCALARS_MONT : 0u) | (b_is_point ? NMX_IPA_B_IS_POINT : 0u));
}
}  // namespace ipa

// HyperKZG's evaluation argument (src/provider/hyperkzg.rs:926-1116) over the C ABI's one call.  `Transcript` is the caller's: any type
// with `Scalar stage(int stage, const uint8_t* data, size_t count, const uint8_t* is_inf)` -- stage 0 absorbs the count = ell - 1
// commitments (64 bytes each, is_inf[i]: point i is the identity) and squeezes r (:861-865), stage 1 absorbs the count = 3 ell scalars of
// v and squeezes q (:869-880), stage 2 absorbs the three w (:1069; what it returns is ignored).  It runs on the calling thread and must not
// synchronise the device.  The pairing check and tau_H stay the caller's.
namespace hyperkzg {
using provider::check;
using provider::CommitmentKey;
using provider::Point;
using provider::Scalar;

struct EvaluationArgument {  // com, w, v (:310-330)
  std::vector<Point> com;
  std::vector<std::array<Scalar, 3>> v;
  std::array<Point, 3> w{};
};
namespace detail {
template <class Transcript> int stage_cb(void* ctx, int stage, const uint8_t* data, size_t count, const uint8_t* is_inf, uint8_t* out) {
  try {
    const Scalar c = static_cast<Transcript*>(ctx)->stage(stage, data, count, is_inf);
    std::copy(c.begin(), c.end(), out);
    return 0;
  } catch (...) {
    return 1;  // never let an exception cross the C frame: the call fails with NMX_E_ARG
  }
}
// hat_P: n = 2^ell elements where `flags` says; point: ell coordinates, point[0] first as the reference's x
inline EvaluationArgument prove_call(const CommitmentKey& ck, const void* hat_P, size_t n, const std::vector<Scalar>& point, uint32_t flags,
                                     nmx_transcript_fn_kzg cb, void* ctx) {
  size_t ell = 0;
  while (((size_t)1 << ell) < n) ell++;
  if (n < 2 || point.size() != ell) throw std::invalid_argument("hyperkzg::prove: n = 2^ell >= 2 and ell coordinates");
  std::vector<uint8_t> com(64 * ell), com_inf(ell), v(96 * ell), w(192), w_inf(3);
  check(nmx_hyperkzg_prove(ck.handle(), hat_P, n, point.data(), flags | (ck.mont() ? NMX_BASES_MONT : 0u), cb, ctx, com.data(), com_inf.data(),
                           v.data(), w.data(), w_inf.data()));
  EvaluationArgument out;
  out.com.resize(ell - 1), out.v.resize(ell);
  for (size_t i = 0; i + 1 < ell; i++) {
    std::copy(com.begin() + 64 * i, com.begin() + 64 * i + 64, out.com[i].xy.begin());
    out.com[i].is_inf = com_inf[i] != 0;
  }
  for (size_t i = 0; i < ell; i++)
    for (size_t j = 0; j < 3; j++) std::copy(v.begin() + 96 * i + 32 * j, v.begin() + 96 * i + 32 * j + 32, out.v[i][j].begin());
  for (size_t j = 0; j < 3; j++) {
    std::copy(w.begin() + 64 * j, w.begin() + 64 * j + 64, out.w[j].xy.begin());
    out.w[j].is_inf = w_inf[j] != 0;
  }
  return out;
}
}  // namespace detail
template <class Transcript>
EvaluationArgument prove(const CommitmentKey& ck, const std::vector<Scalar>& hat_P, const std::vector<Scalar>& point, Transcript& tr, bool mont = false) {
  return detail::prove_call(ck, hat_P.data(), hat_P.size(), point, mont ? NMX_SCALARS_MONT : 0u, &detail::stage_cb<Transcript>, &tr);
}
}  // namespace hyperkzg

// Mercury's evaluation argument (src/provider/mercury.rs:891-1268) over the C ABI's one call.  `Transcript` is the caller's, of the shape
// hyperkzg::prove takes: stage 0 absorbs comm_h and squeezes alpha, stage 1 comm_q and comm_g -> gamma, stage 2 comm_s and comm_d -> zeta,
// stage 3 the six evaluations (count = 6 scalars; what it returns is ignored), stage 4 comm_quot_f -> beta, stage 5 comm_w -> z, stage 6
// comm_w_prime (ignored: the reference squeezes the pairing challenge there).  The caller has absorbed f, u and e (:905-907) before.  It
// runs on the calling thread and must not synchronise the device.  verify, G2 and tau_H stay the caller's.
namespace mercury {
using provider::check;
using provider::CommitmentKey;
using provider::Point;
using provider::Scalar;

struct EvaluationArgument {  // the fields of the reference's struct, in its order
  Point comm_h, comm_g, comm_q, comm_s, comm_d, comm_quot_f, comm_w, comm_w_prime;
  Scalar g_zeta{}, g_zeta_inv{}, h_zeta{}, h_zeta_inv{}, s_zeta{}, s_zeta_inv{};
};
namespace detail {
// poly: n = 2^ell >= 4 elements where `flags` says; point: ell coordinates in the reference's order
inline EvaluationArgument prove_call(const CommitmentKey& ck, const void* poly, size_t n, const std::vector<Scalar>& point, uint32_t flags,
                                     nmx_transcript_fn_kzg cb, void* ctx) {
  size_t ell = 0;
  while (((size_t)1 << ell) < n) ell++;
  if (n < 4 || point.size() != ell) throw std::invalid_argument("mercury::prove: n = 2^ell >= 4 and ell coordinates");
  std::vector<uint8_t> comms(512), infs(8), evals(192);
  check(nmx_mercury_prove(ck.handle(), poly, n, point.data(), flags | (ck.mont() ? NMX_BASES_MONT : 0u), cb, ctx, comms.data(), infs.data(),
                          evals.data()));
  EvaluationArgument out;
  Point* const pts[8] = {&out.comm_h, &out.comm_g, &out.comm_q, &out.comm_s, &out.comm_d, &out.comm_quot_f, &out.comm_w, &out.comm_w_prime};
  for (size_t i = 0; i < 8; i++) {
    std::copy(comms.begin() + 64 * i, comms.begin() + 64 * i + 64, pts[i]->xy.begin());
    pts[i]->is_inf = infs[i] != 0;
  }
  Scalar* const evs[6] = {&out.g_zeta, &out.g_zeta_inv, &out.h_zeta, &out.h_zeta_inv, &out.s_zeta, &out.s_zeta_inv};
  for (size_t i = 0; i < 6; i++) std::copy(evals.begin() + 32 * i, evals.begin() + 32 * i + 32, evs[i]->begin());
  return out;
}
}  // namespace detail
template <class Transcript>
EvaluationArgument prove(const CommitmentKey& ck, const std::vector<Scalar>& poly, const std::vector<Scalar>& point, Transcript& tr, bool mont = false) {
  return detail::prove_call(ck, poly.data(), poly.size(), point, mont ? NMX_SCALARS_MONT : 0u, &hyperkzg::detail::stage_cb<Transcript>, &tr);
}
}  // namespace mercury

// Hosts that keep their vectors in HBM between provider calls (INTEGRATION.md sections 2b-2e: the patched r1cs/mod.rs, nifs.rs,
// snark.rs): the same operations over device pointers.  Thin by design -- each function is one C call with NMX_SCALARS_DEVICE (and
// NMX_ASYNC where the host does not look at the result before its next synchronous call); allocation is the host's business
// (hipMalloc, a pool, torch).  `n` counts 32-byte elements.  Used by bench/csnark_replay.cpp (the chained CompressedSNARK::prove replay).
namespace resident {
using provider::Affine;
using provider::check;
using provider::CommitmentKey;
using provider::Point;
using provider::Scalar;
constexpr uint32_t kDev = NMX_SCALARS_DEVICE, kAsync = NMX_SCALARS_DEVICE | NMX_ASYNC;

inline Point commit(const CommitmentKey& ck, const void* v, size_t n, const Scalar& r) {  // CE::commit (pedersen.rs:263-270, hyperkzg.rs:584-591)
  Point p;
  uint8_t inf = 0;
  check(nmx_commit(ck.handle(), v, n, ck.h().data(), r.data(), kDev, p.xy.data(), &inf));
  p.is_inf = inf != 0;
  return p;
}
// CE::ck_derive_by_address (commitment.rs:177-194) with the n addresses (64-bit words) in HBM: the kernel checks them against table_size
inline CommitmentKey derive_by_address(const CommitmentKey& ck, const uint64_t* d_addresses, size_t n, size_t table_size, bool precompute = true) {
  return ck.derive_by_device_address(d_addresses, n, table_size, precompute);
}
inline uint64_t commit_begin(const CommitmentKey& ck, const void* v, size_t n, const Scalar& r) {  // one arm of a rayon::join of two commits
  uint64_t t = 0;
  check(nmx_commit_begin(ck.handle(), v, n, ck.h().data(), r.data(), kDev, &t));
  return t;
}
inline Point commit_finish(uint64_t ticket) {
  Point p;
  uint8_t inf = 0;
  check(nmx_commit_finish(ticket, p.xy.data(), &inf));
  p.is_inf = inf != 0;
  return p;
}
inline std::vector<Point> batch_commit(const CommitmentKey& ck, const std::vector<const void*>& vs, const std::vector<size_t>& lens) {  // hyperkzg.rs:593-612, r_i = 0
  const size_t k = vs.size();
  std::vector<uint8_t> xy(64 * (k ? k : 1)), inf(k ? k : 1);
  check(nmx_msm_batch_handle(ck.handle(), vs.data(), lens.data(), k, kDev, xy.data(), inf.data()));
  std::vector<Point> out(k);
  for (size_t i = 0; i < k; i++) {
    std::copy(xy.begin() + 64 * i, xy.begin() + 64 * i + 64, out[i].xy.begin());
    out[i].is_inf = inf[i] != 0;
  }
  return out;
}
// z = [W | u | X | 0 ...] (snark.rs:133, r1cs/mod.rs:638-639)
inline void concat_z(int field, const void* W, size_t n, const Scalar& u, const Scalar& X, size_t n_out, void* out) {
  const void* parts[3] = {W, u.data(), X.data()};
  const size_t lens[3] = {n, 1, 1};
  check(nmx_field_concat(field, parts, lens, 1u, 3, n_out, kAsync, out));
}
inline void clone(int field, const void* v, size_t n, void* out) {
  const void* parts[1] = {v};
  const size_t lens[1] = {n};
  check(nmx_field_concat(field, parts, lens, 1u, 1, n, kAsync, out));
}
inline void vec_add(int field, const void* a, const void* b, size_t n, void* out) { check(nmx_field_vec_add(field, a, b, n, kAsync, out)); }
inline void axpy(int field, const void* a, const void* b, const Scalar& r, size_t n, void* out) { check(nmx_field_axpy(field, a, b, r.data(), n, kAsync, out)); }
inline void axpy2(int field, const void* a, const void* b, const void* c, const Scalar& r, size_t n, void* out) {
  check(nmx_field_axpy2(field, a, b, c, r.data(), n, kAsync, out));
}
inline void cross_term2(int field, const void* az, const void* bz, const void* cz, const void* e1, const void* e2, const Scalar& u, size_t n, void* out) {
  check(nmx_field_cross_term2(field, az, bz, cz, e1, e2, u.data(), n, kAsync, out));
}
// R1CSShape::multiply_vec / compute_eval_table_sparse: the three products in one call
inline void multiply_vec3(const uint64_t mats[3], bool transposed, const void* x, size_t x_len, void* const outs[3]) {
  check(nmx_spmv_apply_many(mats, 3, transposed ? 1 : 0, x, x_len, kAsync, outs));
}
// AZ o BZ - u CZ - E over Z = z (sample_random_instance_witness with E = 0, r1cs/mod.rs:803-812)
inline void r1cs_cross_term(const uint64_t mats[3], const void* z, size_t z_len, const void* e, const Scalar& u, void* out) {
  check(nmx_r1cs_cross_term(mats[0], mats[1], mats[2], z, nullptr, z_len, e, u.data(), kAsync, out));
}
// R1CSShape::is_sat / is_sat_relaxed (r1cs/mod.rs:474-574; the three checks of RecursiveSNARK::verify, nova/mod.rs:637-660) as one
// call each: the equation decided on the device, the commitments beside it.  W (n_w elements) and E (n_e) are HBM pointers, or host
// arrays with device = false (a proof received from a peer); X is a host vector; comm_W / comm_E in the key's form (Montgomery when
// ck.mont(), like ck.h()).  ck == nullptr: the equation only (the prover-side debug_assert!).
struct SatResult {
  uint32_t verdict = 0;  // OR of NMX_UNSAT_*
  uint64_t bad_rows = 0, first_bad_row = ~0ull;
  bool ok() const { return verdict == 0; }
  bool eq_ok() const { return !(verdict & NMX_UNSAT_EQ); }
  bool comm_W_ok() const { return !(verdict & NMX_UNSAT_COMM_W); }
  bool comm_E_ok() const { return !(verdict & NMX_UNSAT_COMM_E); }
};
inline SatResult r1cs_is_sat_relaxed(const uint64_t mats[3], const CommitmentKey* ck, const void* W, size_t n_w, const void* E, size_t n_e,
                                     const Scalar& u, const std::vector<Scalar>& X, const Point& comm_W, const Point& comm_E,
                                     const Scalar& r_W = Scalar{}, const Scalar& r_E = Scalar{}, bool device = true, bool mont = false) {
  SatResult s;
  const uint32_t flags = (device ? kDev : 0u) | (mont ? NMX_SCALARS_MONT : 0u) | ((ck && ck->mont()) ? NMX_BASES_MONT : 0u);
  check(nmx_r1cs_is_sat(mats[0], mats[1], mats[2], ck ? ck->handle() : 0, W, n_w, E, n_e, u.data(), X.empty() ? nullptr : X[0].data(), X.size(),
                        r_W.data(), r_E.data(), ck ? ck->h().data() : nullptr, comm_W.xy.data(), comm_W.is_inf ? 1 : 0, comm_E.xy.data(),
                        comm_E.is_inf ? 1 : 0, flags, &s.verdict, &s.bad_rows, &s.first_bad_row));
  return s;
}
inline SatResult r1cs_is_sat(const uint64_t mats[3], const CommitmentKey* ck, const void* W, size_t n_w, const std::vector<Scalar>& X,
                             const Point& comm_W, const Scalar& r_W = Scalar{}, bool device = true, bool mont = false) {
  SatResult s;
  const uint32_t flags = (device ? kDev : 0u) | (mont ? NMX_SCALARS_MONT : 0u) | ((ck && ck->mont()) ? NMX_BASES_MONT : 0u);
  check(nmx_r1cs_is_sat(mats[0], mats[1], mats[2], ck ? ck->handle() : 0, W, n_w, nullptr, 0, nullptr, X.empty() ? nullptr : X[0].data(), X.size(),
                        r_W.data(), nullptr, ck ? ck->h().data() : nullptr, comm_W.xy.data(), comm_W.is_inf ? 1 : 0, nullptr, 0, flags,
                        &s.verdict, &s.bad_rows, &s.first_bad_row));
  return s;
}
// RelaxedR1CSSNARK::verify's multi_evaluate (spartan/snark.rs:325-353) as one call: evals[i] = sum over the entries (row, col, val) of
// mats[i] of eq(r_x, row) eq(r_y, col) val -- what snark.rs:355 multiplies by eval_Z.  r_x, r_y are host vectors (element 0 the most
// significant variable) with rows <= 2^r_x.size() and cols <= 2^r_y.size() for every matrix; mont: they, and the result, are
// Montgomery limbs.  Reads the forward CSR arrays only: no transposed form is built.
inline std::vector<Scalar> r1cs_evaluate(const uint64_t* mats, size_t k, const std::vector<Scalar>& r_x, const std::vector<Scalar>& r_y,
                                         bool mont = false) {
  std::vector<Scalar> out(k ? k : 1);
  check(nmx_r1cs_evaluate(mats, k, r_x.empty() ? nullptr : r_x[0].data(), r_x.size(), r_y.empty() ? nullptr : r_y[0].data(), r_y.size(),
                          mont ? NMX_SCALARS_MONT : 0u, out[0].data()));
  out.resize(k);
  return out;
}
inline Scalar mle_evaluate(int field, const void* z, size_t len, const std::vector<Scalar>& r) {
  Scalar out;
  check(nmx_mle_evaluate(field, z, len, r.data(), r.size(), kDev, out.data()));
  return out;
}
inline std::vector<Scalar> mle_multi_evaluate(int field, const std::vector<const void*>& zs, size_t len, const std::vector<Scalar>& r) {
  std::vector<Scalar> out(zs.size());
  check(nmx_mle_multi_evaluate(field, zs.data(), zs.size(), len, r.data(), r.size(), kDev, out[0].data()));
  return out;
}
inline void eq_evals(int field, const std::vector<Scalar>& r, void* out) { check(nmx_eq_evals_from_points(field, r.data(), r.size(), kDev, out)); }
inline void lincomb_powers(int field, const std::vector<const void*>& vs, const std::vector<size_t>& lens, const Scalar& s, size_t n_out, void* out) {
  check(nmx_field_lincomb_powers(field, vs.data(), lens.data(), vs.size(), s.data(), n_out, kDev, out));
}
inline void fold_pairs(int field, const void* p, size_t len, const Scalar& x, void* out) { check(nmx_poly_fold_pairs(field, p, len, x.data(), kAsync, out)); }
// the fold loop of hyperkzg.rs:1085-1095 in one call: outs[i] = fold(outs[i - 1] or p, xs[i])
inline void fold_chain(int field, const void* p, size_t len, const std::vector<Scalar>& xs, const std::vector<void*>& outs) {
  check(nmx_poly_fold_chain(field, p, len, xs.data(), xs.size(), kAsync, outs.data()));
}
inline void suffix_horner(int field, const void* f, size_t n, const Scalar& u, void* out) { check(nmx_poly_suffix_horner(field, f, n, u.data(), kDev, out)); }
inline std::vector<Scalar> poly_eval_multi(int field, const std::vector<const void*>& polys, const std::vector<size_t>& lens, const std::vector<Scalar>& pts) {
  std::vector<Scalar> out(polys.size() * pts.size());
  check(nmx_poly_eval_multi(field, polys.data(), lens.data(), polys.size(), pts.data(), pts.size(), kDev, out[0].data()));
  return out;
}
// Mercury's N-sized prover passes over an HBM-resident f of n_rows * n_cols coefficients (mercury.rs:966, :995, :1163-1180)
inline void mercury_h_poly(int field, const void* f, size_t n_rows, size_t n_cols, const void* eq_col, void* out_h) {  // compute_h_poly; out_h: n_rows
  check(nmx_mercury_h_poly(field, f, n_rows, n_cols, eq_col, kAsync, out_h));
}
// divide_by_binomial: out_q (n_rows - 1) * n_cols elements (the reference's layout after its transpose, without the zero tail), out_g n_cols
inline void mercury_divide_by_binomial(int field, const void* f, size_t n_rows, size_t n_cols, const Scalar& alpha, void* out_q, void* out_g) {
  check(nmx_mercury_divide_by_binomial(field, f, n_rows, n_cols, alpha.data(), kAsync, out_q, out_g));
}
// the quot_f block from calls that exist.  neg_zeta_b_alpha = -(zeta^b - alpha), the scalar the reference hands to batch_add_with_polynomials
// (:1171); tmp and out: n elements each.  out[1..n) is quot_f; the returned out[0] must equal g(zeta) (the reference's assert_eq!(rem, ZERO)).
inline Scalar mercury_quot_f(int field, const void* f, size_t n, const void* q, size_t n_q, const Scalar& neg_zeta_b_alpha, const Scalar& zeta, void* tmp,
                             void* out) {
  lincomb_powers(field, {f, q}, {n, n_q}, neg_zeta_b_alpha, n, tmp);
  suffix_horner(field, tmp, n, zeta, out);
  // out[0] comes back through the library (this header includes no HIP runtime and so has no device-to-host copy of its own): the
  // one-coefficient polynomial {out[0]} evaluated at 0 is out[0]
  return poly_eval_multi(field, {out}, {1}, {Scalar{}})[0];
}
// NeutronNova's folding step over HBM-resident vectors (neutron/nifs.rs:200-289).  E: left + right elements, the products
// left * right; the scalars are in the layout of the vectors (mont: Montgomery limbs)
inline void pow_split_evals(int field, const Scalar& tau, size_t left, size_t right, void* out, bool mont = false) {  // power.rs:62-86; out: left + right
  check(nmx_pow_split_evals(field, tau.data(), left, right, kAsync | (mont ? NMX_SCALARS_MONT : 0u), out));
}
// prove_helper (nifs.rs:29-186): the evaluations at t = 0, 2, 3, 4, 5
inline std::array<Scalar, 5> neutron_fold_sums(int field, size_t left, size_t right, const void* E1, const void* Az1, const void* Bz1, const void* Cz1,
                                               const void* E2, const void* Az2, const void* Bz2, const void* Cz2, const Scalar& rho, bool mont = false) {
  std::array<Scalar, 5> out;
  check(nmx_neutron_fold_sums(field, left, right, E1, Az1, Bz1, Cz1, E2, Az2, Bz2, Cz2, rho.data(), kDev | (mont ? NMX_SCALARS_MONT : 0u), out[0].data()));
  return out;
}
// the sum of Structure::is_sat (relation.rs:83-97); the comparison with U.T is the caller's
inline Scalar neutron_relation_sum(int field, size_t left, size_t right, const void* E, const void* Az, const void* Bz, const void* Cz, bool mont = false) {
  Scalar out;
  check(nmx_neutron_relation_sum(field, left, right, E, Az, Bz, Cz, kDev | (mont ? NMX_SCALARS_MONT : 0u), out.data()));
  return out;
}
// FoldedWitness::fold (relation.rs:131-156): w = w1 + r_b (w2 - w1), e = e1 + r_b (e2 - e1); w == w1 and e == e1 (in place) are allowed
inline void neutron_fold_witness(int field, const void* w1, const void* w2, size_t n_w, const void* e1, const void* e2, size_t n_e, const Scalar& r_b,
                                 void* w, void* e, bool mont = false) {
  check(nmx_neutron_fold_witness(field, w1, w2, n_w, e1, e2, n_e, r_b.data(), kAsync | (mont ? NMX_SCALARS_MONT : 0u), w, e));
}
// ppsnark's evaluation_oracles (ppsnark.rs:220-253): out[i] = mem[addr[i]], addr n field elements whose values are the addresses; all in HBM
inline void gather(int field, const void* mem, size_t n_mem, const void* addr, size_t n, void* out, bool mont = false) {
  check(nmx_field_gather(field, mem, n_mem, addr, n, kDev | (mont ? NMX_SCALARS_MONT : 0u), out));
}
// ppsnark's compute_oracles (ppsnark.rs:371-489) without its commitments, every memory in one call: mem, addr, L, ts and the four outputs
// hold one HBM pointer per memory, n elements each.  Throws Error with code NMX_E_ZERO when some T + r or W + r is zero.
inline void ppsnark_mem_oracles(int field, size_t n, const std::vector<const void*>& mem, const std::vector<const void*>& addr,
                                const std::vector<const void*>& L, const std::vector<const void*>& ts, const Scalar& gamma, const Scalar& r,
                                const std::vector<void*>& t_plus_r, const std::vector<void*>& w_plus_r, const std::vector<void*>& t_plus_r_inv,
                                const std::vector<void*>& w_plus_r_inv, bool mont = false) {
  const size_t k = mem.size();
  if (addr.size() != k || L.size() != k || ts.size() != k || t_plus_r.size() != k || w_plus_r.size() != k || t_plus_r_inv.size() != k ||
      w_plus_r_inv.size() != k)
    throw std::invalid_argument("ppsnark_mem_oracles: one pointer per memory in every array");
  check(nmx_ppsnark_mem_oracles(field, k, n, mem.data(), addr.data(), L.data(), ts.data(), gamma.data(), r.data(),
                                kDev | (mont ? NMX_SCALARS_MONT : 0u), t_plus_r.data(), w_plus_r.data(), t_plus_r_inv.data(), w_plus_r_inv.data()));
}
// N of R1CSShapeSparkRepr::new (ppsnark.rs:118-121): max(total entries, 2 num_vars, num_cons).next_power_of_two()
inline size_t ppsnark_spark_size(const std::vector<size_t>& nnzs, size_t num_vars, size_t num_cons) {
  size_t m = 2 * num_vars > num_cons ? 2 * num_vars : num_cons, total = 0;
  for (size_t z : nnzs) total += z;
  if (total > m) m = total;
  size_t n = 1;
  while (n < m) n <<= 1;
  return n;
}
// R1CSShapeSparkRepr::new (ppsnark.rs:117-190) over registered matrices (the reference: A, B, C): row, col, vals[j], ts_row, ts_col are HBM
// vectors of n elements each; any may be nullptr (not computed), vals may be empty or hold one pointer per matrix
inline void ppsnark_spark_repr(const std::vector<uint64_t>& mats, size_t n, void* row, void* col, const std::vector<void*>& vals, void* ts_row,
                               void* ts_col, bool mont = false) {
  if (!vals.empty() && vals.size() != mats.size()) throw std::invalid_argument("ppsnark_spark_repr: one value vector per matrix, or none");
  check(nmx_ppsnark_spark_repr(mats.data(), mats.size(), n, kDev | (mont ? NMX_SCALARS_MONT : 0u), row, col, vals.empty() ? nullptr : vals.data(),
                               ts_row, ts_col));
}
// MaskedEqPolynomial::evals (masked_eq.rs:57-75): eq_evals with the first 2^num_masked_vars entries zero; out: 2^r.size() elements in HBM
inline void masked_eq_evals(int field, const std::vector<Scalar>& r, size_t num_masked_vars, void* out, bool mont = false) {
  check(nmx_masked_eq_evals(field, r.data(), r.size(), num_masked_vars, kDev | (mont ? NMX_SCALARS_MONT : 0u), out));
}
// the sum-check provers over HBM-resident tables (bound in place); `cb` / `ctx`: nmx_transcript_fn and its state
struct Proof {
  std::vector<uint8_t> polys, r, claims;
};
inline Proof prove_cubic(int field, const Scalar& claim, const std::vector<Scalar>& taus, void* A, void* B, void* C, nmx_transcript_fn cb, void* ctx) {
  const size_t l = taus.size();
  Proof p{std::vector<uint8_t>(128 * l), std::vector<uint8_t>(32 * l), std::vector<uint8_t>(96)};
  check(nmx_sumcheck_prove_cubic_with_three_inputs(field, claim.data(), taus.data(), l, A, B, C, kDev, cb, ctx, p.polys.data(), p.r.data(), p.claims.data()));
  return p;
}
inline Proof prove_quad(int field, const Scalar& claim, size_t l, void* A, void* B, nmx_transcript_fn cb, void* ctx) {
  Proof p{std::vector<uint8_t>(96 * l), std::vector<uint8_t>(32 * l), std::vector<uint8_t>(64)};
  check(nmx_sumcheck_prove_quad_prod(field, claim.data(), l, A, B, kDev, cb, ctx, p.polys.data(), p.r.data(), p.claims.data()));
  return p;
}
inline Proof prove_batch(int field, const std::vector<Scalar>& claims, const std::vector<size_t>& nr, const std::vector<void*>& polys,
                         const std::vector<const void*>& points, const std::vector<Scalar>& coeffs, nmx_transcript_fn cb, void* ctx) {
  size_t nmax = 0;
  for (size_t v : nr) nmax = v > nmax ? v : nmax;
  Proof p{std::vector<uint8_t>(96 * nmax), std::vector<uint8_t>(32 * nmax), std::vector<uint8_t>(32 * claims.size())};
  check(nmx_sumcheck_prove_batch_eval(field, claims.data(), nr.data(), polys.data(), points.data(), coeffs.data(), claims.size(), kDev, cb, ctx,
                                      p.polys.data(), p.r.data(), p.claims.data()));
  return p;
}
// prove_batched_cubic (sumcheck.rs:509-577) over 3 k HBM-resident tables (k <= 16, no two sharing memory); claims: k x [A_i(r), B_i(r), C_i(r)]
inline Proof prove_batched_cubic(int field, const Scalar& claim, const std::vector<Scalar>& taus, const std::vector<void*>& As, const std::vector<void*>& Bs,
                                 const std::vector<void*>& Cs, const std::vector<Scalar>& alphas, nmx_transcript_fn cb, void* ctx) {
  const size_t l = taus.size(), k = As.size();
  if (Bs.size() != k || Cs.size() != k || alphas.size() != k) throw std::invalid_argument("one B, C and alpha per A");
  Proof p{std::vector<uint8_t>(128 * l), std::vector<uint8_t>(32 * l), std::vector<uint8_t>(96 * k)};
  check(nmx_sumcheck_prove_batched_cubic(field, claim.data(), taus.data(), l, As.data(), Bs.data(), Cs.data(), alphas.data(), k, kDev, cb, ctx,
                                         p.polys.data(), p.r.data(), p.claims.data()));
  return p;
}
// prove_helper (ppsnark.rs:886-983) over the sixteen HBM-resident tables of ppsnark's inner sum-check, in the order NMX_PPS_* (no two sharing
// memory); claims: the sixteen tables at r
inline Proof prove_ppsnark(int field, const std::vector<void*>& tables, const std::vector<Scalar>& rhos, const std::vector<Scalar>& r_outer,
                           const std::array<Scalar, 2>& claims2, const std::array<Scalar, 9>& coeffs, nmx_transcript_fn cb, void* ctx) {
  const size_t l = rhos.size();
  if (tables.size() != NMX_PPS_TABLES || r_outer.size() != l) throw std::invalid_argument("sixteen tables, one r_outer per rho");
  Proof p{std::vector<uint8_t>(128 * l), std::vector<uint8_t>(32 * l), std::vector<uint8_t>(32 * NMX_PPS_TABLES)};
  check(nmx_sumcheck_prove_ppsnark(field, l, tables.data(), rhos.data(), r_outer.data(), claims2.data(), coeffs.data(), kDev, cb, ctx, p.polys.data(),
                                   p.r.data(), p.claims.data()));
  return p;
}
// ck_c.scale(&r) (src/provider/ipa_pc.rs:190-191, pedersen.rs:499-506): one point times one scalar -- a commitment to the empty
// vector with h = the point
inline Affine scale_point(const CommitmentKey& ck, const Affine& h, const Scalar& r) {
  Affine out{};
  uint8_t inf = 0;
  check(nmx_commit(ck.handle(), nullptr, 0, h.data(), r.data(), 0, out.data(), &inf));
  return out;
}
// InnerProductArgument::prove (src/provider/ipa_pc.rs:174-281) over HBM-resident a, b; `ck_c` already scaled (scale_point)
struct IpaProof {
  std::vector<uint8_t> L, R, inf;  // log2 n points of 64 bytes each; inf[2k] / inf[2k + 1]: L_k / R_k is the identity
  Scalar a_hat{};
};
inline IpaProof ipa_prove(const CommitmentKey& ck, const Affine& ck_c, const void* a, const void* b, size_t n, nmx_ipa_transcript_fn cb, void* ctx) {
  size_t rounds = 0;
  while (((size_t)1 << rounds) < n) rounds++;
  IpaProof p{std::vector<uint8_t>(64 * (rounds ? rounds : 1)), std::vector<uint8_t>(64 * (rounds ? rounds : 1)), std::vector<uint8_t>(2 * (rounds ? rounds : 1)), {}};
  check(nmx_ipa_prove(ck.handle(), ck_c.data(), a, b, n, kDev, cb, ctx, p.L.data(), p.R.data(), p.inf.data(), p.a_hat.data()));
  p.L.resize(64 * rounds), p.R.resize(64 * rounds), p.inf.resize(2 * rounds);
  return p;
}
// The three openings of kzg_open_batch (hyperkzg.rs:1007-1072) in one pass over HBM-resident vectors: outs[j][t] = sum_{s >= t} B[s] pts[j]^(s - t)
// with B = sum_i q^i polys[i] (never stored); outs: pts.size() <= 3 vectors of max(lens) elements.  Mercury's quot_f is k = 2, m = 1.
inline void lincomb_quotients(int field, const std::vector<const void*>& polys, const std::vector<size_t>& lens, const Scalar& q,
                              const std::vector<Scalar>& pts, const std::vector<void*>& outs) {
  if (outs.size() != pts.size() || polys.size() != lens.size()) throw std::invalid_argument("lincomb_quotients: one output per point, one length per vector");
  check(nmx_poly_lincomb_quotients(field, polys.data(), lens.data(), polys.size(), q.data(), pts.data(), pts.size(), kDev, outs.data()));
}
// EvaluationEngineTrait::prove of HyperKZG (hyperkzg.rs:926-1116) over an HBM-resident hat_P of n = 2^ell elements; the
// callback runs on the calling thread and must not synchronise the device
inline hyperkzg::EvaluationArgument hyperkzg_prove(const CommitmentKey& ck, const void* hat_P, size_t n, const std::vector<Scalar>& point,
                                                   nmx_transcript_fn_kzg cb, void* ctx, bool mont = false) {
  return hyperkzg::detail::prove_call(ck, hat_P, n, point, kDev | (mont ? NMX_SCALARS_MONT : 0u), cb, ctx);
}
// make_s_polynomial (mercury.rs:391-475) as a correlation over HBM-resident vectors of b elements each; out_s: b - 1
inline void mercury_s_poly(int field, const void* a1, const void* b1, const void* a2, const void* b2, size_t b, const Scalar& gamma, void* out_s) {
  check(nmx_mercury_s_poly(field, a1, b1, a2, b2, b, gamma.data(), kAsync, out_s));
}
// EvaluationEngineTrait::prove of Mercury (mercury.rs:891-1268) over an HBM-resident polynomial of n = 2^ell >= 4 elements; the callback runs on
// the calling thread and must not synchronise the device
inline mercury::EvaluationArgument mercury_prove(const CommitmentKey& ck, const void* poly, size_t n, const std::vector<Scalar>& point,
                                                 nmx_transcript_fn_kzg cb, void* ctx, bool mont = false) {
  return mercury::detail::prove_call(ck, poly, n, point, kDev | (mont ? NMX_SCALARS_MONT : 0u), cb, ctx);
}
// InnerProductArgument::verify (src/provider/ipa_pc.rs:286-390) over an HBM-resident b_vec of n elements
inline bool ipa_verify(const CommitmentKey& ck, const Affine& ck_c, const provider::Point& comm_a, const Scalar& c, const void* b, size_t n,
                       const ipa::InnerProductArgument& proof, const std::vector<Scalar>& rs, bool mont = false) {
  return ipa::detail::verify_call(ck, ck_c, comm_a, c, b, n, proof, rs, kDev | (mont ? NMX_SCALARS_MONT : 0u));
}
}  // namespace resident
}  // namespace nova
