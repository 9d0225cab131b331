// host_point4.hpp -- HOST-ONLY extended-Jacobian (X, Y, ZZ, ZZZ) point arithmetic on HostFp4 (host_fp4.hpp: 4 x 64-bit limbs,
// ~25 ns per product), and the end of the bit-sliced bucket reduction on it.
//
// The last launch of the bit-sliced reduction (reduce_bitsliced.hpp) can leave a bucket set's L + 1 points -- the root and the
// slices O_0 .. O_(L-1) -- instead of combining them: root + sum_l 2^l O_l is L - 1 dependent doublings and a few additions, which
// one 512-thread block runs back to back on one CU while the rest of the chip idles.  A host core does the same chain faster,
// but not with XYZZ<FID> (curve.hpp): its 9 x 29-bit limbs are built for the device and cost 1.1 - 2.6 us per operation on the
// host.  Same formulas (add-2008-s, dbl-2008-s-1 with a = 0) and the same exceptional cases as curve.hpp.
#pragma once
#include "curve.hpp"
#include "host_fp4.hpp"

namespace nmx {

template <int FID> struct HostPoint4 {
  using F = HostFp4<FID>;
  F x, y, zz, zzz;  // identity <=> zz == 0

  static HostPoint4 identity() { return HostPoint4{F::one(), F::one(), F::zero(), F::zero()}; }
  bool is_identity() const { return zz.is_zero(); }

  // XYZZW holds canonical words of value * 2^261 mod p (fp.hpp's form); HostFp4 is value * 2^256.  One Montgomery product each
  // way: words * 2^251 / 2^256 = value * 2^256 on the way in (2^251 < p for all four fields), element * (2^261 mod p) / 2^256 on
  // the way out (the residue of the ELEMENT 2^5 is the integer 2^261 mod p).
  static const F& k_in() {
    static const F k = [] {
      F r = F::zero();
      r.v[3] = (uint64_t)1 << 59;
      return r;
    }();
    return k;
  }
  static const F& k_out() {
    static const F k = F::pow2(5);
    return k;
  }
  static HostPoint4 load(const XYZZW& m) {
    const uint32_t* z = m.w + 16;
    if ((z[0] | z[1] | z[2] | z[3] | z[4] | z[5] | z[6] | z[7]) == 0) return identity();
    HostPoint4 r;
    r.x = F::from_plain_times(m.w, k_in());
    r.y = F::from_plain_times(m.w + 8, k_in());
    r.zz = F::from_plain_times(m.w + 16, k_in());
    r.zzz = F::from_plain_times(m.w + 24, k_in());
    return r;
  }
  void store(XYZZW& m) const {  // canonical: a Montgomery product of values < p is < p
    const HostPoint4 p = is_identity() ? identity() : *this;
    const F o[4] = {p.x * k_out(), p.y * k_out(), p.zz * k_out(), p.zzz * k_out()};
    for (int i = 0; i < 4; i++) memcpy(m.w + 8 * i, o[i].v, 32);
  }

  // dbl-2008-s-1 with a = 0; a point of order 2 (y == 0) cannot occur on these prime-order curves
  void dbl_in_place() {
    if (is_identity()) return;
    const F u = y.dbl();
    const F v = u * u;
    const F w = u * v;
    const F s = x * v;
    const F xx = x * x;
    const F m = xx.dbl() + xx;
    const F x3 = m * m - s.dbl();
    const F y3 = m * (s - x3) - w * y;
    x = x3;
    y = y3;
    zz = zz * v;
    zzz = zzz * w;
  }
  // add-2008-s: identity on either side, P == Q -> the doubling, P == -Q -> the identity
  void add(const HostPoint4& o) {
    if (o.is_identity()) return;
    if (is_identity()) {
      *this = o;
      return;
    }
    const F u1 = x * o.zz, u2 = o.x * zz;
    const F s1 = y * o.zzz, s2 = o.y * zzz;
    const F d = u2 - u1, r = s2 - s1;
    if (d.is_zero()) {
      if (r.is_zero())
        dbl_in_place();
      else
        *this = identity();
      return;
    }
    const F pp = d * d;
    const F ppp = d * pp;
    const F q = u1 * pp;
    const F x3 = r * r - ppp - q.dbl();
    const F y3 = r * (q - x3) - s1 * ppp;
    x = x3;
    y = y3;
    zz = zz * o.zz * pp;
    zzz = zzz * o.zzz * ppp;
  }
};

// One bucket set's end of the bit-sliced reduction: slices[0] = the root (sum of all buckets), slices[1 + l] = O_l for l < L, in
// the form the device stores (XYZZW).  out = root + sum_l 2^l O_l, as the device's combine leaves it (XYZZW; another
// representative of the same point).  One thread: only the operation count matters, so Horner from the top -- L - 1 doublings
// and L additions -- and not the device's pairwise order.
template <int FID> inline void combine_slices(const XYZZW* slices, uint32_t L, XYZZW* out) {
  using P = HostPoint4<FID>;
  P acc = L ? P::load(slices[L]) : P::identity();
  for (uint32_t l = L; l-- > 1;) {
    acc.dbl_in_place();
    acc.add(P::load(slices[l]));
  }
  acc.add(P::load(slices[0]));
  acc.store(*out);
}

}  // namespace nmx
