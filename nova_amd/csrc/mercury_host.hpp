// mercury_host.hpp -- HOST-ONLY: the b-sized algebra of Mercury's batch opening (BDFG20 4.1; generate_batch_evaluate_arg,
// src/provider/mercury.rs:567-770) in HostFp4, between the commitments of nmx_mercury_prove (capi.hip).  Plain C++17 with no HIP call:
// tests/cpp/mercury_host_test.cpp drives it under g++ against the restatement of the reference in Python integers.
//
// The four polynomials g, h, d (b coefficients; h zero-padded, d = g reversed) and s (b - 1) are opened at
//     S_g = {zeta, 1/zeta}   S_h = {zeta, 1/zeta, alpha}   S_s = {zeta, 1/zeta}   S_d = {zeta},     T = {alpha, zeta, 1/zeta}.
// The interpolants g*, h*, s*, d* (:592-614) are the Newton form through those points -- the polynomial the reference's Gaussian
// elimination (UniPoly::from_evals_with_xs) finds, and like it undefined when two points coincide: zeta = 0, zeta^2 = 1, alpha = zeta
// or alpha = 1/zeta are refused (set_points).  Then
//     m(X)  = (X - alpha)(g - g*) + beta (h - h*) + beta^2 (X - alpha)(s - s*) + beta^3 (X - alpha)(X - 1/zeta)(d - d*)        (:619-665)
//     W(X)  = m(X) / (X - alpha) / (X - zeta) / (X - 1/zeta), every remainder zero, b - 1 coefficients                           (:668-677)
//     L(X)  = (z - alpha)(g - g*(z)) + beta (h - h*(z)) + beta^2 (z - alpha)(s - s*(z))
//             + beta^3 (z - alpha)(z - 1/zeta)(d - d*(z)) - (z - alpha)(z - 1/zeta)(z - zeta) W(X)                               (:687-751)
//     W'(X) = L(X) / (X - z), remainder zero, b - 1 coefficients                                                                 (:754-764)
// O(b) products each.  beta = 0 and any z (an interpolation point included) are legal.
#pragma once
#include <stdint.h>

#include <vector>

#include "host_fp4.hpp"

namespace nmx {

template <int FID> struct MercuryOpening {
  using H = HostFp4<FID>;
  using Poly = std::vector<H>;
  Poly g, h, s, d;
  H zeta, zeta_inv, alpha;
  H g_zeta, g_zeta_inv, h_zeta, h_zeta_inv, h_alpha, s_zeta, s_zeta_inv, d_zeta;
  Poly g_star, h_star, s_star, d_star;
  H beta;
  Poly W;
  bool prepared = false;
  Poly Q[4];    // the quotients of the four products of m(X) by (X - alpha)(X - zeta)(X - 1/zeta)   (prepare)
  H rem[4][3];  // ... and the remainder each of the three divisions left

  static H eval(const Poly& f, const H& x) {
    H acc = H::zero();
    for (size_t i = f.size(); i-- > 0;) acc = acc * x + f[i];
    return acc;
  }
  // f <- f - r (the longer of the two lengths)
  static void sub(Poly& f, const Poly& r) {
    if (f.size() < r.size()) f.resize(r.size(), H::zero());
    for (size_t i = 0; i < r.size(); i++) f[i] = f[i] - r[i];
  }
  // f <- f + k r
  static void add_scaled(Poly& f, const Poly& r, const H& k) {
    if (f.size() < r.size()) f.resize(r.size(), H::zero());
    for (size_t i = 0; i < r.size(); i++) f[i] = f[i] + k * r[i];
  }
  // f <- f (X - r)
  static void mul_linear(Poly& f, const H& r) {
    f.push_back(H::zero());
    for (size_t i = f.size() - 1; i > 0; i--) f[i] = f[i - 1] - r * f[i];
    f[0] = H::zero() - r * f[0];
  }
  // f <- f / (X - r), returns the remainder (divide_by_linear_polynomial, :281-288)
  static H div_linear(Poly& f, const H& r) {
    if (f.empty()) return H::zero();
    for (size_t i = f.size() - 1; i-- > 0;) f[i] = f[i] + f[i + 1] * r;
    const H rem = f[0];
    f.erase(f.begin());
    return rem;
  }
  // the line through (x0, y0), (x1, y1); x0 != x1
  static Poly line(const H& x0, const H& y0, const H& x1, const H& y1) {
    const H c1 = (y1 - y0) * (x1 - x0).inv();
    return {y0 - c1 * x0, c1};
  }
  // the parabola through three points with distinct abscissae (Newton's divided differences, expanded)
  static Poly parabola(const H& x0, const H& y0, const H& x1, const H& y1, const H& x2, const H& y2) {
    const H f01 = (y1 - y0) * (x1 - x0).inv(), f12 = (y2 - y1) * (x2 - x1).inv();
    const H f012 = (f12 - f01) * (x2 - x0).inv();
    return {y0 - f01 * x0 + f012 * x0 * x1, f01 - f012 * (x0 + x1), f012};
  }

  // false: two interpolation points coincide (zeta = 0 included: it has no inverse)
  bool set_points(const H& zeta_, const H& alpha_) {
    zeta = zeta_, alpha = alpha_;
    if (zeta.is_zero()) return false;
    zeta_inv = zeta.inv();
    return !(zeta == zeta_inv) && !(alpha == zeta) && !(alpha == zeta_inv);
  }
  // b elements of g and h, b - 1 of s, 32 bytes each in the caller's form; d = g reversed (:1113-1120)
  void load(const uint8_t* gw, const uint8_t* hw, const uint8_t* sw, size_t b, bool mont) {
    auto get = [&](const uint8_t* w, size_t n) {
      Poly f(n);
      for (size_t i = 0; i < n; i++) f[i] = mont ? H::from_mont256(w + 32 * i) : H::from_canonical(w + 32 * i);
      return f;
    };
    g = get(gw, b), h = get(hw, b), s = get(sw, b - 1);
    d.assign(g.rbegin(), g.rend());
  }
  void set_evals(const H& gz, const H& gzi, const H& hz, const H& hzi, const H& ha, const H& sz, const H& szi, const H& dz) {
    g_zeta = gz, g_zeta_inv = gzi, h_zeta = hz, h_zeta_inv = hzi, h_alpha = ha, s_zeta = sz, s_zeta_inv = szi, d_zeta = dz;
    g_star = line(zeta, g_zeta, zeta_inv, g_zeta_inv);
    h_star = parabola(zeta, h_zeta, zeta_inv, h_zeta_inv, alpha, h_alpha);
    s_star = line(zeta, s_zeta, zeta_inv, s_zeta_inv);
    d_star = {d_zeta};
    prepared = false;
  }
  // the evaluations on the host (the library takes them from the device's poly_eval_multi launch; the tests and the check take these)
  void eval_all() {
    set_evals(eval(g, zeta), eval(g, zeta_inv), eval(h, zeta), eval(h, zeta_inv), eval(h, alpha), eval(s, zeta), eval(s, zeta_inv), eval(d, zeta));
  }
  // Everything of W that does not depend on beta: the four products of m(X), each padded to b + 2 coefficients and divided by X - alpha,
  // X - zeta and X - 1/zeta with its three remainders kept.  Division with remainder is linear, so W and the remainders of m are the
  // beta-combinations of these (make_w): 3 b products behind the challenge instead of 10 b.  nmx_mercury_prove runs this on a helper
  // thread under the commitment of quot_f.
  void prepare() {
    Poly pr[4] = {g, h, s, d};
    sub(pr[0], g_star), sub(pr[1], h_star), sub(pr[2], s_star), sub(pr[3], d_star);
    mul_linear(pr[0], alpha);
    mul_linear(pr[2], alpha);
    mul_linear(pr[3], alpha), mul_linear(pr[3], zeta_inv);
    const size_t len = pr[3].size();  // b + 2: the longest
    for (int i = 0; i < 4; i++) {
      pr[i].resize(len, H::zero());
      rem[i][0] = div_linear(pr[i], alpha);
      rem[i][1] = div_linear(pr[i], zeta);
      rem[i][2] = div_linear(pr[i], zeta_inv);
      Q[i] = std::move(pr[i]);
    }
    prepared = true;
  }
  // W; false: a remainder is not zero (the evaluations do not belong to the polynomials)
  bool make_w(const H& beta_) {
    if (!prepared) prepare();
    beta = beta_;
    const H b2 = beta * beta, b3 = b2 * beta;
    W = Q[0];
    add_scaled(W, Q[1], beta), add_scaled(W, Q[2], b2), add_scaled(W, Q[3], b3);
    bool ok = true;
    for (int j = 0; j < 3; j++) ok &= (rem[0][j] + beta * rem[1][j] + b2 * rem[2][j] + b3 * rem[3][j]).is_zero();
    return ok;
  }
  // W' for the challenge z; false: the remainder is not zero
  bool make_w_prime(const H& z, Poly& out) const {
    const H b2 = beta * beta, b3 = b2 * beta;
    const H t1 = z - alpha, t4 = t1 * (z - zeta_inv), t = t4 * (z - zeta);
    auto shifted = [&](const Poly& f, const Poly& star, const H& k) {  // k (f - star(z))
      Poly r = f;
      if (r.empty()) r.push_back(H::zero());
      r[0] = r[0] - eval(star, z);
      for (H& c : r) c = c * k;
      return r;
    };
    Poly L = shifted(g, g_star, t1);
    sub(L, shifted(h, h_star, H::zero() - beta));
    sub(L, shifted(s, s_star, H::zero() - b2 * t1));
    sub(L, shifted(d, d_star, H::zero() - b3 * t4));
    add_scaled(L, W, H::zero() - t);
    const bool ok = div_linear(L, z).is_zero();
    out = std::move(L);
    return ok;
  }
  static void store(const Poly& f, bool mont, uint8_t* words) {
    for (size_t i = 0; i < f.size(); i++) {
      if (mont) f[i].to_mont256(words + 32 * i);
      else f[i].to_canonical(words + 32 * i);
    }
  }
};

}  // namespace nmx
