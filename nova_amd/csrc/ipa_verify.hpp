// ipa_verify.hpp -- the field side of the inner-product argument's VERIFIER (InnerProductArgument::verify,
// /root/reference/src/provider/ipa_pc.rs:286-390), included by sumcheck.hip next to ipa.hpp (it uses that file's block sum and
// the provers' pinned mailbox).  The one piece of the verifier that is linear in n is the tensor vector
//     s[i] = prod_k (bit_{ell-1-k}(i) ? r_k : r_k^-1),   i < n = 2^ell                                  (:335-349)
// which is committed against the whole key (ck_hat, :351-354) and dotted with b_vec (:356).  The reference fills it with a
// sequential recurrence (s[i] = s[i - 2^pos] * r_sq[ell - 1 - pos]); here it is born in HBM from its tensor structure:
//   * the index splits into lb = min(ell, 8) low bits and the high rest.  A block builds the table of the low part,
//         T[j] = prod_{pos < lb} (bit_pos(j) ? r : r^-1)_{ell-1-pos},  2^lb entries, internal residue form,
//     by doubling: T[0] = prod r^-1 comes from the host, step pos writes T[j + 2^pos] = T[j] * r^2 for j < 2^pos, one barrier
//     per step -- 255 products for 256 entries;
//   * a block then walks groups of kIpaSTiles consecutive tiles (a tile = 2^lb consecutive indices).  Lanes 0..kIpaSTiles-1 each run
//     the chain of one tile's high factor H = (prod_{pos >= lb} r^-1) * prod_{set bits} r^2: at most ell - lb dependent products,
//     without divergence (the factor is selected, not branched on).  H is kept as a PLAIN integer, so that
//   * every element is ONE product T[j] * H (internal x plain = the plain value), one canonicalisation and one 32-byte store of
//     the canonical integer -- the form the MSM's digit pass reads (no NMX_SCALARS_MONT on that call).
// Lane t of a block owns position t of every tile, so it reads its table entry from LDS once and keeps it in registers; LDS is
// touched by the doubling steps and the high factors only.
// LDS layout: limb-major, word (limb * 256 + j) -- 9 x 256 words = 9 KB.  ds_read_b32 / ds_write_b32 bank on (address / 4) mod 32
// within a 32-lane half, so consecutive j is conflict-free in every doubling step.  Row-major 9-word (36-byte) rows would be
// conflict-free too (odd stride), 8-word (32-byte) rows of packed words are 8-way conflicted for dword access and would need a
// from_words / to_words round trip per step; limb-major is what block_sum uses and needs no padding argument at all.
// The range [lo, lo + cnt) lets each shard of a key over several devices produce its own piece: s, b and the partials are the
// RANGE's arrays (element i of the vector sits at index i - lo).
// With a vector b the same pass loads b[i] (in the form it arrives in) and accumulates b[i] * s[i] lazily: a product of a stored
// element (< 2^256 <= 4.1 p) and a canonical s (< p) is normalised and < 2 p; six of them on top of a canonical accumulator are
// < 13 p < 16 p with limbs < 7 * 2^29 < 2^32, which norm() + canon() take -- the cadence of k_ipa_round.  Per block one sum through
// block_sum_waves into pinned host memory; the host adds the partials and multiplies by 2^261 (the raw sum is sum b s / 2^261).
#pragma once

namespace nmx {

static constexpr uint32_t kIpaSTile = 256, kIpaSTileLog2 = 8, kIpaSTiles = 16, kIpaSMaxBlocks = 128;

template <int FID> struct IpaSArgs {
  uint32_t* s;          // cnt elements, canonical integers
  const uint32_t* b;    // cnt elements in the caller's form (WITH_B only)
  uint32_t* partial;    // 8 words per block (WITH_B only)
  Fp<FID> t0;           // prod_{pos < lb} r^-1, internal, canonical representative
  Fp<FID> hs0;          // prod_{pos >= lb} r^-1 as a plain integer < p (1 when lb == ell)
  Fp<FID> rsq[31];      // r_{ell-1-pos}^2 by bit position pos, internal, canonical representative
  uint64_t lo, cnt;
  uint32_t ell, lb;
};

template <int FID> NMX_HD Fp<FID> ipa_s_lds_load(const uint32_t* a, uint32_t stride, uint32_t j) {
  Fp<FID> r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = a[i * stride + j];
  return r;
}
template <int FID> NMX_HD void ipa_s_lds_store(uint32_t* a, uint32_t stride, uint32_t j, const Fp<FID>& v) {
#pragma unroll
  for (int i = 0; i < 9; i++) a[i * stride + j] = v.l[i];
}

// One block's share of s (and of <b, s>): returns the lane's partial sum, canonical.  tab: 9 * kIpaSTile words, hf: 9 * kIpaSTiles.
// No wave-level intrinsic in here: tests/host_emul runs this body on the CPU.
template <int FID, bool WITH_B> NMX_DEV Fp<FID> ipa_s_block(const IpaSArgs<FID>& p, uint32_t* tab, uint32_t* hf) {
  using F = Fp<FID>;
  const uint32_t t = NMX_TID, lb = p.lb, tl = 1u << lb;
  if (t == 0) ipa_s_lds_store<FID>(tab, kIpaSTile, 0, p.t0);
  NMX_SYNC();
  for (uint32_t pos = 0; pos < lb; pos++) {
    if (t < (1u << pos)) ipa_s_lds_store<FID>(tab, kIpaSTile, t + (1u << pos), (ipa_s_lds_load<FID>(tab, kIpaSTile, t) * p.rsq[pos]).canon());
    NMX_SYNC();
  }
  const F mine = ipa_s_lds_load<FID>(tab, kIpaSTile, t & (tl - 1u));
  const uint64_t first_tile = p.lo >> lb, last_tile = (p.lo + p.cnt - 1) >> lb;
  const uint64_t groups = (last_tile - first_tile) / kIpaSTiles + 1;
  F acc = F::zero();
  uint32_t pending = 0;
  for (uint64_t g = NMX_BID; g < groups; g += NMX_GDIM) {
    const uint64_t tile0 = first_tile + g * kIpaSTiles;
    NMX_SYNC();  // the previous group's high factors have been read
    if (t < kIpaSTiles) {
      const uint64_t tile = tile0 + t;
      F x = p.hs0;
      for (uint32_t pos = lb; pos < p.ell; pos++) {
        const F y = x * p.rsq[pos];  // < 2 p: (< 2 p) x (< p)
        if ((tile >> (pos - lb)) & 1u) x = y;
      }
      ipa_s_lds_store<FID>(hf, kIpaSTiles, t, x.canon());
    }
    NMX_SYNC();
    for (uint32_t j = 0; j < kIpaSTiles; j++) {
      const uint64_t i = ((tile0 + j) << lb) | t;
      if (t < tl && i >= p.lo && i - p.lo < p.cnt) {
        const size_t at = (size_t)(i - p.lo);
        const F s = (mine * ipa_s_lds_load<FID>(hf, kIpaSTiles, j)).canon();
        s.to_words(p.s + 8 * at);
        if (WITH_B) {
          acc = acc + F::from_words(p.b + 8 * at) * s;
          if (++pending == 6) {
            acc = acc.norm().canon();
            pending = 0;
          }
        }
      }
    }
  }
  return acc.norm().canon();
}

// blocks of a launch over [lo, lo + cnt): one per group of tiles, at most kIpaSMaxBlocks (then a block walks several groups)
static inline uint32_t ipa_s_blocks(uint64_t lo, uint64_t cnt, uint32_t lb) {
  const uint64_t groups = (((lo + cnt - 1) >> lb) - (lo >> lb)) / kIpaSTiles + 1;
  return (uint32_t)(groups < kIpaSMaxBlocks ? groups : kIpaSMaxBlocks);
}

#if defined(__HIPCC__) || defined(__HIP__)
template <int FID, bool WITH_B> __global__ __launch_bounds__(256) void k_ipa_s(IpaSArgs<FID> p) {
  __shared__ uint32_t tab[9 * kIpaSTile], hf[9 * kIpaSTiles], red[36];
  Fp<FID> x[1] = {ipa_s_block<FID, WITH_B>(p, tab, hf)};
  if (WITH_B) {
    block_sum_waves<FID, 1>(x, red);
    if (threadIdx.x == 0) x[0].to_words(p.partial + 8 * blockIdx.x);
  }
}

// The host half: challenges (ABI form of `flags`) -> r^2, r^-2 (ABI form, for the group side), the kernel's constants, and with an
// evaluation point the closed form b_hat = prod_k ((1 - x_k) r_k^-1 + x_k r_k).  One inversion (Montgomery's trick).
template <int FID> struct IpaVerifyHost {
  using H = HostFp4<FID>;
  std::vector<H> r, rinv;
  static H load(const void* p32, bool mont, const char* what) {
    uint32_t w[8];
    memcpy(w, p32, 32);
    require(Fp<FID>::words_lt_p(w), NMX_E_SCALAR_RANGE, what);
    return mont ? H::from_mont256(p32) : H::from_canonical(p32);
  }
  static void store(const H& x, bool mont, void* out32) {
    if (mont) x.to_mont256(out32);
    else x.to_canonical(out32);
  }
  IpaVerifyHost(const void* rs, uint32_t ell, bool mont) : r(ell), rinv(ell) {
    H all = H::one();
    std::vector<H> pre(ell);
    for (uint32_t k = 0; k < ell; k++) {
      r[k] = load((const uint8_t*)rs + 32 * k, mont, "challenge >= field modulus");
      require(!r[k].is_zero(), NMX_E_ZERO, "a round challenge is zero");  // batch_invert(&r)? fails (ipa_pc.rs:328)
      pre[k] = all;
      all = all * r[k];
    }
    H inv = all.inv();
    for (uint32_t k = ell; k-- > 0;) {
      rinv[k] = inv * pre[k];
      inv = inv * r[k];
    }
  }
  static Fp<FID> plain_limbs(const H& x) {
    uint32_t w[8];
    x.to_canonical(w);
    return Fp<FID>::from_words(w);
  }
  void fill(IpaSArgs<FID>& p) const {
    const uint32_t ell = (uint32_t)r.size();
    p.ell = ell, p.lb = ell < kIpaSTileLog2 ? ell : kIpaSTileLog2;
    H t0 = H::one(), h0 = H::one();
    for (uint32_t pos = 0; pos < ell; pos++) {
      const uint32_t k = ell - 1 - pos;
      (pos < p.lb ? t0 : h0) = (pos < p.lb ? t0 : h0) * rinv[k];
      p.rsq[pos] = (r[k] * r[k]).to_device().canon();
    }
    for (uint32_t pos = ell; pos < 31; pos++) p.rsq[pos] = Fp<FID>::zero();
    p.t0 = t0.to_device().canon();
    p.hs0 = plain_limbs(h0);
  }
};

template <int FID>
static void ipa_verify_s_t(Ctx& c, const void* rs, uint32_t ell, const void* point, uint32_t flags, uint64_t lo, uint64_t cnt, uint32_t* s_out,
                           const uint32_t* b_dev, uint8_t* rsq_abi, uint8_t* rinvsq_abi, uint8_t* bhat_point, const uint32_t** partial_host,
                           uint32_t* blocks_out) {
  using H = HostFp4<FID>;
  using V = IpaVerifyHost<FID>;
  const bool mont = flags & NMX_SCALARS_MONT;
  const V h(rs, ell, mont);
  H bh = H::one();
  if (point) {
    for (uint32_t k = 0; k < ell; k++) {
      const H x = V::load((const uint8_t*)point + 32 * k, mont, "evaluation point >= field modulus");
      bh = bh * ((H::one() - x) * h.rinv[k] + x * h.r[k]);
    }
  }
  for (uint32_t k = 0; k < ell; k++) {
    V::store(h.r[k] * h.r[k], mont, rsq_abi + 32 * k);
    V::store(h.rinv[k] * h.rinv[k], mont, rinvsq_abi + 32 * k);
  }
  if (point) V::store(bh, mont, bhat_point);
  IpaSArgs<FID> p{};
  h.fill(p);
  p.s = s_out, p.b = b_dev, p.lo = lo, p.cnt = cnt;
  const uint32_t blocks = ipa_s_blocks(lo, cnt, p.lb);
  *blocks_out = blocks;
  static_assert(kIpaSMaxBlocks * 32 <= kMailSlots * kPartSlotBytes, "the partials fit the mailbox's partial area");
  if (b_dev) {
    ScDev<FID> m(c, flags);  // (allocates the mailbox on first use)
    p.partial = m.part_dev(0);
    *partial_host = m.part_host(0);
    hipLaunchKernelGGL((k_ipa_s<FID, true>), dim3(blocks), dim3(256), 0, c.stream, p);
  } else {
    *partial_host = nullptr;
    hipLaunchKernelGGL((k_ipa_s<FID, false>), dim3(blocks), dim3(256), 0, c.stream, p);
  }
  HIPCHK(hipGetLastError());
}

// <b, s> in the ABI form of `flags` once the kernel has completed: raw = sum b_stored s / 2^261, so the element (in the form b
// came in) is raw * 2^261 -- from_plain_times multiplies by value(k) / 2^256 and yields the residue the form's store writes back
template <int FID> static void ipa_verify_bhat_t(const uint32_t* area, uint32_t blocks, uint32_t flags, uint8_t* out32) {
  using H = HostFp4<FID>;
  static const H corr[2] = {H::pow2(261u + 256u), H::pow2(261u)};
  const bool mont = flags & NMX_SCALARS_MONT;
  H acc = H::zero();
  for (uint32_t i = 0; i < blocks; i++) acc = acc + H::from_plain_times(area + 8 * (size_t)i, corr[mont ? 1 : 0]);
  if (mont) acc.to_mont256(out32);
  else acc.to_canonical(out32);
}

template <int FID> static void ipa_verify_mul_t(const void* a, const void* b, uint32_t flags, uint8_t* out32) {
  using V = IpaVerifyHost<FID>;
  const bool mont = flags & NMX_SCALARS_MONT;
  V::store(V::load(a, mont, "scalar >= field modulus") * V::load(b, mont, "scalar >= field modulus"), mont, out32);
}

void fv_ipa_verify_s(Ctx& c, int field, const void* rs, uint32_t ell, const void* point, uint32_t flags, uint64_t lo, uint64_t cnt,
                     uint32_t* s_out, const uint32_t* b_dev, uint8_t* rsq_abi, uint8_t* rinvsq_abi, uint8_t* bhat_point,
                     const uint32_t** partial_host, uint32_t* blocks) {
  with_field(field, [&](auto F) { ipa_verify_s_t<F()>(c, rs, ell, point, flags, lo, cnt, s_out, b_dev, rsq_abi, rinvsq_abi, bhat_point, partial_host, blocks); });
}
void fv_ipa_verify_bhat(int field, const uint32_t* partial_host, uint32_t blocks, uint32_t flags, uint8_t* out32) {
  with_field(field, [&](auto F) { ipa_verify_bhat_t<F()>(partial_host, blocks, flags, out32); });
}
void fv_field_mul_host(int field, const void* a, const void* b, uint32_t flags, uint8_t* out32) {
  with_field(field, [&](auto F) { ipa_verify_mul_t<F()>(a, b, flags, out32); });
}
#endif

}  // namespace nmx
