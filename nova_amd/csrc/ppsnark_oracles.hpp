// ppsnark_oracles.hpp -- the two N-sized steps of the pre-processing SNARK's prover (src/spartan/ppsnark.rs of the reference) between its
// witness and its batched inner sum-check (sumcheck_ppsnark.hpp) that nothing else in the C ABI can express, on vectors resident in HBM:
//     gather       R1CSShapeSparkRepr::evaluation_oracles (ppsnark.rs:220-253)   out[i] = mem[addr[i]]      (L_row = eq[row], L_col = z[col])
//     mem_oracles  MemorySumcheckInstance::compute_oracles (ppsnark.rs:371-489) without its four commitments, for k memories at once:
//                      t_plus_r[i] = mem[i] gamma + i + r          t_plus_r_inv[i] = ts[i] / t_plus_r[i]
//                      w_plus_r[i] = L[i] gamma + addr[i] + r      w_plus_r_inv[i] = 1 / w_plus_r[i]
// Included at the end of fieldvec.hip (after mercury.hpp, whose arena helper it uses).  The lane bodies use no wave-level intrinsic, so
// tests/host_emul/ppsnark_oracles_emul.cpp runs them on the CPU (simt.hpp).
//
// The gather is one lane per element: the address words are brought to an integer (Montgomery words by ONE product with 32), checked
// against n_mem (and, Montgomery words, against p) BEFORE anything is read through them, and the 32 bytes are copied as they are.  A lane
// that refuses its address raises one device word and reads nothing; the host reads the word after the launch (NMX_E_ARG).
//
// The oracles are Montgomery's trick (batch_invert, fieldvec.hip) over the 2 k n values [T_0 | W_0 | T_1 | W_1 | ...] as ONE batch -- one
// chain of levels and one host round trip for all memories -- with level 0 fused with the hashing and with the product by ts:
//     forward   a lane owns a strided chunk of ONE segment (segment s = 2 m + kind, kind 0 = T, 1 = W): its elements are cl, cl + Tn,
//               cl + 2 Tn, ... < n with Tn = ceil(n / K) chunks per segment, K = binv_chunk(2 k n).  For each it computes x from the inputs,
//               stores x canonical into t_plus_r / w_plus_r, stores the running prefix product into the matching *_inv output and multiplies
//               x in; the chunk's product goes to the arena (chunk s Tn + cl of 2 k Tn).
//     above     levels >= 1 and the host top are batch_invert's own (binv_levels): BatchInvFwdFn / BatchInvBwdFn over the chunk products.
//     backward  re-reads x from t_plus_r / w_plus_r and the prefix from the *_inv output and writes the inverse; a T chunk multiplies by ts.
// Chunks never straddle a segment: a chunk is all T or all W, so the form factor of the ts product (below) is paid once per T CHUNK, and no
// index is mapped per element (one division per lane).  When n is no multiple of Tn the chunks cl >= n mod Tn are one element shorter.
//
// Forms.  F = 1 for canonical words, 2^256 for Montgomery words (NMX_SCALARS_MONT); R = 2^261 is the multiplier's own factor, a (x) b =
// a b / R.  gamma is in the internal form (gamma R), so mem (x) gamma is in mem's form; r is in the vectors' form; i enters as i F: the
// chunk's first index by one product, small(cl) (x) (F R), and every further one by adding the constant Tn F.  The levels hand every
// chunk c_inv = F^2 / P for its stored product P, which walks down to F^2 / X = F / x per element: the inverse in the vectors' form.  The
// product with a stored ts = ts F needs the factor R / F once more: a T chunk starts from c_inv (x) (R^2 / F) (R2 canonical, C266
// Montgomery -- the constant k of CrossTermFn), which every inverse of the chunk inherits, and (acc (x) prefix) (x) ts lands in the vectors' form.
//
// Bounds (p = the modulus; a product of operands below a p and b p with a b < 127 is normalised and below p (1 + a b / 127); stored words
// are taken to be below p, the header's default, and nothing worse than a wrong residue happens below 2^256 < 6 p):
//   hash      in (< 6 p) (x) gamma (canonical) < 1.05 p; + i F (canonical) or addr (< 6 p); + r (canonical): < 8.05 p < 16 p, three
//             normalised addends: limbs < 3 * 2^29 -> norm().canon(): what is stored
//   index     small(cl) (< 2^32) (x) (F R canonical) < 1.01 p -> canon(); iF + Tn F: two canonical values, < 2 p -> norm().canon4()
//   forward   acc (< 1.01 p) (x) x (canonical) < 1.01 p, never reduced further; stored through canon()
//   backward  acc canonical after every step (as BatchInvBwdFn); acc (x) prefix < 1.01 p; (x) ts (< 6 p) < 1.05 p -> canon() in st
// Products per element: T half 1 (hash) + 1 (forward) + 3 (inverse, ts, chain) = 5, plus 2 / K per chunk (index, form factor); W half 4.
// Levels >= 1 add 3 / K of that.  Traffic per element: T half reads mem, ts, x, prefix and writes x, prefix, inverse: 7 x 32 bytes; W half
// reads L, addr, x, prefix and writes three: 7 x 32 bytes too; + 4 x 32 / K for the chunk
// products.  At 3 products per element batch_invert is bound by the multiplier (fieldvec.hip), so this is expected to be as well.
#pragma once

#include "msm_partition.hpp"  // NMX_DEV: the device / emulation spelling
#include "spmv_row.hpp"       // ld / st

namespace nmx {

static constexpr uint32_t kPpsOraMaxMem = 8;

// ---- the gather --------------------------------------------------------------------------------------------------------------------
template <int FID> struct GatherFn {
  const uint32_t *mem, *addr;
  uint32_t *out, *err;  // err: one word, zero before the launch; any lane that refuses its address stores 1
  uint32_t n_mem, mont;
  NMX_HD void operator()(uint32_t i) const {
    using F = Fp<FID>;
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = addr[8 * (size_t)i + j];
    bool ok = true;
    if (mont) {  // a 2^256 -> a: one product with 32; a word >= p is no field element and no address
      ok = F::words_lt_p(w);
      F::from_words(w).mont256_to_canonical().to_words(w);
    }
    uint32_t hi = 0;
#pragma unroll
    for (int j = 1; j < 8; j++) hi |= w[j];
    if (!ok || hi != 0 || w[0] >= n_mem) {  // (covers canonical words >= p: their high words are not zero)
      *err = 1u;
      return;
    }
    const uint32_t* __restrict__ s = mem + 8 * (size_t)w[0];
    uint32_t v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = s[j];
#pragma unroll
    for (int j = 0; j < 8; j++) out[8 * (size_t)i + j] = v[j];
  }
};

// ---- level 0 of the oracles --------------------------------------------------------------------------------------------------------
// the pointer table: four 64-bit addresses per segment s = 2 m + kind
//   kind 0 (T_m): mem[m], ts[m],   out_t_plus_r[m], out_t_plus_r_inv[m]
//   kind 1 (W_m): L[m],   addr[m], out_w_plus_r[m], out_w_plus_r_inv[m]
template <int FID> struct PpsOraArgs {
  const uint64_t* tab;   // 2 k x 4 addresses (device memory)
  uint32_t* chunk;       // 2 k Tn elements: forward writes the chunk products, backward reads the chunk inverses
  Fp<FID> gamma;         // gamma R, canonical
  Fp<FID> r;             // r in the vectors' form, canonical
  Fp<FID> form;          // F R, canonical: small(i) (x) form = i F
  Fp<FID> step;          // Tn F, canonical
  Fp<FID> tscale;        // R^2 / F
  uint32_t n, Tn, K;     // elements per segment, chunks per segment, elements per chunk (Tn = ceil(n / K))
};
template <int FID> NMX_HD Fp<FID> pps_small(uint32_t v) {
  Fp<FID> f = Fp<FID>::zero();
  f.l[0] = v & LIMB_MASK, f.l[1] = v >> LIMB_BITS;
  return f;
}
// chunk c of 2 k Tn -> its segment's pointers
struct PpsOraSeg {
  const uint32_t *in0, *in1;
  uint32_t *x, *inv;
  uint32_t cl, kind;
};
template <int FID> NMX_HD PpsOraSeg pps_ora_seg(const PpsOraArgs<FID>& a, uint32_t c) {
  const uint32_t s = c / a.Tn;
  const uint64_t* t = a.tab + 4 * (size_t)s;
  return {(const uint32_t*)(uintptr_t)t[0], (const uint32_t*)(uintptr_t)t[1], (uint32_t*)(uintptr_t)t[2], (uint32_t*)(uintptr_t)t[3], c - s * a.Tn, s & 1u};
}
template <int FID> struct PpsOraFwdFn {
  PpsOraArgs<FID> a;
  NMX_HD void operator()(uint32_t c) const {
    using F = Fp<FID>;
    const PpsOraSeg g = pps_ora_seg<FID>(a, c);
    F acc = F::one();
    F iF = g.kind ? F::zero() : (pps_small<FID>(g.cl) * a.form).canon();  // cl F
    for (uint32_t j = 0; j < a.K; j++) {
      const uint64_t i = (uint64_t)g.cl + (uint64_t)j * a.Tn;
      if (i >= a.n) break;
      const F h = ld<FID>(g.in0, i) * a.gamma;                                                  // < 1.05 p
      const F x = ((h + (g.kind ? ld<FID>(g.in1, i) : iF)).norm() + a.r).norm().canon();        // < 8.05 p -> canonical
      h.check_below(1.05, "PpsOraFwdFn: in * gamma");
      x.to_words(g.x + 8 * i);
      st<FID>(g.inv, i, acc);
      acc = acc * x;
      iF = (iF + a.step).norm().canon4();  // < 2 p -> canonical (unused on a W chunk)
    }
    st<FID>(a.chunk, c, acc);
  }
};
template <int FID> struct PpsOraBwdFn {
  PpsOraArgs<FID> a;
  NMX_HD void operator()(uint32_t c) const {
    using F = Fp<FID>;
    const PpsOraSeg g = pps_ora_seg<FID>(a, c);
    F acc = ld<FID>(a.chunk, c);
    if (!g.kind) acc = (acc * a.tscale).canon();
    uint32_t cnt = 0;
    while (cnt < a.K && (uint64_t)g.cl + (uint64_t)cnt * a.Tn < a.n) cnt++;
    for (uint32_t j = cnt; j-- > 0;) {
      const uint64_t i = (uint64_t)g.cl + (uint64_t)j * a.Tn;
      const F p = ld<FID>(g.inv, i), x = ld<FID>(g.x, i);
      F o = acc * p;
      if (!g.kind) o = o * ld<FID>(g.in1, i);  // ts
      st<FID>(g.inv, i, o);
      acc = (acc * x).canon();
    }
  }
};

#if defined(__HIPCC__) || defined(__HIP__)
// ---- the host half -----------------------------------------------------------------------------------------------------------------
template <int FID>
static bool gather_t(Ctx& c, const void* mem, size_t n_mem, const void* addr, size_t n, uint32_t flags, void* out) {
  const bool dev = flags & NMX_SCALARS_DEVICE;
  arena_reserve(c, 256 + (dev ? 0 : pad256(n_mem * 32) + 2 * pad256(n * 32)) + 256);
  if (!c.pinned) HIPCHK(hipHostMalloc((void**)&c.pinned, DeviceBackend::kPinnedBytes, hipHostMallocDefault));
  MercuryArena ws{c};
  uint32_t* err = (uint32_t*)ws.take(256);
  volatile uint32_t* land = (volatile uint32_t*)c.pinned;
  *land = 1u;
  const bool prof = G.profiling;
  DeviceBackend be(c, false, prof);
  try {
    be.memset0(err, 4);
    const uint32_t* dmem = ws.in(mem, n_mem, dev);
    const uint32_t* daddr = ws.in(addr, n, dev);
    uint32_t* dout = dev ? (uint32_t*)out : (uint32_t*)ws.take(n * 32);
    be.mark("kernel");
    be.launch(GatherFn<FID>{dmem, daddr, dout, err, (uint32_t)n_mem, (flags & NMX_SCALARS_MONT) ? 1u : 0u}, (uint32_t)n);
    be.mark("end");
    HIPCHK(hipMemcpyAsync((void*)c.pinned, err, 4, hipMemcpyDeviceToHost, c.stream));
    if (!dev) HIPCHK(hipMemcpyAsync(out, dout, n * 32, hipMemcpyDeviceToHost, c.stream));
    stream_wait(c.stream);
  } catch (...) {
    (void)hipStreamSynchronize(c.stream);
    throw;
  }
  if (prof && be.nmarks == 2) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
    prof_store(&ms, 1);
  }
  return *land == 0;
}

// false: some T + r or W + r is zero.  NULLs, k, n, the sizes, the scalars' range and the overlaps are the caller's to check (capi.hip).
template <int FID>
static bool pps_oracles_t(Ctx& c, size_t k, size_t n, const void* const* mem, const void* const* addr, const void* const* Lv, const void* const* ts,
                          const void* gamma, const void* r, uint32_t flags, void* const* o_t, void* const* o_w, void* const* o_tinv,
                          void* const* o_winv) {
  using F = Fp<FID>;
  using H = HostFp4<FID>;
  const bool mont = flags & NMX_SCALARS_MONT, dev = flags & NMX_SCALARS_DEVICE;
  const size_t nv = 2 * k * n;  // < 2^32
  const uint32_t K = binv_chunk(nv);
  const size_t Tn = (n + K - 1) / K;
  // level sizes: the 2 k n values, the 2 k Tn chunk products, then batch_invert's own rule down to at most kBinvHostBelow
  std::vector<size_t> sz{nv, 2 * k * Tn};
  while (sz.back() > kBinvHostBelow) sz.push_back((sz.back() + binv_chunk(sz.back()) - 1) / binv_chunk(sz.back()));
  const size_t Lt = sz.size() - 1;
  size_t need = 256 + 256;
  if (!dev) need += 8 * k * pad256(n * 32);
  for (size_t l = 1; l <= Lt; l++) need += 2 * pad256(sz[l] * 32);  // products (= the level's input) and prefix / inverse arrays, as batch_invert_t
  arena_reserve(c, need);
  if (!c.pinned) HIPCHK(hipHostMalloc((void**)&c.pinned, DeviceBackend::kPinnedBytes, hipHostMallocDefault));
  MercuryArena ws{c};
  uint64_t* dtab = (uint64_t*)ws.take(2 * kPpsOraMaxMem * 4 * 8);
  // the pointer table is built in the pinned buffer past the host level's 2 x 128 elements (binv_levels)
  static_assert(2 * kBinvHostBelow * 32 + 2 * kPpsOraMaxMem * 4 * 8 <= DeviceBackend::kPinnedBytes, "the pointer table lives in the pinned buffer");
  uint64_t* htab = (uint64_t*)(c.pinned + 2 * kBinvHostBelow * 32);
  const F g_i = challenge<FID>(gamma, mont);
  uint32_t rw[8];
  memcpy(rw, r, 32);
  require(F::words_lt_p(rw), NMX_E_SCALAR_RANGE, "challenge >= field modulus");
  uint32_t fw[8], sw[8];
  H::pow2(mont ? 517 : 261).to_canonical(fw);                                      // F R
  (H::from_u64((uint64_t)Tn) * H::pow2(mont ? 256 : 0)).to_canonical(sw);          // Tn F
  std::vector<std::pair<void*, void*>> back;  // (device, host) of the staged outputs
  std::vector<const uint32_t*> in(Lt + 1);
  std::vector<uint32_t*> res(Lt + 1);
  const bool prof = G.profiling;
  DeviceBackend be(c, false, prof);
  bool ok = false;
  try {
    for (size_t m = 0; m < k; m++) {
      uint64_t* e = htab + 8 * m;
      auto outp = [&](void* p) {
        if (dev) return (uint64_t)(uintptr_t)p;
        char* d = ws.take(n * 32);
        back.push_back({d, p});
        return (uint64_t)(uintptr_t)d;
      };
      e[0] = (uint64_t)(uintptr_t)ws.in(mem[m], n, dev), e[1] = (uint64_t)(uintptr_t)ws.in(ts[m], n, dev);
      e[2] = outp(o_t[m]), e[3] = outp(o_tinv[m]);
      e[4] = (uint64_t)(uintptr_t)ws.in(Lv[m], n, dev), e[5] = (uint64_t)(uintptr_t)ws.in(addr[m], n, dev);
      e[6] = outp(o_w[m]), e[7] = outp(o_winv[m]);
    }
    HIPCHK(hipMemcpyAsync(dtab, htab, 2 * k * 4 * 8, hipMemcpyHostToDevice, c.stream));
    // level 0 has no input vector and no result vector of its own (in[0] / res[0] stay unused); level 1's input is its chunk products
    in[0] = nullptr, res[0] = nullptr;
    for (size_t l = 1; l <= Lt; l++) {
      in[l] = (const uint32_t*)ws.take(sz[l] * 32);
      res[l] = (uint32_t*)ws.take(sz[l] * 32);
    }
    PpsOraArgs<FID> a;
    a.tab = dtab, a.chunk = (uint32_t*)in[1];
    a.gamma = g_i, a.r = F::from_words(rw), a.form = F::from_words(fw), a.step = F::from_words(sw);
    a.tscale = mont ? F::from_limbs(FpParams<FID>::C266) : F::from_limbs(FpParams<FID>::R2);
    a.n = (uint32_t)n, a.Tn = (uint32_t)Tn, a.K = K;
    be.mark("kernel");
    be.launch(PpsOraFwdFn<FID>{a}, (uint32_t)sz[1]);
    ok = binv_levels<FID>(c, be, sz, in, res, 1, mont);
    if (ok) {
      a.chunk = res[1];
      be.launch(PpsOraBwdFn<FID>{a}, (uint32_t)sz[1]);
      be.mark("end");
      for (auto& b : back) HIPCHK(hipMemcpyAsync(b.second, b.first, n * 32, hipMemcpyDeviceToHost, c.stream));
    }
    stream_wait(c.stream);
  } catch (...) {
    (void)hipStreamSynchronize(c.stream);  // nothing of this call still reads or writes the caller's vectors
    throw;
  }
  if (ok && prof && be.nmarks == 2) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
    prof_store(&ms, 1);
  }
  return ok;
}

bool fv_gather(Ctx& c, int field, const void* mem, size_t n_mem, const void* addr, size_t n, uint32_t flags, void* out) {
  return with_field(field, [&](auto F) { return gather_t<F()>(c, mem, n_mem, addr, n, flags, out); });
}
bool fv_ppsnark_mem_oracles(Ctx& c, int field, size_t k, size_t n, const void* const* mem, const void* const* addr, const void* const* L,
                            const void* const* ts, const void* gamma, const void* r, uint32_t flags, void* const* o_t, void* const* o_w,
                            void* const* o_tinv, void* const* o_winv) {
  return with_field(field, [&](auto F) { return pps_oracles_t<F()>(c, k, n, mem, addr, L, ts, gamma, r, flags, o_t, o_w, o_tinv, o_winv); });
}
#endif

}  // namespace nmx
