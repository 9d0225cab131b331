/* nova_mi355x.h -- C ABI of libnova_mi355x.so: the MI355X (gfx950) commitment / MSM provider for Nova.
 *
 * Drop-in boundary.  Each entry point names the reference interface it replaces; paths are
 * relative to the reference tree (microsoft/Nova, nova-snark 0.75.0).  The Rust-side binding a maintainer
 * would add (an external `nova-mi355x-sys` shim crate, wired exactly where the optional CUDA `blitzar`
 * backend is wired: src/provider/bn256_grumpkin.rs:43-78, src/provider/blitzar.rs:7-40) is in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; every function returns 0 on success, a negative NMX_E_* otherwise, and
 *     nmx_last_error() gives a thread-local message.  A failed call never writes a (possibly wrong) point.
 *   - field elements: 32 bytes.  Default = canonical little-endian integer < modulus, i.e. the bytes of
 *     `to_repr()` / `to_bytes()` (what blitzar.rs:10 sends).  With the *_MONT flags = the raw in-memory
 *     4 x u64 Montgomery limbs (R = 2^256) of halo2curves (what `SerdeObject::write_raw` moves, ptau.rs:205).
 *   - affine point: x || y, 64 bytes; the identity is the all-zero encoding in both forms
 *     (src/provider/traits.rs:303-312 returns (0, 0, true)).
 *   - results: affine canonical x || y plus an `is_inf` byte -- exactly `to_coordinates()`.
 *   - all functions are thread-safe and re-entrant (the trait methods are static and are called from rayon
 *     worker threads concurrently: src/r1cs/mod.rs:509-512, src/provider/hyperkzg.rs:1062-1065).
 *   - inputs are borrowed for the duration of the call only.
 */
#ifndef NOVA_MI355X_H
#define NOVA_MI355X_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* curve ids: src/provider/bn256_grumpkin.rs:26-33 (bn256, grumpkin), src/provider/pasta.rs:24-31 */
enum { NMX_BN254_G1 = 0, NMX_GRUMPKIN = 1, NMX_PALLAS = 2, NMX_VESTA = 3, NMX_NUM_CURVES = 4 };

/* flags */
enum {
  NMX_SCALARS_MONT = 1u << 0,   /* scalars are raw Montgomery limbs instead of canonical LE            */
  NMX_BASES_MONT = 1u << 1,     /* base coordinates are raw Montgomery limbs instead of canonical LE     */
  NMX_SCALARS_DEVICE = 1u << 2, /* `scalars` is a device (HBM) pointer on the library's device           */
  NMX_BASES_DEVICE = 1u << 3,   /* `bases` is a device pointer (nmx_bases_register only)                 */
  NMX_BASES_PRECOMPUTE = 1u << 5, /* nmx_bases_register / nmx_bases_generate: also build the window tables          */
  NMX_BASES_VALIDATE = 1u << 6,   /* nmx_bases_register*: reject coordinates >= p and points off the curve with
                                     NMX_E_POINT (identity (0,0) passes) -- what read_points enforces on loaded
                                     keys, /root/reference/src/provider/ptau.rs:372-391                            */
                                /* 2^(c*w) * P_i in HBM (W x the key size; c = 17, W = 15 for keys of 2^20 points).    */
                                /* MSMs over >= 4096 points of such a key run all windows into one bucket set. */
  NMX_BASES_NOCACHE = 1u << 7,  /* slice-form calls (nmx_msm, nmx_msm_u64, nmx_msm_batch): do not look the base  */
                                /* array up in / insert it into the slice cache (one-shot arrays)               */
  NMX_SCALARS_SHARDED = 1u << 8, /* shard-resident scalars (nmx_msm_handle, nmx_msm_u64_handle with an explicit max_num_bits,
                                    nmx_commit, nmx_msm_batch_handle): `scalars` is a HOST array of device pointers, one per
                                    piece that nmx_bases_shard_plan(handle, offset, n) reports (= nmx_shard_plan(REGISTERED key
                                    length, devices, offset, n)), in its order; every piece must be device memory on its shard's
                                    GPU and at least count_j scalars long (checked: NMX_E_ARG otherwise); piece j = the `count_j` scalars of the pairs whose bases live on `device_j`, in
                                    the HBM of THAT device -- the reference chunks coefficients and bases together
                                    (src/provider/msm.rs:564-574), so nothing crosses xGMI or PCIe inside the call.  A key on
                                    one device has one piece.  nmx_svec_* allocates vectors in this layout.          */
  NMX_ASYNC = 1u << 9,          /* element-wise field kernels and SpMV on HBM-resident vectors (nmx_field_axpy / _axpy2 /
                                   _cross_term / _cross_term2 / _vec_add, nmx_mle_bind_top, nmx_poly_fold_pairs, nmx_spmv_apply[_pair],
                                   nmx_r1cs_cross_term, nmx_nifs_fold; ignored elsewhere and with
                                   host operands): return once the kernel is ENQUEUED.  The calling host thread's later calls
                                   -- any entry point -- are ordered behind it, and every call that is synchronous (all MSMs
                                   and commitments, all reductions, anything with a host operand) still returns with
                                   everything the thread enqueued before it complete; nmx_sync() waits explicitly.  A vector
                                   written by an asynchronous call must not be handed to ANOTHER host thread, freed or
                                   read by the host before one of the two.  The NIFS chain between two commitments --
                                   Z = W1 + W2, AZ / BZ / CZ, T (src/r1cs/mod.rs:590-622), the folds (1044-1107) -- is the
                                   intended use: five dependent launches with no host wake-up between them.          */
  NMX_IPA_B_IS_POINT = 1u << 10, /* nmx_ipa_verify: `b` is the evaluation point (log2(n) elements, host) instead of U.b_vec */
  NMX_OUT_PARTIAL = 1u << 4     /* write a 128-byte partial sum instead of an affine point: the per-GPU   */
                                /* result of a sharded MSM, input of nmx_point_sum.  Format: extended     */
                                /* Jacobian (X, Y, ZZ, ZZZ), x = X/ZZ, y = Y/ZZZ, each coordinate the     */
                                /* 32-byte LE integer v * 2^261 mod p (the library's internal residue     */
                                /* form), identity <=> ZZ == 0.                                           */
};

/* error codes */
enum {
  NMX_OK = 0,
  NMX_E_ARG = -1,          /* null pointer / bad curve id / bad flags / length mismatch                  */
  NMX_E_NO_DEVICE = -2,    /* no usable HIP device: the library never falls back to a CPU path            */
  NMX_E_HIP = -3,          /* a HIP runtime call failed (message has the hipError string)                 */
  NMX_E_SCALAR_RANGE = -4, /* a canonical scalar >= modulus (from_repr would reject it)                   */
  NMX_E_SMALL_RANGE = -5,  /* a small scalar >= 2^max_num_bits (msm.rs:543-552 would index out of bounds)  */
  NMX_E_HANDLE = -6,       /* unknown / stale base handle, or offset + n beyond the registered key       */
  NMX_E_TOO_LARGE = -7,    /* n * windows >= 2^32                                                         */
  NMX_E_IO = -8,           /* key file cannot be opened / read (PtauFileError::IoError)                    */
  NMX_E_FORMAT = -9,       /* key file header rejected (InvalidHead, UnsupportedVersion, InvalidNumSections,
                              InvalidPrime, InsufficientPowerForG1/G2; ptau.rs:104-151)                    */
  NMX_E_POINT = -10,       /* a loaded point is not canonical or not on the curve (PointNotOnCurve)        */
  NMX_E_ZERO = -11         /* nmx_field_batch_invert: an element is zero (NovaError::InternalError, spartan/mod.rs:103-105) */
};

/* ---- lifetime ------------------------------------------------------------------------------------- */
/* Selects the HIP device for this process (one process per GPU) and creates the stream/workspace pool.
 * Idempotent.  device < 0 => honour LOCAL_RANK, else device 0.  No reference counterpart (the reference is
 * single-address-space); corresponds to blitzar's implicit backend init. */
int nmx_init(int device);
int nmx_shutdown(void);
int nmx_device_count(void);
int nmx_sync(void); /* waits for the calling thread's NMX_ASYNC calls (no-op when there are none) */
/* Several GPUs behind ONE host process (the reference is one address space: its own MSM decomposition is in-process,
 * `par_chunks` + `reduce(identity, +)`, src/provider/msm.rs:564-574,664-676).  After
 * nmx_init_devices(k, flags) the process owns logical devices 0 .. k-1 (HIP devices 0 .. k-1; k == 0: every visible
 * device; k > nmx_device_count(): NMX_E_NO_DEVICE unless NMX_DEVICES_OVERSUBSCRIBE, which maps logical device i to HIP
 * device i mod count -- several shards per GPU, for tests on a 1-GPU box).  Every key of at least `shard_min_n` points
 * (default 2^20, env NMX_SHARD_MIN_N, nmx_set_option("shard_min_n")) registered AFTERWARDS -- nmx_bases_register*,
 * nmx_bases_generate, and the slice cache behind nmx_msm / nmx_msm_u64 / nmx_msm_batch -- is cut into k contiguous shards
 * (shard i = points [i*n/k ...), exactly nova_amd/dist.py shard_range), shard i resident on device i with its own window
 * tables.  An MSM / commit over such a key runs one host thread + stream per shard touched, each producing a 128-byte
 * partial.  The combine step: inside ONE process every shard worker hands its partial to the calling thread
 * in host memory, so the default is the host sum of the k partials (nmx_point_sum: <= 8 additions of ~0.5 us, nothing on a
 * stream).  nmx_set_option("combine", 2) routes it through RCCL instead -- ONE ncclAllGather of the 128-byte partials over
 * xGMI (bound at run time; one rank per GPU, issued by the calling thread inside a group call), then the G-term sum from rank
 * 0's copy -- which exercises the communicator but adds two copies and k stream syncs; the all-gather is the real exchange
 * step in the one-process-per-GPU deployment (nova_amd/dist.py).  No bucket array crosses devices, and the call is still one
 * synchronous C call.
 * Scalars: shard-resident (NMX_SCALARS_SHARDED, nmx_svec_*: each piece already in the HBM of the GPU that holds its bases --
 * the intended form), or one HBM array on logical device 0 (NMX_SCALARS_DEVICE: a shard on another GPU pulls its slice
 * peer-to-peer over xGMI inside the call), or host memory (each GPU pulls its slice over its own PCIe link).
 * Field-vector kernels on plain pointers, keys below the threshold and keys registered from a device pointer stay on logical
 * device 0; nmx_svec_map runs the NIFS kernels shard by shard.  Without this call (or env NMX_DEVICES=k) the library uses one device, as
 * before.  May be called again to change k (keys keep the layout they were registered with). */
#define NMX_DEVICES_OVERSUBSCRIBE 1u
int nmx_init_devices(int count, uint32_t flags);
int nmx_devices_in_use(void); /* logical devices new keys are sharded over (1 = unsharded) */
/* How a key of n_key points is laid out over k devices and which shards a call over key[offset, offset + n) touches:
 * writes up to cap triples (device, offset inside the shard, count) and returns how many the call needs.  Pure host
 * arithmetic (no device needed): the rule the library itself uses. */
int nmx_shard_plan(size_t n_key, int k, size_t offset, size_t n, size_t* out_triples, int cap);
/* The same triples for a REGISTERED key, from the layout it actually has (a key keeps the layout of the device set it was
 * registered under; an unsharded key answers one triple), plus its registered length in *n_key (may be NULL).  This is the
 * plan to cut NMX_SCALARS_SHARDED pieces by: a plan computed from a length that is not the registered one (e.g. a key
 * registered with its blinding point appended has n + 1 points) puts the cut in the wrong place.  Returns the number of
 * triples or a negative error. */
int nmx_bases_shard_plan(uint64_t handle, size_t offset, size_t n, size_t* out_triples, int cap, size_t* n_key);
const char* nmx_last_error(void);
const char* nmx_version(void);

/* ---- commitment-key residency ------------------------------------------------------------------------
 * The reference passes bases as a prefix slice of a long-lived key (`&ck.ck[..v.len()]`,
 * src/provider/pedersen.rs:267, src/provider/hyperkzg.rs:588).  Register the whole key once; every later
 * call addresses bases[offset .. offset + n) of it in HBM.  `handle` 0 is never valid. */
int nmx_bases_register(int curve, const void* bases_xy64, size_t n, uint32_t flags, uint64_t* handle);
/* On-disk keys.  Points in both formats are halo2curves `write_raw` records: x || y as raw
 * R = 2^256 Montgomery limbs, 64 bytes -- the layout NMX_BASES_MONT takes, so the file is streamed to HBM through
 * pinned staging buffers and converted / validated there; NMX_BASES_VALIDATE is always applied (read_points does).
 *  - nmx_bases_register_ptau: HyperKZG `load_setup` (src/provider/hyperkzg.rs:658-674) -> `read_ptau`
 *    (src/provider/ptau.rs:270-436): "ptau" magic, version 1, 11 or 3 sections, header section (n8, prime == base
 *    modulus of `curve`, power with num_g1 <= 2^(power+1) - 1 and num_g2 <= 2^power), then the first num_g1 points
 *    of section 2 become the key.  Section 3 (G2) is left to the host: pairings are outside this library.
 *  - nmx_bases_register_keyfile: Pedersen `load_setup` (src/provider/pedersen.rs:318-340): 12-byte head
 *    "PEDERSEN_KEY", then h, then ck[0 .. n) (the caller passes n already rounded with next_power_of_two as the
 *    reference does); h comes back as canonical x || y in h_xy64.
 * flags: NMX_BASES_PRECOMPUTE. */
int nmx_bases_register_ptau(int curve, const char* path, size_t num_g1, size_t num_g2, uint32_t flags, uint64_t* handle);
int nmx_bases_register_keyfile(int curve, const char* path, size_t n, uint32_t flags, uint64_t* handle,
                               uint8_t* h_xy64);
int nmx_bases_unregister(uint64_t handle);
/* copies registered bases [offset, offset+n) back to the host as canonical x||y (test / key export helper) */
int nmx_bases_read(uint64_t handle, size_t offset, size_t n, void* out_xy64);

/* Synthetic key: P_i = (k0 + i) * G for i in [0, n), generated in HBM (the construction of
 * src/provider/curve_property_tests.rs:186-194; plays the role of the test-utils `setup`,
 * src/provider/hyperkzg.rs:357-376, whose real keys come from the host). */
int nmx_bases_generate(int curve, uint64_t k0, size_t n, uint32_t flags, uint64_t* handle);

/* ---- fixed-base keys ----------------------------------------------------------------------------------
 * The key HyperKZG users make first: CommitmentKey::setup_from_rng (src/provider/hyperkzg.rs:357-410, reached from
 * CommitmentEngine::setup, :565-567) computes ck[i] = tau^i * G for n.next_power_of_two() points with setup_from_tau_direct, or
 * with setup_from_tau_fixed_base_exp -> fixed_base_exp_comb_batch (:443-) from 100 000 points on.  Both calls below make such a
 * key in HBM -- no N-sized host work, no upload -- as N fixed-base multiplications over ONE table T[w][d] = d * 2^(c w) * B of
 * affine points (c = 8 by default: 32 x 255 points; nmx_set_option("fixed_base_c", 4..16)): a lane cuts its scalar into c-bit
 * digits, adds one table entry per non-zero digit with no doubling, and a block of 256 lanes shares one inversion on the way to
 * affine (nova_amd/csrc/fixed_base.hpp).  from_label (hash-to-curve for h) and tau_H on G2 stay on the host: one point each.
 *  - nmx_bases_from_scalars: key[i] = scalars[i] * B.  B = base_xy64 (64 bytes, host, in the form NMX_BASES_MONT names), or the
 *    curve's standard generator when NULL.
 *  - nmx_bases_setup_from_tau: key[i] = tau^i * G, i in [0, n): setup_from_tau_direct / setup_from_tau_fixed_base_exp.  tau32: host,
 *    32 bytes.  The host computes the 31 squarings tau^(2^j); lane i multiplies those the bits of i select.  The caller rounds n
 *    (next_power_of_two) as the reference does.
 * flags: NMX_SCALARS_MONT (the scalars and tau), NMX_SCALARS_DEVICE (from_scalars only: `scalars` is in HBM; such a key stays on
 * logical device 0), NMX_BASES_MONT (the form of base_xy64; from_scalars only), NMX_BASES_PRECOMPUTE (window tables, as for
 * nmx_bases_generate).
 * Errors, with nothing registered and *handle untouched: NMX_E_ARG for n == 0 or n >= 2^31, a NULL handle, scalars or tau32, an
 * unknown curve or a flag that does not apply; NMX_E_POINT for a base that is not canonical, is off the curve or is the identity;
 * NMX_E_SCALAR_RANGE for a scalar or tau >= r (stored words, either form, as nmx_msm_handle treats scalars): tau and host scalars
 * are checked on the host before anything is launched, HBM scalars by the kernel, which reads such a scalar as zero -- no table
 * read depends on it -- and raises a flag.
 * A scalar that is 0 mod r gives the identity, stored as the all-zero x || y; the key then counts as holding identity points, as a
 * registered key with (0, 0) entries does, so MSMs over it stay correct.  The result is an ordinary key handle: nmx_bases_read,
 * nmx_msm_handle, nmx_commit, nmx_bases_unregister, and sharding over the active devices as nmx_bases_generate (shard p of a tau key
 * computes tau^(begin + i) from its own begin). */
int nmx_bases_from_scalars(int curve, const void* base_xy64, const void* scalars, size_t n, uint32_t flags, uint64_t* handle);
int nmx_bases_setup_from_tau(int curve, const void* tau32, size_t n, uint32_t flags, uint64_t* handle);

/* ---- key derived by address -----------------------------------------------------------------------------
 * CommitmentEngineTrait::ck_derive_by_address (src/traits/commitment.rs:177-194; Pedersen src/provider/pedersen.rs:360-381, HyperKZG
 * src/provider/hyperkzg.rs:731-749): from a key ck and n addresses, a key of table_size points
 *     derived[j] = sum of ck[i] over all i < n with addresses[i] == j,
 * the identity where no address matches, so that Comm(L, ck) == Comm(T, derived) for L[i] = T[addresses[i]] (nmx_field_gather): a
 * prover that looks things up commits to the small T instead of the n-sized L.  The reference adds serially on the host; here the
 * key never leaves HBM: one window of a bucket MSM whose digit is the address -- pair sort, bucket bounds, over-long buckets split
 * into tasks, accumulate, strided folds -- stopped before the bucket reduction, every bucket normalised to affine with one shared
 * inversion per block of 256 (nova_amd/csrc/derive_key.hpp).  Skewed addresses (padding: a large share of all points on one index)
 * are the normal case: no lane adds more than lmax points, by default min(4 x mean bucket, n / 2^14) within [32, 1024];
 * nmx_set_option("derive_lmax", 2..1024) overrides it (0: the default; never changes a result).
 *  - ck_handle: any registered key on ONE device; the points used are its first n (the reference's ck[i], i < addresses.len()).
 *  - addresses: n 64-bit words (the reference's usize), a host pointer, or an HBM pointer with NMX_SCALARS_DEVICE.
 *  - *handle: an ordinary key handle of table_size points that owns its memory (unregistering the source changes nothing), whole on
 *    the device of its source: nmx_bases_read, nmx_msm_handle, nmx_commit, nmx_msm_batch_handle, nmx_msm_sparse_handle,
 *    nmx_bases_unregister and a further nmx_bases_derive_by_address all work on it.
 * flags: NMX_SCALARS_DEVICE (the addresses), NMX_BASES_PRECOMPUTE (window tables for the derived key, as for nmx_bases_generate).
 * An index with no address, or one whose points cancel (P and -P), is stored as the all-zero x || y and the key then counts as holding
 * identity points, exactly as nmx_bases_from_scalars marks a key with a zero scalar.  Identity SOURCE points (all-zero rows: a derived
 * key, a key from zero scalars) contribute nothing; this is the one place the call is wider than the reference, which panics on such
 * a key in ck_to_group_elements (pedersen.rs:346-358), and it is what makes a derivation from a derived key work.  n == 0 is allowed
 * (the reference returns Ok): table_size identities.
 * Errors, with nothing registered and *handle untouched: NMX_E_ARG for a NULL handle, NULL addresses with n > 0, table_size == 0,
 * table_size >= 2^31 or n >= 2^31, a flag that does not apply, an address >= table_size (the reference's InvalidIndex: host addresses
 * are checked on the host before a device is touched, HBM addresses by the kernel, which sends such an entry to the trash bucket and
 * raises a flag -- no memory access depends on it, as in nmx_field_gather) and a source key sharded over several devices (out of
 * scope: derive per shard on the caller's side, or register the source with sharding off); NMX_E_HANDLE for an unknown ck_handle and for
 * n larger than the key (the reference's InvalidCommitmentKeyLength); NMX_E_TOO_LARGE when table_size plus the task count leaves 32
 * bits; NMX_E_HIP when the workspace or the key does not fit.  Every check that needs no device precedes the first one that does. */
int nmx_bases_derive_by_address(uint64_t ck_handle, const uint64_t* addresses, size_t n, size_t table_size,
                                uint32_t flags, uint64_t* handle);

/* ---- key algebra ----------------------------------------------------------------------------------------
 * CommitmentKeyExtTrait (src/provider/pedersen.rs:430-529): split_at, combine, fold, scale and reinterpret_commitments_as_ck, the
 * divide-and-conquer interface the reference's inner-product argument is written against (src/provider/ipa_pc.rs:183,194,212-227,255,
 * 294,310,353-363,380), on keys that stay in HBM (nova_amd/csrc/key_ext.hpp).  nmx_ipa_prove / nmx_ipa_verify never fold the key and do
 * not need these; a caller that wants the folded or scaled key itself does.
 *  - nmx_bases_concat: the new key is the concatenation of rows [offsets[j], offsets[j] + lens[j]) of ck_handles[j], j < k, 1 <= k <= 8.
 *    offsets == NULL: all zero.  lens == NULL: every key whole (from its offset to its end).  split_at(n) is two calls with k = 1;
 *    combine is k = 2; ipa_pc.rs's ck_R.combine(&ck_c) is ONE call with the ranges (ck, n/2, n/2) and (ck_c, 0, 1).  The copies are device
 *    to device in the internal form; no point arithmetic is done.  The result counts as holding identity points if ANY source key
 *    does, whether or not the copied rows hold one: conservative (an MSM over it then reads the rows to skip identities), never wrong.
 *  - nmx_bases_fold: fold(w1, w2) (pedersen.rs:484-497): with h = n / 2, out[i] = w1 * ck[offset + i] + w2 * ck[offset + h + i], i < h.
 *    For odd n the last point is ignored, as in the reference (self.ck.len() / 2 both times).
 *  - nmx_bases_scale: scale(r) (pedersen.rs:500-512): out[i] = r * ck[offset + i], i < n.
 *  - reinterpret_commitments_as_ck (pedersen.rs:515-528) needs no call of its own: it is nmx_bases_register over the commitments' x || y.
 * w1, w2 and r are 32-byte HOST values (transcript challenges; there is no HBM form), canonical, or Montgomery words with
 * NMX_SCALARS_MONT.  The host recodes them once into a signed-binary digit stream (the non-adjacent form of r; Solinas' joint sparse form
 * of (w1, w2)) that the kernel arguments carry: one lane per output point, every lane on the same digits, doublings and mixed additions
 * only, one shared inversion per block of 256 on the way to the affine rows.
 * flags: NMX_SCALARS_MONT (fold and scale only), NMX_BASES_PRECOMPUTE (window tables for the result, as for nmx_bases_generate; a folded
 * key that is used for two MSMs and folded again does not want them).  Every other flag, NMX_ASYNC included: NMX_E_ARG.
 * *handle: an ordinary key handle that owns its memory (unregistering a source changes nothing), whole on the device of its source:
 * nmx_bases_read, nmx_msm_handle, nmx_commit, nmx_msm_batch_handle, nmx_msm_sparse_handle, nmx_bases_derive_by_address,
 * nmx_bases_unregister and a further concat, fold or scale all work on it.  An identity SOURCE row (all zero) contributes nothing, as the
 * reference's msm skips it (msm.rs:247-249).  An output that is the identity -- a zero weight, w1 L = -w2 R, an identity row under scale --
 * is stored as the all-zero x || y and the key then counts as holding identity points, exactly as nmx_bases_from_scalars marks a key with
 * a zero scalar.
 * Errors, with nothing registered and *handle untouched: NMX_E_ARG for a NULL handle, a NULL handles array or a NULL weight; k == 0 or
 * k > 8; a zero total length (concat), n == 0 (scale), n < 2 (fold); any length or total >= 2^31; a flag that does not apply; concat
 * sources of different curves or on different devices; a source key sharded over several devices (out of scope, as for
 * nmx_bases_derive_by_address).  NMX_E_SCALAR_RANGE for a weight whose stored words are >= r, checked on the host (the modulus is the
 * key's, so an unknown handle is reported first).  NMX_E_HANDLE for an unknown handle and for a range that leaves its key.  NMX_E_HIP when
 * the key does not fit.  Every check that needs no device precedes the first one that does. */
int nmx_bases_concat(const uint64_t* ck_handles, const size_t* offsets, const size_t* lens, size_t k,
                     uint32_t flags, uint64_t* handle);
int nmx_bases_fold(uint64_t ck_handle, size_t offset, size_t n, const void* w1, const void* w2,
                   uint32_t flags, uint64_t* handle);
int nmx_bases_scale(uint64_t ck_handle, size_t offset, size_t n, const void* r,
                    uint32_t flags, uint64_t* handle);

/* ---- MSM ---------------------------------------------------------------------------------------------
 * DlogGroupExt::vartime_multiscalar_mul (src/provider/traits.rs:79; impls src/provider/bn256_grumpkin.rs:45-47,
 * src/provider/traits.rs:371-377) == msm() (src/provider/msm.rs:225-419):  out = sum_i scalars[i] * bases[i].
 * n == 0 -> identity (msm.rs:228).  Identity bases and zero scalars contribute nothing (msm.rs:247-249).
 *
 * Slice form = the trait's own signature: the reference passes `&ck.ck[..n]` and no handle (pedersen.rs:263-270,
 * hyperkzg.rs:584-591, blitzar.rs:7-20).  The library therefore keeps a SLICE CACHE of resident keys: a call whose
 * `bases_xy64` pointer is the first element of (or lies inside) an array it has seen before runs over the resident
 * copy exactly like nmx_msm_handle -- no upload, no conversion; a longer prefix of the same array re-registers it at the
 * new length, so one resident copy serves `&ck[..n]` for every n.  First and second sight of an array: the key alone;
 * from its third use on it also has its window tables, built from the resident copy (arrays seen once or twice -- IPA's
 * per-round Vecs, ipa_pc.rs:212-230 -- never pay for them; nmx_set_option("cache_table_after")).  Tables that do not
 * fit the cache budget or the HBM left: the key stays resident without them (plain GPU path).
 * The trait is a pure function of the slice, and the cache keeps it one: identity of an array = (curve, layout flag, host
 * address), confirmed on EVERY call from the caller's bytes against the 64-bit hashes of ALL points recorded at upload.
 * Default (option "cache_verify" = 0): every point of the slice is re-hashed on every hit -- slices up to 2048 points before
 * anything is launched; longer ones get a quick look first (first point, last point, eight probes that move from call to call:
 * a freed-and-reused address fails here) and the full pass runs on host pool threads WHILE the GPU computes the MSM (2^20
 * points = 64 MiB, ~1 ms on 8 threads, under a ~2 ms call); the result is handed out only after the pass succeeded, otherwise
 * the entry is dropped, the call repeated on a fresh upload and the stale result discarded (NMX_STAT_CACHE_STALE).  So an
 * in-place edit of even ONE point changes the very next result.  Host cost: one read of the slice per call; the library never
 * runs more than 8 verification workers at a time across ALL callers (concurrent rayon callers share them, the surplus
 * verifies on its calling thread's share only) -- INTEGRATION.md section 2 has the numbers.
 * Opt-in "cache_verify" = 1 (callers whose keys are immutable, which is every caller in the reference tree): the quick look
 * plus a rolling window of max(4096, n/16) consecutive points that continues where the previous call stopped; an in-place edit
 * is then caught within 16 calls instead of at once, and nmx_cache_invalidate is the contract for in-place edits.
 * Arrays shorter than the cache's min_n (default 128 points) and calls with NMX_BASES_NOCACHE are uploaded for the call only.
 * LRU eviction under a byte budget (default: a quarter of the device's HBM), also when an upload runs out of HBM; evicted or
 * invalidated keys stay alive until the calls using them return.  Keys that must never be re-hashed: register them
 * (nmx_bases_register) and call the *_handle forms. */
int nmx_msm(int curve, const void* scalars, const void* bases_xy64, size_t n, uint32_t flags,
            uint8_t* out, uint8_t* out_is_inf);
/* Slice-cache control.  nmx_cache_configure: max_bytes / min_n / max_entries, 0 = leave unchanged. */
int nmx_cache_clear(void);
int nmx_cache_invalidate(const void* bases_xy64);
int nmx_cache_configure(size_t max_bytes, size_t min_n, size_t max_entries);
/* Smallest n for which the shim should send an MSM to the GPU at all (below it: stay on the CPU `msm()`).  The
 * reference issues thousands of tiny MSMs through this same trait -- IPA's CommitmentKeyExtTrait::fold is n/2
 * two-point MSMs per round (src/provider/pedersen.rs:484-497), msm() itself switches to msm_simple for n <= 16
 * (src/provider/msm.rs:233-235) -- and one GPU MSM costs 0.2-0.3 ms whatever its size.  Default 128 (measured
 * cross-over against the CPU oracle), env NMX_MIN_N overrides.  The library itself accepts any n. */
size_t nmx_min_gpu_n(int curve);
/* One-time self-check for the zero-copy layouts (NMX_BASES_MONT / NMX_SCALARS_MONT): the shim passes the raw
 * in-memory bytes of the curve's standard generator (`G1Affine::generator()`, 64 bytes) and of the scalar
 * `Scalar::from(value)` (32 bytes); returns NMX_OK iff they are x*2^256 mod p little-endian limbs as the *_MONT
 * flags assume (halo2curves does not promise repr(C)), NMX_E_FORMAT otherwise.  Pure host code. */
int nmx_check_layout(int curve, const void* generator_raw64, const void* scalar_raw32, uint64_t value);
/* Monotonic counters of this process (cap >= NMX_STAT_COUNT entries are written; returns NMX_STAT_COUNT). */
enum {
  NMX_STAT_CACHE_HITS = 0,    /* slice-form calls served by a resident key                                   */
  NMX_STAT_CACHE_UPLOADS = 1, /* keys uploaded into the slice cache (first sight, or content mismatch)        */
  NMX_STAT_CACHE_REGROWS = 2, /* of those: re-registrations because a longer prefix of a known array arrived  */
  NMX_STAT_CACHE_EVICTIONS = 3,
  NMX_STAT_CACHE_ENTRIES = 4, /* current                                                                      */
  NMX_STAT_CACHE_BYTES = 5,   /* current HBM bytes held by the slice cache (keys + tables)                    */
  NMX_STAT_UNCACHED_CALLS = 6,/* slice-form calls that uploaded their bases for the call only                 */
  NMX_STAT_BASE_BYTES_H2D = 7,/* bytes of base points copied host -> device by slice-form calls               */
  NMX_STAT_MSM_CALLS = 8,     /* MSMs run (every entry point; a batch counts each vector)                     */
  NMX_STAT_FUSED_RUNS = 9,    /* batch calls whose short vectors ran as one fused pipeline run                */
  NMX_STAT_SHARDED_CALLS = 10,/* MSMs that fanned out over the shards of a multi-device key                   */
  NMX_STAT_CACHE_STALE = 11,  /* slice-form calls whose rolling content check caught an in-place edit of a cached
                                 array: the entry was dropped and the call repeated on a fresh upload          */
  NMX_STAT_TABLE_FALLBACKS = 12, /* keys left without window tables because the tables did not fit (budget / HBM) */
  NMX_STAT_LAUNCH_GAP_NS = 13, /* gauge: cost of one dependent one-wave launch on this box, measured once: a box
                                  diagnostic (slow-launch boxes of a pool show here); 0 until the first MSM       */
  NMX_STAT_SCAN_TIMEOUTS = 14, /* suffix-Horner calls whose single-pass scan gave up a look-back wait and were repeated on
                                  the two-pass kernels (never observed; the guard that turns a hang into a slower call) */
  NMX_STAT_SC_TORN_INJECTED = 15, /* option "sc_torn_test" only: deliberately torn challenge lines the host wrote ahead of the whole one */
  NMX_STAT_SC_TORN_REJECTS = 16,  /* ... and waits in which a pre-launched sum-check pass saw such a line and polled past it
                                     (sequence words new, checksum wrong); counted while "sc_torn_test" is on            */
  NMX_STAT_COUNT = 17
};
int nmx_stats(uint64_t* out, int cap);
/* same, bases taken from a registered key */
int nmx_msm_handle(uint64_t handle, size_t offset, const void* scalars, size_t n, uint32_t flags,
                   uint8_t* out, uint8_t* out_is_inf);

/* DlogGroupExt::vartime_multiscalar_mul_small_with_max_num_bits (src/provider/traits.rs:99-106) ==
 * msm_small_with_max_num_bits (src/provider/msm.rs:478-503): scalars are integers < 2^max_num_bits
 * (u8..u64 widened by the caller, `Into<u64>`); max_num_bits == 0 -> identity (msm.rs:489).
 * vartime_multiscalar_mul_small (traits.rs:93-96 / msm.rs:469-475) = this with max_num_bits = bit length of
 * the largest scalar, which nmx_msm_u64 computes itself when max_num_bits == NMX_BITS_AUTO. */
#define NMX_BITS_AUTO 0xffffffffu
int nmx_msm_u64(int curve, const uint64_t* scalars, const void* bases_xy64, size_t n, uint32_t max_num_bits,
                uint32_t flags, uint8_t* out, uint8_t* out_is_inf);
int nmx_msm_u64_handle(uint64_t handle, size_t offset, const uint64_t* scalars, size_t n,
                       uint32_t max_num_bits, uint32_t flags, uint8_t* out, uint8_t* out_is_inf);

/* Sparse commitments over a registered key (src/provider/pedersen.rs:395-427, src/provider/hyperkzg.rs:751-790):
 *   scalars != NULL: commit_sparse's MSM   out = sum_j scalars[j] * ck[indices[j]]
 *   scalars == NULL: commit_sparse_binary / batch_add (src/provider/msm.rs:689-708)   out = sum_j ck[indices[j]]
 * indices are `usize` on the reference side (host pointer); an index >= the key length is NMX_E_HANDLE. */
int nmx_msm_sparse_handle(uint64_t handle, const uint64_t* indices, const void* scalars, size_t k, uint32_t flags,
                          uint8_t* out, uint8_t* out_is_inf);

/* DlogGroupExt::batch_vartime_multiscalar_mul (src/provider/traits.rs:82-90; blitzar override
 * src/provider/blitzar.rs:22-40): k MSMs over one base array, the j-th using bases[..lens[j]]
 * (HyperKZG batch_commit, src/provider/hyperkzg.rs:593-612).  out = k x 64 bytes, out_is_inf = k bytes.
 * The shortest vectors of a batch (up to 32 on a 2^14 .. 2^19-point key, 16 at 2^20 .. 2^21, 256 below 2^14) run as ONE fused pass over the
 * key's window tables with a bucket set per vector; the others run as independent MSMs on concurrent streams.  Keys of >= 2^22
 * points (2^19 buckets per set: nothing beyond pairs fuses) carry a second, narrow table set over their first 2^18 points: the
 * vectors -- and single MSMs / commitments -- that stay inside it run there (option "prefix_tables" = 0: off). */
int nmx_msm_batch(int curve, const void* const* scalar_vecs, const size_t* lens, size_t k,
                  const void* bases_xy64, size_t n_bases, uint32_t flags, uint8_t* out, uint8_t* out_is_inf);
int nmx_msm_batch_handle(uint64_t handle, const void* const* scalar_vecs, const size_t* lens, size_t k,
                         uint32_t flags, uint8_t* out, uint8_t* out_is_inf);
/* DlogGroupExt::batch_vartime_multiscalar_mul_small (src/provider/traits.rs:109-117; CommitmentEngineTrait::batch_commit_small,
 * src/traits/commitment.rs:139-150): k vectors of u64 scalars over prefixes of one base array, the j-th using
 * bases[..lens[j]]; max_num_bits as nmx_msm_u64 (NMX_BITS_AUTO: per vector, from the data; 0: every result is the identity,
 * msm.rs:489).  Vector by vector over the resident key, several in flight. */
int nmx_msm_u64_batch(int curve, const uint64_t* const* scalar_vecs, const size_t* lens, size_t k, const void* bases_xy64,
                      size_t n_bases, uint32_t max_num_bits, uint32_t flags, uint8_t* out_xy64, uint8_t* out_is_inf);
int nmx_msm_u64_batch_handle(uint64_t handle, const uint64_t* const* scalar_vecs, const size_t* lens, size_t k,
                             uint32_t max_num_bits, uint32_t flags, uint8_t* out_xy64, uint8_t* out_is_inf);

/* CommitmentEngineTrait::commit (src/traits/commitment.rs:52-195; Pedersen src/provider/pedersen.rs:263-270,
 * HyperKZG src/provider/hyperkzg.rs:584-591):  out = msm(v, ck[..n]) + h * r.  `h_xy64` / `r` follow the same
 * flags as bases / scalars and are host pointers. */
int nmx_commit(uint64_t ck_handle, const void* v, size_t n, const void* h_xy64, const void* r,
               uint32_t flags, uint8_t* out, uint8_t* out_is_inf);
/* A commitment that runs beside the caller's next calls.  The two MSMs of a folding step do not depend on each other:
 * commit_T reads W2 and X, never comm_W (src/r1cs/mod.rs:590-622), and the RO that absorbed comm_W (src/nova/nifs.rs:53) is
 * squeezed only behind comm_T (:60-63).  So `W.commit(ck)` (src/frontend/r1cs.rs:47) can be BEGUN, `S.commit_T(..)` computed,
 * and comm_W collected before `U2.absorb_in_ro` -- on the reference side a `rayon::join`, here two calls.  Each MSM ends in a
 * latency-bound tail (fold passes, reduce tree) that leaves most of the chip idle; side by side one's tail hides under the
 * other's accumulation (prove_step replay, bench.py --overlap-commits: 1.41 -> 1.1-1.2 ms).
 *   nmx_commit_begin   same arguments as nmx_commit; h_xy64 and r are copied, `v` must stay valid and unchanged until the
 *                      ticket is finished.  The commitment is ordered behind the calling thread's NMX_ASYNC calls like a
 *                      synchronous one would be, and runs on its own context and stream.
 *   nmx_commit_finish  waits, writes out[64] (128 with NMX_OUT_PARTIAL) / out_is_inf and retires the ticket.  Whatever the
 *                      commitment failed with is reported HERE (code and nmx_last_error); an unknown or already finished ticket
 *                      is NMX_E_HANDLE.  Every ticket must be finished (nmx_shutdown waits for the ones that were not and drops
 *                      their results).  nmx_profile_last does not describe these calls. */
int nmx_commit_begin(uint64_t ck_handle, const void* v, size_t n, const void* h_xy64, const void* r, uint32_t flags,
                     uint64_t* ticket);
int nmx_commit_finish(uint64_t ticket, uint8_t* out, uint8_t* out_is_inf);

/* ---- shard-resident vectors (multi-device keys) ----------------------------
 * A field vector laid out like the key it will be committed against: element i lives in the HBM of the device that holds
 * point i of a key of `n_key` points (nmx_shard_plan(n_key, nmx_devices_in_use(), 0, n)), so W, E, T are BORN on the shard
 * that commits them -- the reference chunks coefficients and bases together (src/provider/msm.rs:564-574).  Elements are raw
 * 32-byte words (canonical or Montgomery: the caller's choice, stated per call with NMX_SCALARS_MONT as everywhere else).
 *   nmx_svec_alloc / free / write (host -> shards) / read (shards -> host)
 *   nmx_svec_parts: the pieces (device pointer, element count, HIP device ordinal) for hosts that fill them with their own
 *     kernels; returns the number of pieces
 *   nmx_svec_map: the element-wise NIFS kernels shard by shard, every GPU on its own piece at the same time --
 *     NMX_OP_AXPY  out = in0 + r*in1                       RelaxedR1CSWitness::fold   src/r1cs/mod.rs:1058-1067
 *     NMX_OP_AXPY2 out = in0 + r*in1 + r^2*in2             fold_relaxed               src/r1cs/mod.rs:1096-1101
 *     NMX_OP_CROSS_TERM  out = in0*in1 - u*in2 - in3       commit_T                   src/r1cs/mod.rs:614-620
 *     NMX_OP_CROSS_TERM2 out = in0*in1 - u*in2 - in3 - in4 commit_T_relaxed           src/r1cs/mod.rs:652-659
 *     NMX_OP_VEC_ADD out = in0 + in1                       Z = Z1 + Z2                src/r1cs/mod.rs:590-609
 *     (`challenge` = r or u, host pointer, < p; operands and `out` must share one layout; out may be an operand; operand words are
 *     any 256-bit values read mod p and the output is canonical, as for the nmx_field_* calls below)
 *   nmx_msm_svec / nmx_commit_svec: nmx_msm_handle(key, 0, ..) / nmx_commit over the first n elements, the scalars taken
 *     shard by shard from the vector (it must have been allocated with n_key = the key's length). */
enum { NMX_OP_AXPY = 0, NMX_OP_AXPY2 = 1, NMX_OP_CROSS_TERM = 2, NMX_OP_CROSS_TERM2 = 3, NMX_OP_VEC_ADD = 4 };
int nmx_svec_alloc(size_t n_key, size_t n, uint64_t* svec);
int nmx_svec_free(uint64_t svec);
int nmx_svec_write(uint64_t svec, const void* host_elems32);
int nmx_svec_read(uint64_t svec, void* host_elems32);
int nmx_svec_parts(uint64_t svec, void** dev_ptrs, size_t* counts, int* hip_devices, int cap);
int nmx_svec_map(int field, int op, const uint64_t* in, int n_in, const void* challenge, uint32_t flags, uint64_t out);
int nmx_msm_svec(uint64_t key_handle, uint64_t svec, size_t n, uint32_t flags, uint8_t* out, uint8_t* out_is_inf);
int nmx_commit_svec(uint64_t ck_handle, uint64_t svec, size_t n, const void* h_xy64, const void* r, uint32_t flags,
                    uint8_t* out, uint8_t* out_is_inf);

/* Sum of `count` 128-byte partials (NMX_OUT_PARTIAL results gathered from the ranks of a sharded MSM) into one
 * affine point: the G-term combine of SURVEY.md 8(e) (the reference's rayon `reduce(identity, +)`,
 * src/provider/msm.rs:566-571,667-673). */
int nmx_point_sum(int curve, const uint8_t* partials128, size_t count, uint8_t* out, uint8_t* out_is_inf);

/* ---- field-vector kernels either side of the MSM -------------------------------
 * field ids: 0 = BN254 Fq (Grumpkin scalars), 1 = BN254 Fr (BN254 scalars), 2 = Pasta Fp (Vesta scalars),
 * 3 = Pasta Fq (Pallas scalars).  Vectors are n x 32 bytes; flags: NMX_SCALARS_MONT (vectors and the challenge
 * are raw Montgomery limbs), NMX_SCALARS_DEVICE (every vector pointer incl. `out` is an HBM pointer -- results
 * then stay resident for the next nmx_msm_handle(..., NMX_SCALARS_DEVICE)); the challenge is always a host pointer.
 * OPERAND WORDS.  For nmx_field_axpy, nmx_field_axpy2, nmx_field_cross_term, nmx_field_cross_term2, nmx_field_vec_add,
 * nmx_mle_bind_top, nmx_poly_fold_pairs, nmx_poly_fold_chain, nmx_field_lincomb_powers, nmx_nifs_fold, nmx_svec_map,
 * nmx_sumcheck_eq_sums, nmx_sumcheck_bind_eq_sums, nmx_sumcheck_plain_sums, nmx_field_batch_invert (v), nmx_mle_evaluate (z),
 * nmx_mle_multi_evaluate (zs) and nmx_poly_eval_multi (polys) every 32-byte word of an input VECTOR (eq tables
 * included) may hold ANY 256-bit value w and is read as w mod p; every output word -- vector element, bound table entry, sum or
 * evaluation -- is canonical (< p).  (In the Montgomery layout w stands for w * 2^-256 mod p, whatever w is.)  A CHALLENGE or POINT
 * (r, u, x, xs, s, points; every coordinate of r for nmx_eq_evals_from_points, nmx_mle_evaluate and nmx_mle_multi_evaluate) must be
 * < p: NMX_E_SCALAR_RANGE otherwise, found before anything is launched, and nothing is written. */
enum { NMX_F_BN254_FQ = 0, NMX_F_BN254_FR = 1, NMX_F_PASTA_FP = 2, NMX_F_PASTA_FQ = 3 };
/* out = a + r*b : RelaxedR1CSWitness::fold, W = W1 + r*W2 and E = E1 + r*T (src/r1cs/mod.rs:1058-1067) */
int nmx_field_axpy(int field, const void* a, const void* b, const void* r, size_t n, uint32_t flags, void* out);
/* out = a + r*b + r^2*c : fold_relaxed's E (src/r1cs/mod.rs:1096-1101) */
int nmx_field_axpy2(int field, const void* a, const void* b, const void* c, const void* r, size_t n, uint32_t flags,
                    void* out);
/* out = az*bz - u*cz - e : the cross term T of commit_T (src/r1cs/mod.rs:614-620) */
int nmx_field_cross_term(int field, const void* az, const void* bz, const void* cz, const void* e, const void* u,
                         size_t n, uint32_t flags, void* out);
/* out = az*bz - u*cz - e1 - e2 : the cross term of commit_T_relaxed, two relaxed instances (src/r1cs/mod.rs:652-659;
 * NIFSRelaxed::prove, src/nova/mod.rs:817,833), u = U1.u + U2.u formed by the caller */
int nmx_field_cross_term2(int field, const void* az, const void* bz, const void* cz, const void* e1, const void* e2,
                          const void* u, size_t n, uint32_t flags, void* out);
/* out = a + b : Z = Z1 + Z2 (src/r1cs/mod.rs:590-609) */
int nmx_field_vec_add(int field, const void* a, const void* b, size_t n, uint32_t flags, void* out);
/* batch_invert (src/spartan/mod.rs:54-118; callers: ppsnark's lookup argument src/spartan/ppsnark.rs:430, IPA src/provider/
 * ipa_pc.rs:328): out[i] = 1 / v[i].  A word of v is ANY 256-bit value w, read as w mod p at every n (OPERAND WORDS above); the
 * outputs are canonical.  NMX_E_ZERO when an element is zero mod p -- the words 0, p, 2p, ... below 2^256 -- at every n (the reference
 * returns Err(NovaError::InternalError)); nothing meaningful is written then.  Montgomery's trick level by level on the device
 * (strided 8..32-element chunks per lane), the top <= 128 products (for n <= 128: the elements themselves, reduced mod p first)
 * inverted on the host.  `out` must not overlap `v`. */
int nmx_field_batch_invert(int field, const void* v, size_t n, uint32_t flags, void* out);
/* out[n_out] = parts[0] || parts[1] || ... || 0 ... 0 for vectors that live in HBM: Spartan's `z = [W.W, vec![U.u], U.X].concat()`
 * then `z.resize(2 * num_vars, 0)` (src/spartan/snark.rs:133, 193-196), and -- with one part -- the clones batch_eval_reduce
 * takes of W and E before it binds them (src/spartan/mod.rs:407-410).  Bit i of device_mask: parts[i] is an HBM pointer (else a
 * host pointer: u and X are host scalars); `out` is HBM (NMX_SCALARS_DEVICE required).  Copies on the library's stream, ordered
 * with the calling thread's other calls; NMX_ASYNC applies when every part is in HBM.  k <= 64. */
int nmx_field_concat(int field, const void* const* parts, const size_t* lens, uint64_t device_mask, size_t k, size_t n_out,
                     uint32_t flags, void* out);
/* MultilinearPolynomial::bind_poly_var_top (src/spartan/polys/multilinear.rs:65-84):
 * out[i] = z[i] + r*(z[i + len/2] - z[i]), i < len/2.  `out` may equal `z` (in place, as the reference does). */
int nmx_mle_bind_top(int field, const void* z, size_t len, const void* r, uint32_t flags, void* out);
/* HyperKZG fold step (src/provider/hyperkzg.rs:1085-1095): out[j] = p[2j] + x*(p[2j+1] - p[2j]), j < len/2 */
int nmx_poly_fold_pairs(int field, const void* p, size_t len, const void* x, uint32_t flags, void* out);
/* The whole fold loop of HyperKZG's prove (src/provider/hyperkzg.rs:1085-1095) as one call (round 6): outs[0] = fold(p, xs[0]) of len / 2
 * elements, outs[i] = fold(outs[i - 1], xs[i]) of len >> (i + 1), i < k <= log2(len); the reference runs it with k = ell - 1 and
 * xs[i] = point[ell - i - 1].  len a power of two; xs: k x 32 bytes on the host; outs: k distinct vectors, none of them p.  With
 * NMX_SCALARS_DEVICE the folds of more than 2048 inputs are one launch each and all the shorter ones run in ONE block (each reading
 * its predecessor's output from LDS); NMX_ASYNC as for nmx_poly_fold_pairs.  Same results, fold by fold, as k single calls. */
int nmx_poly_fold_chain(int field, const void* p, size_t len, const void* xs, size_t k, uint32_t flags, void* const* outs);

/* The N-scaling sums of one eq-factored sum-check round (src/spartan/sumcheck.rs:900-1075), over id in [0, len/2)
 * with x0 = X[id], x1 = X[id + len/2] and factor = eqL[id >> shift] * eqR[id & (2^shift - 1)] (first-half rounds,
 * sumcheck.rs:1233-1247) or factor = eqR[id] when eqL == NULL (last half, sumcheck.rs:1249-1251):
 *   mode 3 (A, B, C): out = (sum (a0*b0 - c0)*factor, sum (a1-a0)*(b1-b0)*factor)    cubic_with_three_inputs
 *   mode 2 (A, B):    out = (sum (a0*b0 - 1)*factor,  sum (a1-a0)*(b1-b0)*factor)    cubic_with_two_inputs
 *   mode 1 (A):       out = (sum a0*factor, 0)                                        quadratic_with_one_input
 * out64 = two field elements in the vectors' own form (host pointer).  The O(1) derivation of the round polynomial
 * from these sums and the claim stays on the caller's side (sumcheck.rs:686-753).  Words of A, B, C, eqL, eqR: any 256-bit values,
 * read mod p; the sums are canonical. */
int nmx_sumcheck_eq_sums(int field, int mode, const void* A, const void* B, const void* C, size_t len, const void* eqL,
                         size_t n_eqL, const void* eqR, size_t n_eqR, uint32_t shift, uint32_t flags, uint8_t* out64);
/* One whole prover round in a single pass over HBM-resident tables (NMX_SCALARS_DEVICE required): bind A, B, C with
 * the round challenge r (bind_poly_var_top, src/spartan/polys/multilinear.rs:65-84, called at
 * src/spartan/sumcheck.rs:535-545) AND return the NEXT round's sums (t_0, t_inf) over the bound tables, exactly what
 * nmx_mle_bind_top x3 followed by nmx_sumcheck_eq_sums(mode, outA, outB, outC, len/2, ...) would give; the eq tables
 * are the next round's.  outX may equal X (in place, as the reference binds).  len % 4 == 0.  Words of A, B, C, eqL, eqR: any 256-bit
 * values, read mod p; the bound tables and the sums are canonical; r < p. */
int nmx_sumcheck_bind_eq_sums(int field, int mode, const void* A, const void* B, const void* C, size_t len, const void* r,
                              const void* eqL, size_t n_eqL, const void* eqR, size_t n_eqR, uint32_t shift,
                              uint32_t flags, void* outA, void* outB, void* outC, uint8_t* out64);
/* The sums of one round of the sum-checks WITHOUT an eq factor, over id in [0, len/2), dX = x1 - x0, X(-1) = 2*x0 - x1:
 *   kind 1 (A, B)    quad_prod  out = (sum a0*b0,    sum dA*dB)                  src/spartan/sumcheck.rs:163-186
 *   kind 2 (A, B)    linear     out = (sum a0 - b0,  sum A(-1) - B(-1))          src/spartan/sumcheck.rs:353-378
 *   kind 3 (A, B)    quadratic  out = (sum a0*b0,    sum A(-1)*B(-1))            src/spartan/sumcheck.rs:380-405
 *   kind 4 (A, B, C) cubic      out = (sum a0*b0*c0, sum dA*dB*dC, sum A(-1)*B(-1)*C(-1))   sumcheck.rs:407-443
 * out96 = three field elements (the third is zero for kinds 1-3), host pointer, in the vectors' own form.  Words of A, B, C: any
 * 256-bit values, read mod p; the sums are canonical. */
int nmx_sumcheck_plain_sums(int field, int kind, const void* A, const void* B, const void* C, size_t len, uint32_t flags,
                            uint8_t* out96);
/* ---- Spartan's sum-check provers, ONE call each (BASELINE.json configs[4]; src/spartan/snark.rs:113-260) -------------------
 * A sum-check round is a streaming pass whose size halves every round, followed by a challenge only the host's transcript can
 * produce; at 2^20 the passes are ~0.1 ms and the rest is per-round latency.  So the round LOOP lives behind the boundary: the
 * tables (HBM-resident with NMX_SCALARS_DEVICE -- the intended form; host arrays otherwise: uploaded for the call, the host
 * copies left untouched) are bound in place, the bind of a round is fused with the next round's
 * sums, results reach the host through a polled mailbox in pinned memory, rounds that fit one block are one launch, and the
 * O(1) algebra of a round (derive_from_claim_deg2/1, UniPoly::from_evals_deg3/2, evaluate, EqSumCheckInstance::bound --
 * src/spartan/sumcheck.rs:680-753, 1226-1231, polys/univariate.rs:90-149) runs in the library.  The one thing that stays on the
 * caller's side is the transcript step `transcript.absorb(b"p", &poly); transcript.squeeze(b"c")` (sumcheck.rs:224-227,
 * 481-484, 315-318): the callback receives the round polynomial as UniPoly coefficients (constant term first; the shim builds
 * `UniPoly { coeffs }`, whose to_transcript_bytes drops the linear term itself) and returns the challenge; elements in the
 * vectors' own form (NMX_SCALARS_MONT as everywhere).  A non-zero return aborts the proof (NMX_E_ARG); a challenge >= p is
 * NMX_E_SCALAR_RANGE.  Outputs (any may be NULL): out_polys = rounds x n_coeffs x 32 bytes (what SumcheckProof compresses),
 * out_r = rounds x 32 (the challenges), final evaluations as listed.  The tables' contents after a call are unspecified (partly
 * bound: the reference's are consumed too).  Once the tables hold <= 2^"sc_host_tail" elements (option, default 7 = 128
 * elements, 0..8) the remaining rounds run on the HOST -- a few hundred field products take the host 1-8 us, any kernel round
 * trip 20-25 us; the last device bind lands the tables in pinned memory.  Option "sc_fused_sum" (default 1): a round is one
 * launch, the block that finishes last adds the per-block partials up; 0: pass + one-block sum.  Option "sc_poll_us": how long a round's mailbox is
 * polled before the stream is synchronised instead (default 2000; 0: always synchronise).  Option "sc_side_streams" (default 1): the
 * claims of a prove_batch_eval round are independent passes and run on one stream each; 0: all on the call's stream.  Options
 * "sc_host_parts" (default 1: a pass of <= 64 blocks hands every block's partial sums to the host, which adds them; 0: the last block
 * does) and "sc_quad" (default 1: passes of <= 2^12 indices of the cubic / quad_prod provers spread an index over four lanes) shorten
 * the dependent chain of the small rounds; "sc_prelaunch" (default 1; needs a large-BAR device and sc_poll_us != 0) enqueues the
 * provers' small passes a round early -- the pass waits on the device for its challenge, which the host
 * writes through the BAR -- taking the launch latency off those rounds; results are identical either way.  The 64-byte challenge
 * line carries a sequence word per 16-byte piece and a 64-bit checksum of its payload: the waiting pass accepts it only whole
 * (no store granularity of the write-combining path is assumed; option "sc_torn_test" = microseconds a deliberately torn line is
 * left on the device first, tests only, with NMX_STAT_SC_TORN_INJECTED / _REJECTS).  At most 256 blocks per device wait this way
 * at any time; passes beyond that budget are launched late.  THE TRANSCRIPT CALLBACK MUST NOT SYNCHRONISE THE DEVICE (hipFree,
 * hipDeviceSynchronize, a blocking copy on the NULL stream, a torch operator): a waiting pass is waiting for the challenge the
 * callback is about to return, and a device-wide wait behind it ends only with the pass's 2 s time-out (the call then fails with
 * NMX_E_HIP; nothing wrong is returned).
 *  - nmx_sumcheck_prove_cubic_with_three_inputs == SumcheckProof::prove_cubic_with_three_inputs (sumcheck.rs:446-507) with its
 *    EqSumCheckInstance (sumcheck.rs:593-1253; all sqrt-size eq tables built by one launch): A, B, C of 2^num_rounds elements,
 *    taus = num_rounds elements (host), 4 coefficients per round, out_claims = [A(r), B(r), C(r)].  A tau of zero (or a
 *    challenge that zeroes eq's running product) takes the reference's third-sum fallback (sumcheck.rs:1085-1136).
 *  - nmx_sumcheck_prove_quad_prod == prove_quad_prod (sumcheck.rs:199-249): A, B of 2^num_rounds elements, 3 coefficients per
 *    round, out_claims = [A(r), B(r)].
 *  - nmx_sumcheck_prove_batch_eval == prove_batch_eval (sumcheck.rs:251-353; batch_eval_reduce, src/spartan/mod.rs:377-437):
 *    k <= 16 claims e_i = P_i(x_i), polys[i] of 2^num_rounds[i] elements (BOUND IN PLACE: the reference binds clones,
 *    spartan/mod.rs:407-410 -- pass copies to keep the originals), eq_points[i] = num_rounds[i] elements (host), claims and
 *    coeffs = k elements each (host), 3 coefficients per round over max(num_rounds) rounds, out_finals = [P_i(r_i)].
 * OPERAND WORDS of the three provers: every word of a table, of taus, eq_points, claims and coeffs must be < p (the first round reads
 * the tables as they are; unlike nmx_sumcheck_eq_sums / _bind_eq_sums / _plain_sums above, words >= p are NOT reduced here). */
typedef int (*nmx_transcript_fn)(void* ctx, const uint8_t* coeffs32, size_t n_coeffs, uint8_t* challenge32_out);
int nmx_sumcheck_prove_cubic_with_three_inputs(int field, const void* claim, const void* taus, size_t num_rounds, void* A, void* B,
                                               void* C, uint32_t flags, nmx_transcript_fn transcript, void* ctx, uint8_t* out_polys,
                                               uint8_t* out_r, uint8_t* out_claims);
int nmx_sumcheck_prove_quad_prod(int field, const void* claim, size_t num_rounds, void* A, void* B, uint32_t flags,
                                 nmx_transcript_fn transcript, void* ctx, uint8_t* out_polys, uint8_t* out_r, uint8_t* out_claims);
int nmx_sumcheck_prove_batch_eval(int field, const void* claims, const size_t* num_rounds, void* const* polys,
                                  const void* const* eq_points, const void* coeffs, size_t k, uint32_t flags,
                                  nmx_transcript_fn transcript, void* ctx, uint8_t* out_polys, uint8_t* out_r, uint8_t* out_finals);
/* nmx_sumcheck_prove_batched_cubic == SumcheckProof::prove_batched_cubic (src/spartan/sumcheck.rs:509-577) with
 * EqSumCheckInstance::evaluation_points_batched_cubic and fallback_eval_inf_batched_cubic (sumcheck.rs:749-894):
 *     sum_x eq(tau, x) * sum_i alpha_i (A_i(x) B_i(x) - C_i(x)) = claim
 * for k triples under ONE sum-check (the outer sum-check of several R1CS instances proven together).
 *   field_id    NMX_F_*: the field of every element of the call, the `field` of the provers above.  (Not spelled `field`: the closed list
 *               of tests/test_gpu_bad_field.py names every entry point with an `int field` parameter; this one's refusal of a bad id is
 *               checked in tests/test_sumcheck_batched_abi.py and tests/test_gpu_sumcheck_batched.py.)
 *   As, Bs, Cs  k tables each (host arrays of k pointers), every table 2^num_rounds elements: HBM-resident with NMX_SCALARS_DEVICE (the
 *               intended form), host arrays otherwise (uploaded for the call, the host copies left untouched).  The tables are
 *               BOUND IN PLACE; their contents after the call are unspecified.
 *   taus        num_rounds elements (host); alphas: k elements (host); claim: one element.  NMX_SCALARS_MONT: everything is
 *               Montgomery limbs, otherwise everything is canonical.
 *   transcript  as for the provers above: once per round with the 4 UniPoly coefficients (constant term first).
 *   out_polys   num_rounds x 4 x 32 bytes (exactly what the callback received); out_r: num_rounds x 32 bytes;
 *   out_claims  k x 3 x 32 bytes, [A_i(r), B_i(r), C_i(r)] for i = 0 .. k-1 (the reference's claims[i]).  Any output may be NULL.
 * 1 <= k <= 16 (the cap of nmx_sumcheck_prove_batch_eval: pointers and alphas travel by value in the kernel arguments); k = 0 (the
 * reference's InvalidNumInstances) and k > 16: NMX_E_ARG.  A NULL table, or two of the 3 k tables overlapping in memory:
 * NMX_E_ARG (an alias would corrupt the proof without a sign).  A claim, tau or alpha >= p: NMX_E_SCALAR_RANGE.  All of these
 * are found before anything is launched: the tables are untouched.  A challenge >= p: NMX_E_SCALAR_RANGE; a callback that
 * returns non-zero: NMX_E_ARG; a bad field id: NMX_E_ARG.  On any failure nothing of the call still runs when it returns.
 * A round is the bind + sums pass over all 3 k tables and a one-block final sum into the mailbox; a tau of zero takes the
 * third-sum fallback (one more pass over the high halves).  Options honoured: "sc_host_tail" (once the tables hold <= 2^that
 * many elements the last device bind brings them to the host and the remaining rounds run there) and "sc_poll_us".  The other
 * sc_* options (sc_fused_sum, sc_side_streams, sc_host_parts, sc_quad, sc_prelaunch, sc_resident, sc_torn_test) do NOT affect
 * this call: every pass is launched after its challenge exists, nothing waits on the device for the host. */
int nmx_sumcheck_prove_batched_cubic(int field_id, const void* claim, const void* taus, size_t num_rounds, void* const* As,
                                     void* const* Bs, void* const* Cs, const void* alphas, size_t k, uint32_t flags,
                                     nmx_transcript_fn transcript, void* ctx, uint8_t* out_polys, uint8_t* out_r, uint8_t* out_claims);
/* nmx_sumcheck_prove_ppsnark == RelaxedR1CSSNARK::prove_helper (src/spartan/ppsnark.rs:886-983), the batched inner sum-check of the
 * pre-processing SNARK, with its three SumcheckEngine instances behind the boundary: MemorySumcheckInstance (ppsnark.rs:520-670, claims
 * 0-5, the logUp memory check), InnerBatchedSumcheckInstance (ppsnark.rs:725-786, claims 6-7) and WitnessBoundSumcheck
 * (ppsnark.rs:293-325, claim 8): ONE sum-check of num_rounds rounds over sixteen tables for nine claims batched by coeffs9.
 *   field_id    NMX_F_*, as for nmx_sumcheck_prove_batched_cubic (not spelled `field` for the same reason; the refusal of a bad id is
 *               checked in tests/test_sumcheck_ppsnark_abi.py and tests/test_gpu_sumcheck_ppsnark.py).
 *   tables      host array of NMX_PPS_TABLES = 16 pointers in the order of the enum below (the reference's fields t_plus_r_row,
 *               t_plus_r_inv_row, w_plus_r_row, w_plus_r_inv_row, ts_row, the same five for col, L_row, L_col,
 *               val = val_A + c val_B + c^2 val_C, E, W (padded) and the masked eq table
 *               MaskedEqPolynomial(eq(r_outer), log2 num_vars).evals(): nmx_eq_evals_from_points, then the first 2^m entries zeroed).
 *               Every table holds 2^num_rounds elements: HBM-resident with NMX_SCALARS_DEVICE (the intended form), host arrays
 *               otherwise (uploaded for the call, the host copies left untouched).  The tables are BOUND IN PLACE; their contents
 *               after the call are unspecified.  All sixteen must be distinct and must not overlap (the reference clones ts_row,
 *               ts_col, L_row, L_col, E and W for this purpose): an overlap is NMX_E_ARG.
 *   rhos        num_rounds elements (host): the taus of the memory instance's EqSumCheckInstance;
 *   r_outer     num_rounds elements (host): the taus of the inner instance's E claim (r_outer_full);
 *   claims2     two elements: the initial claims 6 (ABC) and 7 (claim_E); the other seven are zero (ppsnark.rs:521-523, :294-296);
 *   coeffs9     the nine batching coefficients, powers(s, 9) (ppsnark.rs:920-921): the caller squeezes s itself.
 *               NMX_SCALARS_MONT: everything is Montgomery limbs, otherwise everything is canonical.
 *   transcript  once per round (ppsnark.rs:930-970) with the 4 coefficients of UniPoly::from_evals_deg3([e0, e - e0, lead, em1]),
 *               constant term first; its challenge binds all sixteen tables and e becomes poly(r).
 *   out_polys   num_rounds x 4 x 32 bytes (exactly what the callback received); out_r: num_rounds x 32 bytes;
 *   out_finals  16 x 32 bytes: every table's value at r, in table order (a superset of the reference's final_claims).  Any output
 *               may be NULL.
 * The claims: 0, 1 compute_eval_points_linear (tinv, winv) for row and col (sumcheck.rs:356-379); 2, 4
 * evaluation_points_cubic_with_three_inputs (tinv, t, ts) and 3, 5 evaluation_points_cubic_with_two_inputs (winv, w) under eq(rhos)
 * (sumcheck.rs:900-1037); 6 compute_eval_points_cubic (L_row, L_col, val) (sumcheck.rs:416-443); 7
 * evaluation_points_quadratic_with_one_input (E) under eq(r_outer) (sumcheck.rs:1039-1080); 8 compute_eval_points_quadratic
 * (masked_eq, W) (sumcheck.rs:384-407).  A zero rhos[j] or r_outer[j] takes the reference's third-sum fallback for the claims under
 * that eq (sumcheck.rs:1085-1222).
 * Errors found before a device is leased or anything is written: NULL tables, a NULL entry, a NULL scalar pointer, a null callback, a
 * bad field_id, a flag other than NMX_SCALARS_MONT / NMX_SCALARS_DEVICE, two tables that overlap: NMX_E_ARG; num_rounds >= 31:
 * NMX_E_TOO_LARGE; any of the 2 num_rounds + 11 scalars >= p: NMX_E_SCALAR_RANGE.  During the call a challenge >= p is
 * NMX_E_SCALAR_RANGE and a callback that returns non-zero NMX_E_ARG; on any failure nothing of the call still runs when it returns.
 * num_rounds == 0: no round, out_finals holds the sixteen single elements.  Thread-safe and re-entrant like the other provers.
 * A round is four bind + sums passes (memory row, memory col, inner, witness: 18 sums are too many accumulators for one kernel) and a
 * one-block final sum each into four mailbox slots.  Options honoured: "sc_host_tail" and "sc_poll_us", as for
 * nmx_sumcheck_prove_batched_cubic; the other sc_* options do NOT affect this call: every pass is launched after its challenge
 * exists, nothing waits on the device for the host. */
/* table order of nmx_sumcheck_prove_ppsnark */
enum { NMX_PPS_T_ROW = 0, NMX_PPS_TINV_ROW, NMX_PPS_W_ROW, NMX_PPS_WINV_ROW, NMX_PPS_TS_ROW,
       NMX_PPS_T_COL,     NMX_PPS_TINV_COL, NMX_PPS_W_COL, NMX_PPS_WINV_COL, NMX_PPS_TS_COL,
       NMX_PPS_L_ROW, NMX_PPS_L_COL, NMX_PPS_VAL, NMX_PPS_E, NMX_PPS_W, NMX_PPS_MASKED_EQ, NMX_PPS_TABLES = 16 };
int nmx_sumcheck_prove_ppsnark(int field_id, size_t num_rounds, void* const* tables /* 16 */, const void* rhos,
                               const void* r_outer, const void* claims2, const void* coeffs9, uint32_t flags,
                               nmx_transcript_fn transcript, void* ctx, uint8_t* out_polys, uint8_t* out_r,
                               uint8_t* out_finals /* 16 x 32 */);
/* ---- ppsnark's lookup gather and fused logUp oracles: ten of the sixteen tables above, produced in HBM ------------------------------
 * nmx_field_gather: out[i] = mem[addr[i]], i < n -- R1CSShapeSparkRepr::evaluation_oracles (src/spartan/ppsnark.rs:220-253, called from
 * prove at :1154): L_row[i] = eq(r_outer_full)[row[i]] and L_col[i] = z[col[i]].
 *   field_id   NMX_F_* (not spelled `field`, as for the sum-check provers; the refusal of a bad id is checked in
 *              tests/test_ppsnark_oracles_abi.py and tests/test_gpu_ppsnark_oracles.py).
 *   mem        n_mem elements; their 32 bytes are copied as they are.
 *   addr       n FIELD ELEMENTS whose integer values are the addresses -- the form the reference keeps row / col in as committed
 *              polynomials (ppsnark.rs:180-181) and the form nmx_ppsnark_mem_oracles takes them in.  With NMX_SCALARS_MONT the words are
 *              Montgomery limbs (the kernel takes them out of that form with one product); otherwise canonical integers.
 *   flags      NMX_SCALARS_MONT; NMX_SCALARS_DEVICE: mem, addr and out are in HBM, otherwise host arrays staged for the call.  Any other
 *              flag is NMX_E_ARG -- NMX_ASYNC too: the call reads a device error word back and is synchronous.
 * Errors found before a device is touched, with nothing written: a NULL pointer or n_mem == 0 with n > 0, a bad field_id, an unknown flag,
 * out overlapping mem or addr: NMX_E_ARG; n or n_mem >= 2^32: NMX_E_TOO_LARGE.  Found on the device: an address whose value is not
 * below n_mem (the reference panics on the index) -- non-zero high words, and with NMX_SCALARS_MONT words at or above p, included -- is
 * NMX_E_ARG: the kernel reads nothing through such an address, raises one device word, and the host reads that word after the launch.
 * The contents of out are then unspecified (as for nmx_field_batch_invert's failure); nothing of the call still runs when it returns.
 * n == 0: NMX_OK, no launch.  Thread-safe, and ordered behind the calling thread's NMX_ASYNC calls like every synchronous call. */
int nmx_field_gather(int field_id, const void* mem, size_t n_mem, const void* addr, size_t n,
                     uint32_t flags, void* out /* n */);
/* nmx_ppsnark_mem_oracles == MemorySumcheckInstance::compute_oracles (src/spartan/ppsnark.rs:371-489, called from prove at :1197) without
 * its four commitments (those are nmx_commit / nmx_msm_batch_handle over the outputs), for k memories of n elements in ONE call -- the
 * reference has row and col, k = 2, joined under rayon::join.  For memory m and i < n:
 *     out_t_plus_r[m][i]     = mem[m][i] * gamma + i + r                 (the hash of the table entry, ppsnark.rs:389-396; + r :424-428)
 *     out_w_plus_r[m][i]     = L[m][i] * gamma + addr[m][i] + r          (the hash of the lookup, ppsnark.rs:397-401)
 *     out_t_plus_r_inv[m][i] = ts[m][i] / out_t_plus_r[m][i]             (batch_invert, ppsnark.rs:430, then the product by ts, :439-441)
 *     out_w_plus_r_inv[m][i] = 1 / out_w_plus_r[m][i]
 * i enters as a field element in the vectors' form.  All outputs are canonical (< p) in the inputs' form; the four outputs of memory m
 * are exactly tables NMX_PPS_T_ROW + 5 m, NMX_PPS_W_ROW + 5 m, NMX_PPS_TINV_ROW + 5 m and NMX_PPS_WINV_ROW + 5 m of
 * nmx_sumcheck_prove_ppsnark.
 *   field_id   NMX_F_*, as above.
 *   k, n       1 <= k <= 8 memories of n >= 1 elements each.
 *   mem, addr, L, ts, out_*   host arrays of k pointers, one vector of n elements each.  Inputs may alias one another.
 *   gamma, r   one element each, always host pointers.
 *   flags      NMX_SCALARS_MONT: vectors, gamma and r are Montgomery limbs, otherwise canonical.  NMX_SCALARS_DEVICE: every vector,
 *              inputs and outputs, is in HBM; otherwise host arrays staged for the call.  Any other flag is NMX_E_ARG -- NMX_ASYNC
 *              too: the top of the inversion runs on the host.
 * Errors found before a device is touched, with nothing written: a NULL array or entry, a NULL gamma or r, k outside 1 .. 8, n == 0, a
 * bad field_id, an unknown flag, any output overlapping any input or another output: NMX_E_ARG; 2 k n >= 2^32: NMX_E_TOO_LARGE; gamma
 * or r at or above p: NMX_E_SCALAR_RANGE.  Some T + r or W + r zero: NMX_E_ZERO (the reference's batch_invert(..)? is
 * NovaError::InternalError, ppsnark.rs:430); the outputs are then unspecified and nothing of the call still runs when it returns.
 * Vector words are taken to be below p.  Montgomery's trick over the 2 k n values as one batch: level 0 fused with the hashing and the
 * product by ts, the levels above and the host top those of nmx_field_batch_invert (nova_amd/csrc/ppsnark_oracles.hpp). */
int nmx_ppsnark_mem_oracles(int field_id, size_t k, size_t n,
                            const void* const* mem, const void* const* addr, const void* const* L, const void* const* ts,
                            const void* gamma, const void* r, uint32_t flags,
                            void* const* out_t_plus_r, void* const* out_w_plus_r,
                            void* const* out_t_plus_r_inv, void* const* out_w_plus_r_inv);
/* ---- ppsnark's key tables: the Spark representation, its timestamps and the masked eq table, produced in HBM ---------------------------
 * nmx_ppsnark_spark_repr == R1CSShapeSparkRepr::new (src/spartan/ppsnark.rs:117-190) over matrices that are already resident: no N-sized
 * vector is built on the host.  handles are k matrices from nmx_spmv_register, 1 <= k <= 8, all over one field; the reference has k = 3:
 * A, B, C.  With nnz_j the entry count of matrix j, off_j = nnz_0 + .. + nnz_(j-1) and total = off_k, entry e of matrix j is storage index
 * e of its CSR arrays (the order of SparseMatrix::iter, src/r1cs/sparse.rs:332-390, chained in the order of the handles), and its row is
 * the r with indptr[r] <= e < indptr[r + 1].  Every output is n field elements; for i < n:
 *     out_row[i]      the row of entry i - off_j of the matrix j that i falls into; 0 for i >= total          (ppsnark.rs:123-128)
 *     out_col[i]      that entry's column; n - 1 for i >= total (the lookup into the last, zero, entry of z)
 *     out_vals[j][i]  the entry's value if off_j <= i < off_(j+1), else 0                                     (ppsnark.rs:129-151)
 *     out_ts_row[a]   the number of i < n with row[i] == a; out_ts_col[a]: the same for col (timestamp_calc, ppsnark.rs:154-167).  The
 *                     n - total padding elements count at address 0 for rows and n - 1 for columns; each vector sums to n.
 * Integers become field elements as Scalar::from(u64) (ppsnark.rs:170-174): canonical words, or with NMX_SCALARS_MONT the value * 2^256
 * mod p.  Values come out canonical (< p) in the same form, whatever form the matrix was registered in.  In the order of
 * nmx_sumcheck_prove_ppsnark's tables: out_ts_row is NMX_PPS_TS_ROW and out_ts_col is NMX_PPS_TS_COL (and the ts inputs of
 * nmx_ppsnark_mem_oracles); out_row / out_col are the addr inputs of nmx_field_gather (NMX_PPS_L_ROW, NMX_PPS_L_COL) and of
 * nmx_ppsnark_mem_oracles; NMX_PPS_VAL is val_A + c val_B + c^2 val_C over out_vals (nmx_field_axpy2).
 *   n          the caller's N: the library checks it and does not choose it (the reference's formula, ppsnark.rs:118-121, is
 *              ppsnark_spark_size in the Python and C++ wrappers; R1CSShape::pad stays the caller's).  n must be a power of two, n >= total,
 *              and n >= rows_j, n >= cols_j for every j -- every address is then below n, which nmx_field_gather and the memory check need.
 *   flags      NMX_SCALARS_MONT; NMX_SCALARS_DEVICE: the outputs are HBM pointers on logical device 0, where matrices live, otherwise host
 *              arrays filled through staging.  Any other flag is NMX_E_ARG -- NMX_ASYNC too: the call is synchronous.
 *   outputs    any output pointer, any entry of out_vals and out_vals itself may be NULL: a NULL output is not computed.
 * Errors found before a device is leased, with nothing written: NULL handles, k outside 1 .. 8, an unknown flag, n == 0 or no power of
 * two, n below total or below some matrix's rows or columns (the message names the bound), matrices over different fields, two outputs
 * that overlap: NMX_E_ARG; n >= 2^32: NMX_E_TOO_LARGE; an unknown handle: NMX_E_HANDLE.  The matrices are never modified.  Thread-safe,
 * and ordered behind the calling thread's NMX_ASYNC calls like every synchronous call.  One expansion pass, ts_row from differences of
 * indptr, ts_col as a block-aggregated integer histogram (nova_amd/csrc/ppsnark_key.hpp). */
int nmx_ppsnark_spark_repr(const uint64_t* handles, size_t k, size_t n, uint32_t flags,
                           void* out_row, void* out_col, void* const* out_vals /* k */,
                           void* out_ts_row, void* out_ts_col);
/* nmx_masked_eq_evals == MaskedEqPolynomial::evals (src/spartan/polys/masked_eq.rs:57-75, used at src/spartan/ppsnark.rs:284-285):
 * out[2^ell] is what nmx_eq_evals_from_points(field_id, r, ell, flags, out) gives, with the first 2^num_masked_vars entries zero -- table
 * NMX_PPS_MASKED_EQ of nmx_sumcheck_prove_ppsnark (r = r_outer_full, num_masked_vars = log2 num_vars).  r: ell x 32 bytes, host; out:
 * host, or HBM with NMX_SCALARS_DEVICE; NMX_SCALARS_MONT as there; any other flag: NMX_E_ARG.  ell >= 31 or num_masked_vars > ell:
 * NMX_E_ARG (num_masked_vars == ell gives an all-zero table: evals does not assert `<`, WitnessBoundSumcheck::new does); a coordinate
 * r[i] >= p: NMX_E_SCALAR_RANGE; a NULL r with ell > 0, a NULL out or a field_id that is none of NMX_F_*: NMX_E_ARG.  All found before a
 * device is leased; nothing written.  (field_id is not spelled `field`, as for nmx_field_gather: the closed list of
 * tests/test_gpu_bad_field.py; the refusal of a bad id is checked in tests/test_ppsnark_key_abi.py and tests/test_gpu_ppsnark_key.py.) */
int nmx_masked_eq_evals(int field_id, const void* r, size_t ell, size_t num_masked_vars, uint32_t flags, void* out);
/* ---- inner-product argument (the evaluation engine of the secondary curve) -----------------------------------------------------
 * InnerProductArgument::prove (src/provider/ipa_pc.rs:174-281), reached through EvaluationEngine::prove (:69-82) -- the evaluation
 * argument of S2 in CompressedSNARK::prove (src/nova/mod.rs:862-881; Grumpkin / Pallas / Vesta engines, src/provider/mod.rs:38-148).
 * One call runs every round: c_L, c_R (inner_product, :84-90, :207-208), L = commit(ck_R.combine(ck_c), a_L || c_L, 0) and
 * R = commit(ck_L.combine(ck_c), a_R || c_R, 0) (:213-232), the folds of a and b (:237-247).  The reference also folds the key each
 * round -- ck.fold(r^-1, r), n/2 two-point MSMs (src/provider/pedersen.rs:484-497) -- and commits against the folded halves; this
 * library never folds it: round k's L and R are MSMs over the REGISTERED key with scalars a_k[i] * S_k[m] (S_k = the 2^k products of
 * the earlier r_t^(+-1)), one fused two-vector run over the key's window tables.  Same group elements, so the same L, R, challenges
 * and a_hat as the reference's loop (checked against the oracle's key-folding restatement and the reference's verifier,
 * ipa_pc.rs:286-390, in tests/).
 *   ck_handle   the Pedersen key (CommitmentKey::ck), registered; the first n points are used (`ck.split_at(U.b_vec.len())`, :183);
 *               n > its length: NMX_E_HANDLE
 *   ck_c_xy64   host, 64 bytes: the ALREADY SCALED one-point key `ck_c.scale(&r)` (:190-191; the caller's transcript squeezed that r
 *               after absorbing the instance), in the form NMX_BASES_MONT names
 *   a, b        W.a_vec and U.b_vec: n elements each, n a power of two (2^ell evaluations); host, or HBM with NMX_SCALARS_DEVICE;
 *               canonical, or Montgomery limbs with NMX_SCALARS_MONT (then r and a_hat are Montgomery too).  Not modified.
 *   transcript  called once per round with L and R (affine canonical x || y like every result of this library, and whether each is
 *               the identity): absorb(b"L", &L); absorb(b"R", &R); squeeze(b"r") (:231-234); writes r and returns 0.  Non-zero:
 *               NMX_E_ARG; r >= modulus: NMX_E_SCALAR_RANGE; r = 0: NMX_E_ZERO (`r.invert().unwrap()` panics, :235).
 *   out_L, out_R  log2(n) points of 64 bytes each (L_vec, R_vec; canonical x || y); out_is_inf (may be null): 2 log2(n) bytes, [2k] = L_k is the identity,
 *               [2k + 1] = R_k;  out_a_hat: 32 bytes (a_vec[0] after the last fold, :271).  n = 1: no round, a_hat = a[0].
 * Flags: NMX_SCALARS_MONT, NMX_SCALARS_DEVICE, NMX_BASES_MONT; anything else NMX_E_ARG.  On an error the outputs written so far are
 * unspecified and nothing of the call still runs. */
typedef int (*nmx_ipa_transcript_fn)(void* ctx, const uint8_t* L_xy64, int L_is_inf, const uint8_t* R_xy64, int R_is_inf,
                                     uint8_t* r32_out);
int nmx_ipa_prove(uint64_t ck_handle, const void* ck_c_xy64, const void* a, const void* b, size_t n, uint32_t flags,
                  nmx_ipa_transcript_fn transcript, void* ctx, uint8_t* out_L, uint8_t* out_R, uint8_t* out_is_inf, uint8_t* out_a_hat);
/* ---- HyperKZG's evaluation argument (the evaluation engine of the primary curve) -------------------------------------------------
 * EvaluationEngineTrait::prove of HyperKZG (src/provider/hyperkzg.rs:926-1116: prove :1076-1116, kzg_open_batch :1007-1072, kzg_open
 * :1002-1004, div_by_monomial :961-999) as one call, n = 2^ell >= 2 evaluations of hat_P:
 *   1. the ell - 1 pair folds with x[ell - i - 1] (:1085-1095) into the call's workspace     2. one fused batch commitment of the folded
 *   polynomials over the registered key (:1100, blinding 0)     3. STAGE 0 of the callback with the ell - 1 commitments -> r
 *   (compute_challenge, :861-865)     4. u = [r, -r, r^2] (:1106)     5. the whole v matrix in one launch (:1049-1056)     6. STAGE 1 with
 *   the 3 ell scalars of v -> q (get_batch_challenge, :869-880)     7. the three quotients of B = sum q^i f_i in one pass
 *   (nmx_poly_lincomb_quotients; :1059-1065)     8. one batch commitment of the three quotients of n - 1 coefficients (:1062-1065)
 *   9. STAGE 2 with the three w, so that the caller's transcript reaches the state the verifier's will have
 *   (verifier_second_challenge, :1069); whatever the callback writes at this stage is ignored.
 * The pairing check and tau_H stay the caller's.
 *   ck_handle   a registered key on ONE device with at least n points, of any of the four curves (the field is the curve's scalar
 *               field); unknown, shorter than n or sharded over several devices: NMX_E_HANDLE
 *   hat_P       n elements; host, or HBM with NMX_SCALARS_DEVICE; canonical, or Montgomery limbs with NMX_SCALARS_MONT (then the
 *               challenges and v are Montgomery too).  Never modified.
 *   point       host, ell elements, point[0] first as the reference's x; an element >= p: NMX_E_SCALAR_RANGE
 *   transcript  (ctx, stage, data, count, is_inf, out32) -> 0, or non-zero: NMX_E_ARG.  Stage 0: data = count = ell - 1 points, affine
 *               canonical x || y of 64 bytes each (NMX_BASES_MONT: Montgomery limbs), is_inf[i] = point i is the identity; ell = 1:
 *               count = 0 (the reference absorbs the empty vector and squeezes).  Stage 1: data = count = 3 ell scalars of 32 bytes,
 *               row-major (row i = f_i at r, -r, r^2), is_inf = NULL.  Stage 2: data = 3 points, is_inf as in stage 0.  A challenge
 *               written to out32 (stages 0 and 1, in the scalars' form) >= p: NMX_E_SCALAR_RANGE; r = 0 and q = 0 are legal (nothing
 *               is inverted).  The callback runs on the calling thread and MUST NOT synchronise the device (no nmx_sync, no
 *               hipDeviceSynchronize: the restriction of the sum-check callbacks).
 *   out_com, out_com_is_inf   ell - 1 points of 64 bytes and their identity bytes (out_com may be NULL when ell = 1, out_com_is_inf always)
 *   out_v       ell x 3 scalars;   out_w, out_w_is_inf   3 points and their identity bytes (out_w_is_inf may be NULL)
 * Flags: NMX_SCALARS_MONT, NMX_SCALARS_DEVICE, NMX_ASYNC (accepted; the call is synchronous), NMX_BASES_MONT (the form of the points
 * given to the callback and written out); anything else NMX_E_ARG.  n not a power of two or n < 2 (the reference's `0..ell - 1`
 * underflows at ell = 0), a NULL among hat_P, point, transcript, out_com (ell > 1), out_v, out_w: NMX_E_ARG, before a device or a key is
 * touched.  On an error the outputs written so far are unspecified and nothing of the call still runs.  Synchronous, ordered behind the
 * calling thread's NMX_ASYNC calls; thread-safe like nmx_ipa_prove.  Option kzg_fused_quotients: 1 runs step 7 as the one pass, 0 as
 * nmx_field_lincomb_powers + 3 x nmx_poly_suffix_horner, 2 (the default) chooses by size -- the pass from n = 2^20 on, where it is the
 * faster of the two (docs/measurements.md).  The same bytes every way. */
typedef int (*nmx_transcript_fn_kzg)(void* ctx, int stage, const uint8_t* data, size_t count, const uint8_t* is_inf, uint8_t* out32);
typedef nmx_transcript_fn_kzg nmx_kzg_transcript_fn; /* the same type under the name that reads like nmx_ipa_transcript_fn */
int nmx_hyperkzg_prove(uint64_t ck_handle, const void* hat_P, size_t n, const void* point, uint32_t flags, nmx_transcript_fn_kzg transcript,
                       void* ctx, uint8_t* out_com, uint8_t* out_com_is_inf, uint8_t* out_v, uint8_t* out_w, uint8_t* out_w_is_inf);
/* ---- Mercury's evaluation argument (the second evaluation engine of the primary curve) ---------------------------------------------
 * EvaluationEngineTrait::prove of Mercury (src/provider/mercury.rs:891-1268 with batch_evaluation::generate_batch_evaluate_arg,
 * :567-770) as one call: a constant-size proof of eight commitments and six scalars for n = 2^ell evaluations, ell >= 2
 * (assert!(log_n > 1), :914).  Shape (:911-931): ell' = ell rounded up to even, b = 2^(ell' / 2), f viewed as n_rows x b with
 * n_rows = n / b (b, or b / 2 when ell is odd); an odd ell gives the point a leading 0 (:919-923), so eq_row has a zero upper half and h
 * is zero-padded to b for s only; f is never padded.  The caller's transcript has absorbed f, u and e (:905-907) before the call; `eval`
 * is no argument (the prover uses it in debug assertions only).  Steps and callback stages (count and data as in nmx_transcript_fn_kzg):
 *   1. eq_row, eq_col (:937-938); h (nmx_mercury_h_poly's pass, :966); commit h over n_rows coefficients (:987).  STAGE 0: 1 point,
 *      comm_h -> alpha (:988-991)
 *   2. q, g (nmx_mercury_divide_by_binomial's pass, :995); ONE fused batch commitment of q over (n_rows - 1) b coefficients and g over b
 *      (:1046-1049).  STAGE 1: 2 points, comm_q then comm_g as the reference absorbs them (:1050-1051) -> gamma (:1068)
 *   3. s = nmx_mercury_s_poly(eq_col, g, eq_row, h, gamma) (:1072-1077); d = g reversed (:1113-1120); ONE fused batch commitment of s over
 *      b - 1 coefficients and d over b (:1123-1126).  STAGE 2: 2 points, comm_s then comm_d (:1128-1129) -> zeta (:1132)
 *   4. zeta^-1 (:1134); [g, h, s, d] at [zeta, zeta^-1, alpha] in one nmx_poly_eval_multi launch, eight of the twelve values used
 *      (:1136-1159).  STAGE 3: 6 scalars in the order of out_evals (the reference absorbs them under six labels, :1203-1208); what the
 *      callback writes is ignored
 *   5. quot_f (:1163-1180): the quotient pass over [f, q] with weight -(zeta^b - alpha) at the one point zeta (the k = 2, m = 1 case of
 *      nmx_poly_lincomb_quotients, or lincomb_powers + suffix Horner, by the option kzg_fused_quotients); out[0] is compared with g(zeta)
 *      (the reference's assert_eq!(rem, ZERO), :1177: a difference is a library bug, NMX_E_HIP); commit out[1..n) (:1212-1217).
 *      STAGE 4: 1 point, comm_quot_f (:1218) -> beta (:586)
 *   6. the batch opening (BDFG20 4.1, :567-770) on the host, O(b) products: the interpolants g*, h*, s*, d* in closed form (:592-614),
 *      m(X) (:619-665), W = m / (X - alpha) / (X - zeta) / (X - 1/zeta) with every remainder checked (:668-674), b - 1 coefficients;
 *      commit W (:677).  STAGE 5: 1 point, comm_w -> z (:678-682).  L(X) (:687-751), W' = L / (X - z), remainder checked (:754-761);
 *      commit W' (:764).  STAGE 6: 1 point, comm_w_prime (:1249); what the callback writes is ignored (the reference squeezes the
 *      pairing challenge d only to keep the transcripts aligned, :1250).  g, h and s are read back once (32 b bytes each), W and W' are
 *      uploaded for their commitments.
 * Mercury's verify, G2 and tau_H stay the caller's.
 *   ck_handle   a registered key on ONE device with at least n points, of any of the four curves (the field is the curve's scalar
 *               field); unknown, shorter than n or sharded over several devices: NMX_E_HANDLE
 *   poly        n elements; host, or HBM with NMX_SCALARS_DEVICE; canonical, or Montgomery limbs with NMX_SCALARS_MONT (then the
 *               challenges and the evaluations are Montgomery too).  Never modified.
 *   point       host, ell elements, in the reference's order; an element >= p: NMX_E_SCALAR_RANGE
 *   transcript  (ctx, stage, data, count, is_inf, out32) -> 0, or non-zero: NMX_E_ARG.  Points are affine canonical x || y of 64 bytes
 *               (NMX_BASES_MONT: Montgomery limbs) with is_inf[i] = point i is the identity; scalars (stage 3) are 32 bytes each in the
 *               scalars' form with is_inf = NULL.  A challenge written to out32 (stages 0, 1, 2, 4, 5) >= p: NMX_E_SCALAR_RANGE.
 *               zeta = 0 (zeta.invert().unwrap(), :1134), zeta^2 = 1, alpha = zeta or alpha = 1/zeta: NMX_E_ZERO -- the interpolation
 *               points coincide and the reference's elimination has no solution.  alpha = 0, gamma = 0, beta = 0 and any z (an
 *               interpolation point included) are legal.  The callback runs on the calling thread and MUST NOT synchronise the device.
 *   out_comms   8 points of 64 bytes in the order of the fields of EvaluationArgument: comm_h, comm_g, comm_q, comm_s, comm_d,
 *               comm_quot_f, comm_w, comm_w_prime;   out_is_inf   their 8 identity bytes (may be NULL)
 *   out_evals   6 scalars: g_zeta, g_zeta_inv, h_zeta, h_zeta_inv, s_zeta, s_zeta_inv
 * Flags: NMX_SCALARS_MONT, NMX_SCALARS_DEVICE, NMX_ASYNC (accepted; the call is synchronous), NMX_BASES_MONT; anything else NMX_E_ARG.
 * n not a power of two or n < 4, a NULL among poly, point, transcript, out_comms, out_evals: NMX_E_ARG; n >= 2^31: NMX_E_TOO_LARGE; all
 * before a device or a key is touched.  On an error the outputs written so far are unspecified, nothing of the call still runs and the
 * next call on the same key works.  Synchronous, ordered behind the calling thread's NMX_ASYNC calls; thread-safe like
 * nmx_hyperkzg_prove; the workspace is the call's own (the context's aux buffer).  The zero polynomial gives eight identity points. */
int nmx_mercury_prove(uint64_t ck_handle, const void* poly, size_t n, const void* point, uint32_t flags, nmx_transcript_fn_kzg transcript,
                      void* ctx, uint8_t* out_comms /* 8 x 64 */, uint8_t* out_is_inf /* 8 or NULL */, uint8_t* out_evals /* 6 x 32 */);
/* InnerProductArgument::verify (src/provider/ipa_pc.rs:286-390), reached through EvaluationEngine::verify (:80-99) from
 * RelaxedR1CSSNARK::verify (src/spartan/snark.rs:384, ppsnark.rs:1645) inside CompressedSNARK::verify (src/nova/mod.rs:912), from the
 * point where the caller's transcript has produced its challenges: the verifier's transcript never waits for the device (it absorbs
 * L_vec[i], R_vec[i] from the proof and squeezes, :315-321), so there is no callback.  The work linear in n -- the tensor vector
 * s[i] = prod_k (bit_{ell-1-k}(i) ? r_k : r_k^-1) (:335-349), ck_hat = commit(ck, s) (:351-354) and <b_vec, s> (:356) -- runs on the
 * device: s is generated in HBM next to the registered key (one product per element, nova_amd/csrc/ipa_verify.hpp) and never crosses
 * the bus; the O(log n) group side (:358-376) runs on host threads under the MSM.
 *   ck_handle   the Pedersen key, registered; its first n points are used (`ck.split_at(U.b_vec.len())`, :294); n beyond it:
 *               NMX_E_HANDLE.  Keys over several devices work as for nmx_commit.
 *   ck_c_xy64   host, 64 bytes: the ALREADY SCALED one-point key `ck_c.scale(&r)` (:309-310), as nmx_ipa_prove takes it
 *   comm_a_xy64, comm_a_is_inf, c   U.comm_a_vec (may be null when it is the identity) and U.c (32 bytes) (:312-313)
 *   b, n        U.b_vec: n elements, n a power of two below 2^31 (:297-303); host, or HBM with NMX_SCALARS_DEVICE.  With
 *               NMX_IPA_B_IS_POINT: the evaluation point instead, log2(n) elements on the host, point[0] the most significant
 *               variable as in nmx_eq_evals_from_points -- the eq table EvaluationEngine::verify builds (:88) is never materialised:
 *               <eq(point), s> = prod_k ((1 - point_k) r_k^-1 + point_k r_k).  Not modified.
 *   L_xy64, R_xy64   log2(n) points of 64 bytes each (L_vec, R_vec); is_inf (may be null = none): 2 log2(n) bytes in nmx_ipa_prove's
 *               out_is_inf layout; a_hat: 32 bytes.  A proof goes from nmx_ipa_prove into this call unchanged.
 *   rs          log2(n) challenges, host, round 0 first (:315-321).  rs[k] >= modulus: NMX_E_SCALAR_RANGE; rs[k] = 0: NMX_E_ZERO
 *               (`batch_invert(&r)?` fails, :328)
 *   verdict     0 = the proof is accepted, NMX_IPA_REJECT = P_hat != commit(ck_hat || ck_c, a_hat || a_hat b_hat) (NovaError::InvalidPCS,
 *               :378-388).  The result is NMX_OK whenever the check RAN.
 *   out_ck_hat_xy64, out_ck_hat_is_inf, out_b_hat   (each may be null) the two intermediate values, commit(ck, s, 0) (canonical x || y
 *               like every result) and <b_vec, s> (in the scalars' form): they make a rejection diagnosable.
 * Flags: NMX_SCALARS_MONT (c, b / point, a_hat, rs, out_b_hat are Montgomery limbs), NMX_SCALARS_DEVICE (b only; NMX_E_ARG together
 * with NMX_IPA_B_IS_POINT), NMX_BASES_MONT (ck_c, comm_a, L, R are), NMX_IPA_B_IS_POINT; anything else NMX_E_ARG.  Null arguments and
 * the length rules are NMX_E_ARG before a device or a key is touched; a point of the proof or comm_a that is not canonical or not on
 * the curve: NMX_E_POINT (the reference cannot deserialise it).  On an error nothing is written.  n = 1: no round, s = [1], the
 * equation is still checked.  Synchronous, ordered behind the calling thread's NMX_ASYNC calls; thread-safe like nmx_ipa_prove. */
enum { NMX_IPA_REJECT = 1u << 0 };
int nmx_ipa_verify(uint64_t ck_handle, const void* ck_c_xy64, const void* comm_a_xy64, int comm_a_is_inf, const void* c, const void* b,
                   size_t n, const void* L_xy64, const void* R_xy64, const uint8_t* is_inf, const void* a_hat, const void* rs,
                   uint32_t flags, uint32_t* verdict, uint8_t* out_ck_hat_xy64, uint8_t* out_ck_hat_is_inf, uint8_t* out_b_hat);
/* PolyEvalWitness::batch / batch_diff_size (src/spartan/mod.rs:165-277): out[i] = sum_j s^j * vecs[j][i], i < n_out,
 * vectors shorter than n_out read as zero-padded; every lens[j] <= n_out.  `vecs`, `lens`, `s` are host arrays; the
 * vectors themselves and `out` follow NMX_SCALARS_DEVICE. */
int nmx_field_lincomb_powers(int field, const void* const* vecs, const size_t* lens, size_t k, const void* s, size_t n_out,
                             uint32_t flags, void* out);

/* out[i] = sum_{k >= i} f[k] * u^(k-i), i < n (coefficient form).  out[0] is `poly_eval(f, u)` (Horner,
 * src/provider/hyperkzg.rs:1011-1020); out[1..n) is the quotient h of `div_by_monomial(f, u)`
 * (src/provider/hyperkzg.rs:961-999, h[i-1] = f[i] + h[i]*u) that kzg_open commits to.  `f` and `out` must NOT overlap
 * (NMX_E_ARG for device-resident vectors that do: every out[i] depends on all later coefficients while other waves still
 * read them).  Coefficients may be any 256-bit words; the outputs are canonical (< p). */
int nmx_poly_suffix_horner(int field, const void* f, size_t n, const void* u, uint32_t flags, void* out);
/* The three openings of kzg_open_batch (src/provider/hyperkzg.rs:1007-1072) as ONE pass over the folded polynomials: with
 * B[t] = sum_{i : lens[i] > t} q^i polys[i][t] for t < n_out = max lens[i] (B is :1059; it is summed on the fly and never stored) and
 * m <= 3 points u_j,
 *     outs[j][t] = sum_{s >= t} B[s] u_j^(s - t),  t < n_out
 * so outs[j][0] = B(u_j) (poly_eval, :1011-1020) and outs[j][1..n_out) is the quotient of div_by_monomial(B, u_j) (:961-999).  The
 * outputs are canonical, so they equal nmx_field_lincomb_powers followed by nmx_poly_suffix_horner per point byte for byte; a lane reads
 * only the vectors long enough to reach its index.  u_j = 0, q = 0 and equal points are fine.  Mercury's quot_f is the same pattern with
 * k = 2, m = 1.
 *   polys, lens, q, points, outs   host arrays; k vectors of lens[i] >= 0 elements, coefficients low to high, a word is ANY 256-bit value
 *               read mod p (OPERAND WORDS above); q: 32 bytes; points: m x 32 bytes; outs: m vectors of n_out elements
 *   flags       NMX_SCALARS_DEVICE (the vectors and the outputs are in HBM), NMX_SCALARS_MONT (q, the points and the words are
 *               Montgomery limbs), NMX_ASYNC (HBM operands); anything else NMX_E_ARG
 * k = 0, m = 0, a NULL argument, a field_id that is none of NMX_F_* (not spelled `field`, as for nmx_field_gather), an outs[j] that overlaps an input or another output: NMX_E_ARG;
 * m > 3, k > 4096 or a vector of 2^31 elements or more: NMX_E_TOO_LARGE; q or a point >= p: NMX_E_SCALAR_RANGE.  All found before a
 * device is leased; nothing written.  Options (nmx_set_option; none changes a byte of a result): kzg_quot_chunk (coefficients per lane
 * of the pass over the inputs, 0 = 4, or 8), kzg_quot_scratch (1, the default: the first pass stores B in workspace and the second reads
 * it back; 0: the second sums it again). */
int nmx_poly_lincomb_quotients(int field_id, const void* const* polys, const size_t* lens, size_t k, const void* q, const void* points, size_t m,
                               uint32_t flags, void* const* outs);
/* HyperKZG's evaluation matrix (src/provider/hyperkzg.rs:1011-1020 `poly_eval`, called for every folded polynomial at
 * the three points r, -r, r^2, :1049-1056): out[i * m + j] = polys[i](points[j]) for k polynomials of any lengths
 * (coefficients low to high; an empty polynomial evaluates to 0) at m <= 4 points, all in one launch.  `polys`, `lens`,
 * `points` and `out` are host arrays; the coefficient vectors follow NMX_SCALARS_DEVICE.  A coefficient word is ANY 256-bit value
 * w, read as w mod p; the outputs are canonical (OPERAND WORDS above).  A point >= p: NMX_E_SCALAR_RANGE, before anything is staged or
 * launched, `out` untouched.  m > 4 or k > 4096: NMX_E_TOO_LARGE. */
int nmx_poly_eval_multi(int field, const void* const* polys, const size_t* lens, size_t k, const void* points, size_t m,
                        uint32_t flags, uint8_t* out);
/* ---- Mercury's prover passes (the second evaluation engine on BN254, src/provider/mercury.rs) -----------------------------------
 * The two passes over all N coefficients of f between Mercury's commitments that no other call expresses; f is viewed as an
 * n_rows x n_cols matrix, row-major (the reference calls with n_cols = b = sqrt(N) and n_rows = b, or b / 2 when log N is odd,
 * mercury.rs:919-931).  The third N-sized pass, quot_f (mercury.rs:1163-1180), composes from nmx_field_lincomb_powers over [f, q] with
 * s = -(zeta^b - alpha) and nmx_poly_suffix_horner at zeta: out[1..n) is quot_f and out[0] must equal g(zeta) (the reference's
 * assert_eq!(rem, ZERO)); INTEGRATION.md 2l.  Any n_rows >= 1, n_cols >= 1: no power of two, no n_rows <= n_cols is required.
 * Flags: NMX_SCALARS_MONT (the vectors and alpha are Montgomery limbs), NMX_SCALARS_DEVICE (EVERY vector pointer, the outputs included,
 * is HBM; otherwise host arrays are staged through the context's workspace), NMX_ASYNC (with HBM operands only, as for
 * nmx_poly_fold_pairs); any other flag: NMX_E_ARG.  `alpha` is always a host pointer.  As for nmx_poly_suffix_horner, coefficients
 * (and eq_col) may be any 256-bit words and the outputs are canonical (< p, in the form of the inputs).
 * Errors, all found before a device is touched, and on any error nothing is written: a NULL pointer (other than out_q with
 * n_rows == 1), n_rows == 0 or n_cols == 0, a field_id that is none of NMX_F_*: NMX_E_ARG; n_rows * n_cols overflowing or >= 2^32:
 * NMX_E_TOO_LARGE; alpha >= p: NMX_E_SCALAR_RANGE; overlapping buffers: NMX_E_ARG -- out_q or out_g with f, out_q with out_g, out_h
 * with f or with eq_col (the nmx_poly_suffix_horner rule: every q element depends on rows that other waves still read). */
/* h[row] = sum_{col < n_cols} f[row * n_cols + col] * eq_col[col],  row < n_rows      (compute_h_poly, mercury.rs:369-386, called at :966) */
int nmx_mercury_h_poly(int field_id, const void* f, size_t n_rows, size_t n_cols, const void* eq_col,
                       uint32_t flags, void* out_h /* n_rows */);
/* f(X) = (X^n_cols - alpha) q(X) + g(X), f of n_rows * n_cols coefficients, low to high (divide_by_binomial, mercury.rs:319-356 with
 * divide_by_linear_polynomial :281-288 and transpose :291-312, called at :995):
 *   g[c]              = sum_{j < n_rows}      f[j * n_cols + c] * alpha^j            c < n_cols
 *   q[k * n_cols + c] = sum_{k < j < n_rows}  f[j * n_cols + c] * alpha^(j - k - 1)  k < n_rows - 1
 * q is written in the layout the reference holds AFTER its transpose, as exactly (n_rows - 1) * n_cols elements: the reference's b * b
 * vector before trim() without its all-zero tail.  The reference's trim() may drop further zero top coefficients; those change neither
 * commit(ck, q) nor the later batch_add, so the caller may skip it.  n_rows == 1: q is empty (out_q may be NULL) and g = f.
 * The rows are cut into segments (three launches: local totals, carries, the walk that writes q); option "mercury_seg_rows"
 * of nmx_set_option sets the rows per segment (0 = by size) and never changes a result. */
int nmx_mercury_divide_by_binomial(int field_id, const void* f, size_t n_rows, size_t n_cols, const void* alpha,
                                   uint32_t flags, void* out_q /* (n_rows - 1) * n_cols */, void* out_g /* n_cols */);
/* make_s_polynomial((a1, a2), (b1, b2), log_b, gamma) (mercury.rs:391-475, called at :1072-1077 with (eq_col, eq_row) and (g, h)): the
 * coefficients of X^1 .. X^(b-1) of the Laurent polynomial a1(X) b1(1/X) + a1(1/X) b1(X) + gamma (a2(X) b2(1/X) + a2(1/X) b2(X)):
 *   s[k] = sum_{i=0}^{b-2-k} ( a1[i+k+1] b1[i] + a1[i] b1[i+k+1] ) + gamma sum_{i=0}^{b-2-k} ( a2[i+k+1] b2[i] + a2[i] b2[i+k+1] ),  k < b - 1
 * The reference multiplies by X^(b-1) and goes through four forward FFTs and one inverse FFT of size 2b; nothing wraps mod X^(2b) - 1, so
 * what its drain(..b) keeps is this correlation.  It is exact field arithmetic, independent of any root of unity: valid in all four
 * fields (Grumpkin's scalar field has 2-adicity 1 and no FFT of size 2b) and for ANY b >= 1, no power of two required.  b - 1 canonical
 * elements are written, UNTRIMMED: the reference's trim() drops zero top coefficients, which change neither commit(ck, s) nor an
 * evaluation; where the sum vanishes identically (f = 0) the reference's drain(..b) panics and this call writes zeros.  b == 1: the
 * output is empty, out_s may be NULL and no device is needed.  Flags, words and buffers as for the two passes above: gamma is a host
 * pointer in the vectors' form; every vector pointer follows NMX_SCALARS_DEVICE; NMX_ASYNC with HBM operands; operand words may be any
 * 256-bit value, read mod p.  Errors, found before a device is touched, nothing written: a NULL pointer, a field_id that is none of
 * NMX_F_*, b == 0, another flag, out_s overlapping an input: NMX_E_ARG; gamma >= p: NMX_E_SCALAR_RANGE; b > 2^16: NMX_E_TOO_LARGE (the
 * prover's n stays below 2^31, so its b stays at or below 2^16; the work is 2 b^2 products).  The (k, i) triangle is cut into square
 * tiles, one block each, partial sums exact and added by a finish; option "mercury_s_tile" of nmx_set_option sets the
 * tile (0 = by size, 16, 32, 64) and never changes a byte. */
int nmx_mercury_s_poly(int field_id, const void* a1, const void* b1, const void* a2, const void* b2, size_t b,
                       const void* gamma, uint32_t flags, void* out_s /* b - 1 */);
/* ---- NeutronNova's folding step (neutron::NIFS::prove, src/neutron/nifs.rs:200-289) ----------------------------------------------------
 * The N-sized work of neutron::NIFS::prove that no other call expresses; its commitments are nmx_commit / nmx_msm_u64 and its two
 * multiply_vec products nmx_spmv_apply_many.  Notation: for left, right >= 1, E is a vector of left + right elements,
 * e = E[0, left) and f = E[left, left + right); an N-vector (N = left * right) is indexed k = i * left + j with i < right, j < left;
 * X(t) = X1 + t (X2 - X1).  left and right need not be powers of two.
 * Flags: NMX_SCALARS_MONT (every vector, challenge and output is in Montgomery limbs), NMX_SCALARS_DEVICE (EVERY vector pointer of the
 * call is HBM; otherwise every vector is a host array staged through the context's workspace; mixed placement cannot be expressed),
 * NMX_ASYNC where noted below (with HBM operands only, as for nmx_nifs_fold); any other flag: NMX_E_ARG.  The challenges tau, rho and r_b
 * are always host pointers.  OPERAND WORDS above applies: a 32-byte word of an input vector is ANY 256-bit value w and is read as
 * w mod p, every output word is canonical (< p, in the form of the inputs), and a challenge >= p is NMX_E_SCALAR_RANGE, found before
 * anything is launched: nothing is written.  All argument checks run before a device is touched: a malformed call returns its code on a
 * machine without a GPU and leaves the caller's buffers as they were.  The calls run on logical device 0, are thread-safe and are
 * ordered behind the calling thread's NMX_ASYNC calls. */
/* PowPolynomial::new(tau, ell).split_evals(left, right) (src/spartan/polys/power.rs:62-86): out has left + right elements,
 *   out[j] = tau^j, j < left;      out[left + i] = (tau^left)^i, i < right            (0^0 = 1)
 * right == 1 gives f = [1]; the reference would index out of bounds there (it writes evals[1] of a one-element vector).  One launch:
 * the host computes the squarings tau^(2^b) and (tau^left)^(2^b) and every lane multiplies the ones its index's bits select.
 * left == 0, right == 0 or left + right >= 2^31: NMX_E_ARG.  NMX_ASYNC applies with an HBM `out`. */
int nmx_pow_split_evals(int field_id, const void* tau, size_t left, size_t right, uint32_t flags, void* out /* left + right */);
/* NIFS::prove_helper (src/neutron/nifs.rs:29-186): the five evaluations of the zero-fold's round polynomial at t = 0, 2, 3, 4, 5, in
 * that order, as five elements on the host:
 *   out_t = c_t(rho) * sum_{i < right} f(t)[i] * sum_{j < left} e(t)[j] * (Az(t)[k] * Bz(t)[k] - Cz(t)[k])
 *   c_t(rho) = (1 - rho) + t (2 rho - 1)            -- 1 - rho, 3 rho - 1, 5 rho - 2, 7 rho - 3, 9 rho - 4
 * E1, E2: left + right elements; the six products: left * right elements.  Synchronous.  left == 0 or right == 0: NMX_E_ARG;
 * left * right >= 2^31: NMX_E_TOO_LARGE.  The result is exact mod p and depends neither on the launch geometry nor on the option
 * "neutron_max_blocks" of nmx_set_option (the largest grid of this call and the next: 0 = by size). */
int nmx_neutron_fold_sums(int field_id, size_t left, size_t right, const void* E1, const void* Az1, const void* Bz1, const void* Cz1,
                          const void* E2, const void* Az2, const void* Bz2, const void* Cz2, const void* rho, uint32_t flags,
                          uint8_t* out160);
/* The sum of Structure::is_sat (src/neutron/relation.rs:83-97): out = sum_{i < right} f[i] * sum_{j < left} e[j] * (Az[k] * Bz[k] - Cz[k]),
 * one element on the host; the same kernel as nmx_neutron_fold_sums with one point and one instance.  The comparison with U.T and the two
 * commitments of is_sat stay the caller's (nmx_commit).  Synchronous; limits as for nmx_neutron_fold_sums. */
int nmx_neutron_relation_sum(int field_id, size_t left, size_t right, const void* E, const void* Az, const void* Bz, const void* Cz,
                             uint32_t flags, uint8_t* out32);
/* FoldedWitness::fold (src/neutron/relation.rs:131-156): w = w1 + r_b (w2 - w1) over n_w elements and e = e1 + r_b (e2 - e1) over n_e
 * elements, both in ONE launch (as nmx_nifs_fold).  Either length may be 0; its pointers are then ignored.  Element-wise in-place use
 * (w == w1 or w == w2, e == e1 or e == e2) is allowed; any other overlap of an output with a buffer of the call: NMX_E_ARG.
 * n_w + n_e >= 2^31: NMX_E_TOO_LARGE.  NMX_ASYNC applies with HBM operands.  The scalars r_W, r_E, u, X, T_out and the two point
 * combinations of FoldedInstance::fold are O(1) work and stay on the caller's side. */
int nmx_neutron_fold_witness(int field_id, const void* w1, const void* w2, size_t n_w, const void* e1, const void* e2, size_t n_e,
                             const void* r_b, uint32_t flags, void* w /* n_w */, void* e /* n_e */);
/* EqPolynomial::evals_from_points (src/spartan/polys/eq.rs:54-73): out[2^ell] = eq(r, x) for x in {0,1}^ell, r[0] the
 * most significant variable.  r: ell x 32 bytes, host.  out: host, or HBM with NMX_SCALARS_DEVICE; every entry canonical, in the
 * layout `flags` names (Montgomery: eq * 2^256 mod p).  ell >= 31: NMX_E_ARG.  A coordinate r[i] >= p: NMX_E_SCALAR_RANGE, found
 * before anything is launched; `out` is not written. */
int nmx_eq_evals_from_points(int field, const void* r, size_t ell, uint32_t flags, void* out);
/* MultilinearPolynomial::evaluate / evaluate_with (src/spartan/polys/multilinear.rs:88-129): Z(r), len == 2^ell (NMX_E_ARG otherwise).
 * A word of z is ANY 256-bit value w, read as w mod p, for host and HBM operands alike and at every ell; the result is canonical
 * (OPERAND WORDS above).  z is only read, and never past z[len).  A coordinate r[i] >= p: NMX_E_SCALAR_RANGE, nothing is written. */
int nmx_mle_evaluate(int field, const void* z, size_t len, const void* r, size_t ell, uint32_t flags, uint8_t* out32);
/* MultilinearPolynomial::multi_evaluate_with (src/spartan/polys/multilinear.rs:131-180): k polynomials of the same
 * length 2^ell at one point; the eq tables are built once.  out = k x 32 bytes (host).  Words of the zs, results and errors as
 * for nmx_mle_evaluate: out[j] equals what nmx_mle_evaluate gives for zs[j]. */
int nmx_mle_multi_evaluate(int field, const void* const* zs, size_t k, size_t len, const void* r, size_t ell,
                           uint32_t flags, uint8_t* out);
/* SparseMatrix (CSR, scipy naming: data / indices / indptr, src/r1cs/sparse.rs:232-260) resident in HBM, and
 * SparseMatrix::multiply_vec (sparse.rs:201-229): out[rows] = M * z.  indptr / indices are `usize` on the reference
 * side, hence uint64_t here.  R1CS matrices are fixed per circuit: register once, apply every step.
 * The gathered vector of a product over a registered matrix (z / x of nmx_spmv_apply, _pair, _transposed, _many, and z1 of
 * nmx_r1cs_cross_term when z2 is NULL) may hold ANY 256-bit words: a word w counts as w mod p, the outputs are canonical (< p) and
 * equal the product over the reduced words, in the canonical and in the Montgomery layout alike (there
 * out_word = sum coefficient * (w mod p) mod p).  E and u of nmx_r1cs_cross_term and nmx_r1cs_is_sat are NOT covered by this: they
 * must be < p, the default stated at the top of this header. */
int nmx_spmv_register(int field, const uint64_t* indptr, const uint64_t* indices, const void* data, size_t rows,
                      size_t cols, uint32_t flags, uint64_t* handle);
int nmx_spmv_unregister(uint64_t handle);
int nmx_spmv_apply(uint64_t handle, const void* z, size_t z_len, uint32_t flags, void* out);
/* NIFS::prove's provider work between two commitments as ONE call each (HBM-resident vectors only; NMX_ASYNC applies):
 *  - nmx_r1cs_cross_term: the body of commit_T (src/r1cs/mod.rs:590-620): Z = z1 + z2 (z2 NULL: Z = z1), then for every row
 *    T = (A Z)(B Z) - u (C Z) - E in one pass -- AZ, BZ, CZ never reach HBM.  A, B, C: matrices of one shape and field
 *    (nmx_spmv_register); z1, z2: z_len = cols elements; e, out: rows elements.  Bit-identical to nmx_field_vec_add +
 *    3 x nmx_spmv_apply + nmx_field_cross_term.
 *  - nmx_nifs_fold: R1CSWitness::fold (src/r1cs/mod.rs:1044-1067): w = w1 + r w2 (n_w elements) and e = e1 + r t (n_e
 *    elements) in one launch.  Outputs must not alias inputs other than element-wise in place (w == w1 is fine). */
int nmx_r1cs_cross_term(uint64_t A, uint64_t B, uint64_t C, const void* z1, const void* z2, size_t z_len, const void* e,
                        const void* u, uint32_t flags, void* out);
int nmx_nifs_fold(int field, const void* w1, const void* w2, size_t n_w, const void* e1, const void* t, size_t n_e, const void* r,
                  uint32_t flags, void* w, void* e);
/* R1CSShape::is_sat_relaxed / is_sat (src/r1cs/mod.rs:474-574) as ONE call -- what RecursiveSNARK::verify runs three of under
 * rayon::join (src/nova/mod.rs:637-660), and what `debug_assert!(shape.is_sat_relaxed(..))` needs on the prover's side with the
 * witness already in HBM.  z = [W, u, X]; on every row (A z)(B z) == u (C z) + E (strict form: == C z, u = 1, no E), decided ON THE
 * DEVICE: A z, B z, C z and the residual never reach HBM, a satisfied instance writes nothing at all; and
 * commit(ck, W, r_W) == comm_W, commit(ck, E, r_E) == comm_E, the two commitments begun before the equation pass (the machinery of
 * nmx_commit_begin) so that the pass runs under them.
 *   A, B, C     matrices of one shape and field (nmx_spmv_register); the field must be the scalar field of the key's curve (NMX_E_ARG)
 *   E, u        both NULL: is_sat (n_e, r_E, comm_E_* ignored); both given: is_sat_relaxed; one of the two NULL: NMX_E_ARG
 *   lengths     n_w + 1 + n_io != cols or n_e != rows: NMX_E_ARG, the message says which (the reference's W.len() != num_vars,
 *               X.len() != num_io, E.len() != num_cons, mod.rs:489-494, 540-545); n_w or n_e beyond the key: NMX_E_HANDLE (as nmx_commit);
 *               unknown matrix / key handle: NMX_E_HANDLE.  All of it is checked before anything is launched.
 *   ck_handle   0: the equation only (no commitments; r_*, h, comm_* ignored, the COMM bits stay clear)
 *   flags       NMX_SCALARS_DEVICE: W and E are HBM pointers (otherwise host arrays, uploaded for the call -- a proof that arrives from a
 *               peer is in host memory); NMX_SCALARS_MONT: W, E, u, X, r_W, r_E are Montgomery limbs; NMX_BASES_MONT: h_xy64 AND the two
 *               expected commitments are.  u, X, r_*, h_xy64, comm_* are always host pointers; comm_*_is_inf != 0: the expected
 *               commitment is the identity (its bytes are not read).  Any other flag: NMX_E_ARG.
 *   result      NMX_OK whenever the check RAN; the answer is *verdict: 0 = satisfied, else the OR of NMX_UNSAT_* -- every condition is
 *               evaluated (the reference reports the equation first, mod.rs:516-527: that ordering is the caller's to apply).
 *               *bad_rows / *first_bad_row (may be NULL): number of violated rows and the lowest one, 2^64 - 1 when there is none.
 *               On an error nothing is written.  Synchronous, ordered behind the calling thread's NMX_ASYNC calls like every
 *               synchronous call; keys sharded over several devices work as they do for nmx_commit. */
enum { NMX_UNSAT_EQ = 1u << 0, NMX_UNSAT_COMM_W = 1u << 1, NMX_UNSAT_COMM_E = 1u << 2 };
int nmx_r1cs_is_sat(uint64_t A, uint64_t B, uint64_t C, uint64_t ck_handle, const void* W, size_t n_w, const void* E, size_t n_e,
                    const void* u, const void* X, size_t n_io, const void* r_W, const void* r_E, const void* h_xy64,
                    const void* comm_W_xy64, int comm_W_is_inf, const void* comm_E_xy64, int comm_E_is_inf, uint32_t flags,
                    uint32_t* verdict, uint64_t* bad_rows, uint64_t* first_bad_row);
/* compute_eval_table_sparse's product (src/spartan/mod.rs:497-533: `M_evals[col] += rx[row] * val` over every entry), i.e.
 * out[cols] = M^T * x with x_len == rows -- Spartan's inner sum-check needs it for A, B and C with x = eq(r_x, .)
 * (src/spartan/snark.rs:181-190).  The transposed form (CSC cut into lanes; a column as long as the constant-one column of an
 * R1CS matrix is split so that no lane walks it alone) is built from the resident matrix on the first call and kept with it. */
int nmx_spmv_apply_transposed(uint64_t handle, const void* x, size_t x_len, uint32_t flags, void* out);
/* (M*z1, M*z2) in one pass over the matrix: PrecomputedSparseMatrix::multiply_vec_pair (src/r1cs/sparse.rs:215-229) */
int nmx_spmv_apply_pair(uint64_t handle, const void* z1, const void* z2, size_t z_len, uint32_t flags, void* out1,
                        void* out2);
/* k matrices of one shape family against ONE vector in one call (round 6):
 *   transposed = 0: outs[i] = M_i * x          -- R1CSShape::multiply_vec (src/r1cs/mod.rs:407-471: A z, B z, C z under rayon::join)
 *   transposed = 1: outs[i] = M_i^T * x        -- compute_eval_table_sparse (src/spartan/mod.rs:497-533: the three tables, rayon::join)
 * With NMX_SCALARS_DEVICE the products run side by side (matrix 0 on the call's stream, the others on side streams that start behind
 * it and that it continues behind): they are latency-bound gathers, three in flight take little longer than one; NMX_ASYNC as for the
 * single-matrix calls.  Host operands: one matrix after the other.  1 <= k <= 8, all matrices over the same field. */
int nmx_spmv_apply_many(const uint64_t* handles, size_t k, int transposed, const void* x, size_t x_len, uint32_t flags,
                        void* const* outs);
/* RelaxedR1CSSNARK::verify's multi_evaluate (src/spartan/snark.rs:325-353) as ONE call -- the one piece of CompressedSNARK::verify
 * that grows with the circuit and is not the evaluation argument:
 *   out[i] = sum over every entry (row, col, val) of M_i :  T_x[row] * T_y[col] * val,      i < k
 *   T_x = EqPolynomial::evals_from_points(r_x), T_y = EqPolynomial::evals_from_points(r_y)
 * which the verifier needs for A, B, C to check claim_inner_final == (evals[0] + r evals[1] + r^2 evals[2]) * eval_Z (snark.rs:355).
 * One pass over the resident CSR arrays of all k matrices: T_x is never materialised (two sqrt-size tables, one product per row),
 * T_y is built once in workspace and shared, nothing rows- or cols-sized is written besides it, and the TRANSPOSED form of a
 * matrix is neither built nor required (a verifier that never proves holds the forward arrays only).
 *   handles     k matrices from nmx_spmv_register, 1 <= k <= 8, all over one field (the rule of nmx_spmv_apply_many); any other k,
 *               or matrices over different fields: NMX_E_ARG.  An unknown handle: NMX_E_HANDLE.
 *   r_x, r_y    ell_x / ell_y elements on the HOST, element 0 the most significant variable (as nmx_eq_evals_from_points), canonical,
 *               or Montgomery limbs with NMX_SCALARS_MONT -- then out is Montgomery too.  A coordinate >= the modulus:
 *               NMX_E_SCALAR_RANGE, exactly as nmx_eq_evals_from_points; ell_x, ell_y < 31 as there (NMX_E_ARG).
 *   shapes      rows <= 2^ell_x and cols <= 2^ell_y for EVERY matrix (the reference indexes T_x[row_idx], T_y[col_idx], snark.rs:336,
 *               and would panic; it calls with ell_x = log2(num_cons), ell_y = log2(num_vars) + 1 and cols = num_vars + 1 + num_io
 *               < 2^ell_y).  A violation: NMX_E_ARG, the message names the matrix and the bound.  Matrices of different shapes in
 *               one call are fine as long as each obeys the rule.  More than 2^24 rows: NMX_E_TOO_LARGE.
 *   flags       NMX_SCALARS_MONT or 0; any other flag: NMX_E_ARG.  Null handles / out, null r_x with ell_x > 0 (r_y alike): NMX_E_ARG.
 *   out         k x 32 bytes on the host.  On an error nothing is written.
 * Every argument check runs before a device is touched or a kernel launched.  Synchronous, ordered behind the calling thread's
 * NMX_ASYNC calls like every synchronous call; thread-safe and re-entrant (the reference evaluates the three matrices under
 * into_par_iter, snark.rs:347-350); runs on logical device 0, where matrices live.  The result is exact: it does not depend on
 * the launch geometry. */
int nmx_r1cs_evaluate(const uint64_t* handles, size_t k, const void* r_x, size_t ell_x, const void* r_y, size_t ell_y, uint32_t flags,
                      uint8_t* out /* k x 32 */);

/* ---- measurement ------------------------------------------------------------------------------------
 * With profiling on, every MSM brackets its stages with hipEvents on the stream the kernels run on;
 * nmx_profile_last returns the last call's stage times in milliseconds (same thread).
 * stage order: digits, sort, bounds+plan, accum, fold, reduce, tail(D2H+host Horner) ; returns #stages. */
int nmx_set_profiling(int on);
int nmx_profile_last(float* ms, int cap);
/* The calling thread's last MSM over a multi-device key, shard by shard: returns the number of shards; for shard j < cap
 * ms[j * NMX_PROF_STAGES + s] = its stage times (profiling on; same stage order), dev[j] = its logical device, branch[j] =
 * where its scalars came from (NMX_BRANCH_*); *combine_ms = the combine step alone (all-gather + point sum), *rccl_ranks =
 * ranks of the RCCL communicator it used (0: host sum).  After such a call nmx_profile_last gives the per-stage maximum
 * over the shards. */
#define NMX_PROF_STAGES 12
enum { NMX_BRANCH_HOST = 0,          /* host scalars: the shard's GPU pulled its slice over its own PCIe link            */
       NMX_BRANCH_LOCAL = 1,         /* one HBM array on device 0, this shard is on device 0: used in place              */
       NMX_BRANCH_PEER_COPY = 2,     /* one HBM array on device 0, this shard elsewhere: hipMemcpyPeerAsync over xGMI    */
       NMX_BRANCH_SHARD_RESIDENT = 3,/* NMX_SCALARS_SHARDED: the piece was already in this GPU's HBM                     */
       NMX_BRANCH_NONE = 4 };        /* no scalar array (all-ones sparse form)                                           */
int nmx_profile_last_sharded(float* ms, int* dev, int* branch, int cap, float* combine_ms, int* rccl_ranks);
/* forces the window width (0 = heuristic) -- tuning / tests only */
int nmx_set_window_bits(uint32_t c);
/* Pipeline selection knobs for A/B measurements and tests (the same ones the NMX_TUNE_* environment variables set at
 * start-up); every combination computes the same result.  Names: "no_partition" (1: generic radix-sort path instead of
 * the hand-written LDS partition), "seg_min_total" (segment-balanced accumulate from this many sorted entries on;
 * 0xffffffff: never), "seg_min_len", "seg_lanes" (0: a multiple of the kernel's resident lanes), "no_quad_accum",
 * "no_quad_final", "accum_prefetch" (0: by table size; 1 or 2), "no_batch_fuse" (1: every vector of a batch call runs
 * as its own MSM), "horner_top" (suffix Horner from 1024 coefficients on: 0 = the single-pass scan with decoupled look-back; the two-pass
 * kernels: 8 = 8-coefficient chunks in registers, 4, 1 = chunk-per-lane recursion only), "horner_window" (groups per look-back
 * round of the single-pass scan, 64; 1..63 force its multi-round path in tests), "horner_sub" (512-coefficient sub-tiles per
 * wave of the scan: 0 = by size, 1, 2, 4), "eq_max_blocks" (grid cap of the eq-factored sum passes: 0 = 768 for evaluate_with, 2048 otherwise), "horner_spin_limit" (polls before a wave of the scan gives up and the call falls back
 * to the two-pass kernels: 0 = 2^22; tests set 1),
 * "mercury_s_tile" (outputs x indices per block of nmx_mercury_s_poly's kernel: 0 = by size, or 16, 32, 64; the same bytes at every value),
 * "mercury_seg_rows" (rows per segment of nmx_mercury_divide_by_binomial's kernels: 0 = by size; tests force the multi-segment path
 * at tiny shapes),
 * "neutron_max_blocks" (the largest grid of nmx_neutron_fold_sums / nmx_neutron_relation_sum: 0 = by size, at most 2048; tests force a
 * wave's loop over several tiles at tiny shapes; never changes a result),
 * "fixed_base_c" (window width of the table behind nmx_bases_from_scalars / nmx_bases_setup_from_tau: 4..16, default 8, other values:
 * NMX_E_ARG; the table holds ceil(BITS / c) x (2^c - 1) points of 64 bytes; never changes a result),
 * "derive_lmax" (the longest run of points one lane of nmx_bases_derive_by_address adds before an index is split into tasks: 0 = by
 * rule, else 2..1024, other values: NMX_E_ARG; tests reach the split and fold passes with few points; never changes a result),
 * "host_split" / "host_split_min_n" (an MSM with HOST scalars over at least host_split_min_n = 2^19 pairs of a key on one device is cut
 * into contiguous pieces (host_split = 255, the default: 2 / 3 / 4 pieces from 2^19 / 2^20 / 2^21 pairs; 2..16: that many) -- the
 * reference's own chunk + reduce decomposition, src/provider/msm.rs:564-574 -- so that piece i's scalars cross PCIe while piece
 * i - 1 computes; 0 / 1: one upload, then one MSM),
 * "small_blocks" (MSMs with at most 1024 buckets -- keys below 2^14 points: bucket sums in two block-level launches, this many
 * entries per four-lane group, default 8; 0 = the task path: plan, expand, accumulate, strided folds),
 * "seg_heavy_above" (pieces per bucket summed without a pre-fold pass: 0 = by table width, else 1..63), "no_tree_fuse" (bucket
 * reduction: 0 = fused levels or one launch per level by the box's measured launch gap, 1 = one launch per level, 2 = fused),
 * "reduce_form" (bucket reduction: 0 = by bucket count, 1 = the (D, Y) pair tree, 2 = bit-sliced sums -- the pair-sum tree, the sums of
 * its odd nodes per level and one pairwise combine at the end; other values: NMX_E_ARG),
 * "host_combine" (that combine at the end of the bit-sliced sums: 0 = by rule, 1 = in the reduction's last launch, 2 = on the calling
 * host thread wherever the c points of every bucket set fit the call's 64 KiB landing buffer; other values: NMX_E_ARG),
 * "no_clean_accum" (1: keys without identity points also run the segment accumulate that tests every gathered row for the identity),
 * "accum_prio" (progress-keyed wave priority in the segment accumulate: 0 = by rule, 1 = off, 2 = on -- a wave starts at priority 3 and
 * steps down after a half, three quarters and seven eighths of its segment --, 3 = on with steps after equal quarters; other values:
 * NMX_E_ARG; ignored where the segment accumulate does not run),
 * "part_rows" (first level of the bucket partition: 0 = by rule, 1 = counting and placing passes that reserve runs with global atomics,
 * 2 = per-chunk count rows and a column scan, no global atomics, wherever the shape allows -- window tables of width 15, 16 or 17, keys
 * of up to 16 bits, more than one first-level bin; other values: NMX_E_ARG; same bytes either way),
 * "hist_grid" (blocks of the partition's counting pass; 0 = as the placing pass: measured flat, profiles/r03_msm_2p20/tail_ab.txt),
 * "shard_min_n", "cache_table_after", "max_table_mib" (see the sections above), "force_peer_copy" (1: the HBM-resident scalars of
 * a sharded call are staged through hipMemcpyPeerAsync even when the shard sits on the source GPU: exercises the cross-device
 * branch on a one-GPU box), "combine" (0 and 1: host sum of the partials, the default; 2: RCCL all-gather required -- also with
 * one GPU, an error if it cannot be loaded), "cache_verify" (0: every slice-cache hit
 * re-hashes the caller's whole slice; 1: rolling window, for callers that register immutable keys).
 * Unknown name: NMX_E_ARG. */
int nmx_set_option(const char* name, uint32_t value);

#ifdef __cplusplus
}
#endif
#endif /* NOVA_MI355X_H */
