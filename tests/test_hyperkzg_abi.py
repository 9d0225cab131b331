"""nmx_hyperkzg_prove and nmx_poly_lincomb_quotients without a GPU.
(1) The yardstick (tests/hyperkzg_common.py: EvaluationEngineTrait::prove, src/provider/hyperkzg.rs:926-1116, and ::verify up to the pairing,
:1119-1230, in Python integers) on the reference's own known answers (tests/golden/field_kats.json `hyperkzg_fold_eval`, hyperkzg.rs:1265-1334),
on honest proofs at ell = 1 .. 6 and on proofs with one v entry or one w changed.  ONLY THESE pass without the feature: every test of (2)-(4)
fails on the parent at the missing symbol, header section, emulation source or plan program.
(2) The surface: the two declarations, exported and bound in Python / C++ / Rust, the header section cites the reference lines used, every
argument error returns with no device present and writes nothing, a well-formed call stops only at NMX_E_NO_DEVICE.
(3) The lane bodies of the pass (nova_amd/csrc/hyperkzg.hpp) thread by thread under tests/host_emul/simt.hpp with limb bounds asserted
(-DNMX_DEBUG_BOUNDS), through the library's own launch sequence (lq_run) and thread -> chunk map, against the restatement byte for byte.
(4) The host-side plan (lq_plan, the powers of the points and of q) as a stand-alone g++ -fsanitize=address,undefined program against Python.
What the emulation does NOT run: the launches themselves, staging, the arena, and nmx_hyperkzg_prove's sequence (folds, commitments, the
callback): tests/test_gpu_hyperkzg.py covers those."""
import ctypes
import inspect
import os
import random
import re
import subprocess

import numpy as np
import pytest

from oracle import pyref as R
from tests import fv_common as fc
from tests import hyperkzg_common as hk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nova_amd", "csrc")
LQ_PARAMS = ["int field_id", "const void* const* polys", "const size_t* lens", "size_t k", "const void* q", "const void* points", "size_t m",
             "uint32_t flags", "void* const* outs"]
# the callback type is spelled nmx_transcript_fn_kzg in the prototype (tests/test_integration_shim.py classifies a parameter as a function
# pointer by the prefix nmx_transcript_fn); nmx_kzg_transcript_fn is a typedef of it
PROVE_PARAMS = ["uint64_t ck_handle", "const void* hat_P", "size_t n", "const void* point", "uint32_t flags", "nmx_transcript_fn_kzg transcript",
                "void* ctx", "uint8_t* out_com", "uint8_t* out_com_is_inf", "uint8_t* out_v", "uint8_t* out_w", "uint8_t* out_w_is_inf"]
CB_PARAMS = ["void* ctx", "int stage", "const uint8_t* data", "size_t count", "const uint8_t* is_inf", "uint8_t* out32"]


@pytest.fixture(scope="module")
def L():
    from nova_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- (1) the yardstick -----------------------------------------------------------------------------------------------------------
def test_restated_fold_loop_reproduces_the_references_known_answers():
    for fid, p in fc.FIELDS.items():
        for case in fc.KATS["hyperkzg_fold_eval"]["cases"]:
            polys = hk.folded_polys(p, case["poly"], case["point"])
            last = R.fold_pairs(p, polys[-1], case["point"][0])           # the fold prove leaves to the verifier: x[0]
            assert last == [case["eval"] % p], (fid, case)
            assert R.mle_evaluate(p, case["poly"], case["point"]) == case["eval"] % p


def honest(c, ell, seed, tau=None):
    rng = random.Random(seed)
    p = c.r
    tau = rng.randrange(2, p) if tau is None else tau
    hat_P = [rng.randrange(p) for _ in range(1 << ell)]
    x = [rng.randrange(p) for _ in range(ell)]
    com, v, w = hk.prove(c, tau, hat_P, x, hk.Sha3Transcript(p))
    return tau, hat_P, x, com, v, w


@pytest.mark.parametrize("ell", [1, 2, 3, 4, 5, 6])
def test_restated_verifier_accepts_an_honest_restated_proof_and_rejects_a_changed_one(ell):
    for c in (R.BN254_G1, R.PALLAS) if ell in (1, 3) else (R.BN254_G1,):
        p = c.r
        tau, hat_P, x, com, v, w = honest(c, ell, 100 + ell)
        C, y = hk.commit_tau(c, tau, hat_P), R.mle_evaluate(p, hat_P, x)
        assert len(com) == ell - 1 and len(v) == ell and len(w) == 3
        assert hk.verify(c, tau, C, x, y, com, v, w, hk.Sha3Transcript(p)) == (True, True)
        for i, j in ((0, 0), (ell - 1, 1), (ell - 1, 2), (0, 2)):
            bad = [list(row) for row in v]
            bad[i][j] = (bad[i][j] + 1) % p
            assert hk.verify(c, tau, C, x, y, com, bad, w, hk.Sha3Transcript(p)) != (True, True), (i, j)
        for j in range(3):
            bad_w = list(w)
            bad_w[j] = R.add(c, bad_w[j], (c.gx, c.gy))
            assert hk.verify(c, tau, C, x, y, com, v, bad_w, hk.Sha3Transcript(p))[1] is False, j
        assert hk.verify(c, tau, C, x, (y + 1) % p, com, v, w, hk.Sha3Transcript(p))[0] is False
        assert hk.verify(c, tau, R.add(c, C, (c.gx, c.gy)), x, y, com, v, w, hk.Sha3Transcript(p))[1] is False


def test_restated_quotients_are_the_division_identity():
    p = fc.FIELDS[1]
    rng = random.Random(3)
    polys = [[rng.randrange(p) for _ in range(n)] for n in (9, 4, 0, 13, 1)]
    q, us = rng.randrange(p), [rng.randrange(p), 0, 5]
    outs = hk.lincomb_quotients(p, polys, q, us + [5])
    B = R.lincomb_powers(p, polys, q, 13)
    for u, o in zip(us + [5], outs):
        z = rng.randrange(p)
        assert (R.poly_eval(p, o[1:], z) * (z - u) + o[0]) % p == R.poly_eval(p, B, z) and len(o) == 13
        assert o == [sum(B[s] * pow(u, s - t, p) for s in range(t, 13)) % p for t in range(13)]
    assert outs[1] == B and outs[2] == outs[3]                               # u = 0: out = B itself; equal points, equal outputs


# ---- (2) the surface ----------------------------------------------------------------------------------------------------------------
def _params(text):
    return [re.sub(r"/\*.*?\*/", "", x).strip() for x in re.sub(r"\s+", " ", text).split(",")]


def test_header_declares_library_exports_and_python_binds_the_same_types(L):
    from nova_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nova_mi355x.h")).read()

    def ctype_of(d):
        if d.startswith("nmx_transcript_fn_kzg"):
            return _lib.KZG_TRANSCRIPT_FN
        if "*" in d:
            return ctypes.c_void_p
        return {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}[d.split()[0]]
    for name, want in (("nmx_poly_lincomb_quotients", LQ_PARAMS), ("nmx_hyperkzg_prove", PROVE_PARAMS)):
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert m, "the header does not declare " + name
        assert _params(m.group(1)) == want
        assert hasattr(L, name)
        assert list(getattr(L, name).argtypes) == [ctype_of(d) for d in want]
    m = re.search(r"typedef int \(\*nmx_transcript_fn_kzg\)\(([^;]*)\);", hdr)
    assert m and _params(m.group(1)) == CB_PARAMS
    assert "typedef nmx_transcript_fn_kzg nmx_kzg_transcript_fn;" in hdr
    assert _lib.KZG_TRANSCRIPT_FN._restype_ is ctypes.c_int and len(_lib.KZG_TRANSCRIPT_FN._argtypes_) == len(CB_PARAMS)
    sect = hdr.split("HyperKZG's evaluation argument (the evaluation engine of the primary curve)")[1].split("int nmx_hyperkzg_prove(")[0]
    for needle in ("hyperkzg.rs:926-1116", ":1076-1116", ":1007-1072", ":1002-1004", ":961-999", ":1085-1095", ":1100", ":861-865", ":1106", ":1049-1056",
                   ":869-880", ":1059-1065", ":1062-1065", ":1069", "STAGE 0", "STAGE 1", "STAGE 2", "NMX_E_HANDLE", "NMX_E_SCALAR_RANGE", "NMX_E_ARG",
                   "NMX_BASES_MONT", "NMX_SCALARS_MONT", "NMX_SCALARS_DEVICE", "NMX_ASYNC", "MUST NOT synchronise the device", "Never modified",
                   "r = 0 and q = 0 are legal", "count = 0", "kzg_fused_quotients", "pairing check and tau_H stay the caller's", "sharded"):
        assert needle in sect, needle
    sect = hdr.split("The three openings of kzg_open_batch")[1].split("int nmx_poly_lincomb_quotients(")[0]
    for needle in (":1007-1072", ":1059", ":1011-1020", ":961-999", "byte for byte", "NMX_E_TOO_LARGE", "NMX_E_SCALAR_RANGE", "NMX_E_ARG", "overlaps",
                   "kzg_quot_chunk", "kzg_quot_scratch", "canonical", "nothing written", "u_j = 0"):
        assert needle in sect, needle
    ffi = open(os.path.join(ROOT, "bindings", "rust", "nova-mi355x-sys", "src", "ffi.rs")).read()
    assert "pub fn nmx_hyperkzg_prove(" in ffi and "pub fn nmx_poly_lincomb_quotients(" in ffi and "pub type NmxTranscriptFnKzg" in ffi, \
        "ffi.rs: regenerate with scripts/gen_rust_sys.py"
    assert subprocess.run(["python3", os.path.join(ROOT, "scripts", "gen_rust_sys.py"), "--check"]).returncode == 0, "ffi.rs is stale"


def test_python_and_cpp_wrappers_exist():
    import nova_amd
    from nova_amd import fieldvec as fv
    assert list(inspect.signature(nova_amd.hyperkzg_prove).parameters) == ["ck", "hat_P", "point", "transcript", "ctx", "mont"]
    assert list(inspect.signature(fv.lincomb_quotients).parameters) == ["field", "polys", "q", "points", "mont", "async_"]
    assert "must not synchronise the device" in nova_amd.hyperkzg_prove.__doc__
    hpp = open(os.path.join(ROOT, "include", "nova_mi355x.hpp")).read()
    res = hpp.split("namespace resident {")[1]
    for decl in ("inline void lincomb_quotients(int field", "inline hyperkzg::EvaluationArgument hyperkzg_prove(const CommitmentKey& ck"):
        assert decl in res, decl
    ns = hpp.split("namespace hyperkzg {")[1].split("}  // namespace hyperkzg")[0]
    assert "EvaluationArgument prove(const CommitmentKey& ck, const std::vector<Scalar>& hat_P" in ns
    assert "ck.mont() ? NMX_BASES_MONT : 0u" in ns, "the key's form must reach the call (ADVICE.md, first finding)"
    # ... and the header compiles as C++17 with a transcript type of the documented shape
    prog = ('#include "nova_mi355x.hpp"\nstruct T { nova::provider::Scalar stage(int, const uint8_t*, size_t, const uint8_t*) { return {}; } };\n'
            "int main() { nova::provider::CommitmentKey* ck = nullptr; T t; std::vector<nova::provider::Scalar> p(2), x(1);\n"
            "  if (ck) { nova::hyperkzg::prove(*ck, p, x, t); nova::resident::hyperkzg_prove(*ck, nullptr, 2, x, nullptr, nullptr);\n"
            "            nova::resident::lincomb_quotients(1, {}, {}, {}, {}, {}); }\n  return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"], input=prog, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr


def test_the_options_are_known(L):
    """nmx_set_option applies the environment's defaults first and so needs a device: without one only the refusal can be checked here
    (tests/test_gpu_hyperkzg.py sets the options and requires identical bytes at every value)"""
    from nova_amd import _lib
    ok = 0 if L.nmx_device_count() > 0 else _lib.E_NO_DEVICE
    for name, val, dflt in ((b"kzg_fused_quotients", 0, 2), (b"kzg_quot_chunk", 8, 0), (b"kzg_quot_scratch", 0, 1)):
        assert L.nmx_set_option(name, val) == ok and L.nmx_set_option(name, dflt) == ok
    assert L.nmx_set_option(b"kzg_quot_chunks", 4) != 0
    src = open(os.path.join(CSRC, "capi.hip")).read()
    assert all('n == "%s"' % n in src for n in ("kzg_fused_quotients", "kzg_quot_chunk", "kzg_quot_scratch"))


def test_quotient_argument_errors_need_no_device_and_write_nothing(L):
    from nova_amd import _lib
    fid = 1
    p = fc.FIELDS[fid]
    buf = np.ascontiguousarray(fc.rand_vec(fid, 64, 3).copy())      # f0 = [0, 8), f1 = [8, 12), outs = [16, 24), [24, 32), [32, 40)
    before = buf.copy()
    at = lambda i: buf.ctypes.data + 32 * i  # noqa: E731
    qv, pts = fc.vec([5]).copy(), fc.vec([7, 0, 7]).copy()

    def call(field=fid, polys=(at(0), at(8)), lens=(8, 4), k=None, q=qv.ctypes.data, points=pts.ctypes.data, m=3, flags=0, outs=(at(16), at(24), at(32))):
        k = len(polys) if k is None else k
        pp = (ctypes.c_void_p * max(len(polys), 1))(*polys)
        ll = (ctypes.c_size_t * max(len(lens), 1))(*lens)
        oo = (ctypes.c_void_p * max(len(outs), 1))(*outs)
        return L.nmx_poly_lincomb_quotients(field, pp, ll, k, q, points, m, flags, oo)
    A, TL = _lib.E_ARG, _lib.E_TOO_LARGE
    assert call(k=0) == A and call(m=0) == A and call(q=None) == A and call(points=None) == A
    assert L.nmx_poly_lincomb_quotients(fid, None, None, 2, qv.ctypes.data, pts.ctypes.data, 3, 0, None) == A
    assert call(polys=(None, at(8))) == A and call(outs=(at(16), None, at(32))) == A
    assert call(field=4) == A and call(field=-1) == A
    for fl in (_lib.BASES_MONT, _lib.BASES_DEVICE, _lib.OUT_PARTIAL, 1 << 20):
        assert call(flags=fl) == A, fl
    assert call(m=4, outs=(at(16), at(24), at(32), at(40))) == TL
    assert call(polys=(at(0),) * 4097, lens=(1,) * 4097) == TL and call(lens=(1 << 31, 4)) == TL
    big = fc.vec([p]).copy()
    assert call(q=big.ctypes.data) == _lib.E_SCALAR_RANGE and b"q >=" in L.nmx_last_error()
    bigp = fc.vec([7, (1 << 256) - 1, 7]).copy()
    assert call(points=bigp.ctypes.data) == _lib.E_SCALAR_RANGE and b"point" in L.nmx_last_error()
    # overlaps: an output with an input (by one element at either end), two outputs with each other
    assert call(outs=(at(7), at(24), at(32))) == A and call(outs=(at(16), at(24), at(11))) == A and b"overlap" in L.nmx_last_error()
    assert call(polys=(at(0), at(23)), lens=(8, 4)) == A
    assert call(outs=(at(16), at(23), at(32))) == A and call(outs=(at(16), at(24), at(16))) == A and b"overlap" in L.nmx_last_error()
    assert (buf == before).all(), "a refused call wrote something"
    ok = 0 if L.nmx_device_count() > 0 else _lib.E_NO_DEVICE
    # well-formed calls get past every check: what stops them without a device is NMX_E_NO_DEVICE, nothing else
    assert call() == ok and call(flags=_lib.SCALARS_MONT) == ok and call(m=1) == ok and call(polys=(at(0), None), lens=(8, 0)) == ok
    assert call(polys=(None,), lens=(0,), outs=(None, None, None)) == 0        # nothing to compute: no device needed
    if ok:
        assert (buf == before).all()


def test_prove_argument_errors_need_no_device_and_write_nothing(L):
    from nova_amd import _lib
    fid = 1
    buf = np.ascontiguousarray(fc.rand_vec(fid, 8 + 3 + 64, 5).copy())
    buf[8:11] = fc.vec([1, 2, 3])
    before = buf.copy()
    at = lambda i: buf.ctypes.data + 32 * i  # noqa: E731
    seen = []

    def cb(_ctx, stage, _data, count, _inf, _out):
        seen.append((stage, count))
        return 0
    fn = _lib.KZG_TRANSCRIPT_FN(cb)
    null_fn = ctypes.cast(None, _lib.KZG_TRANSCRIPT_FN)

    def call(h=0xdeadbeef, P=at(0), n=8, point=at(8), flags=0, tr=fn, com=at(16), com_inf=at(20), v=at(24), w=at(40), w_inf=at(48)):
        return L.nmx_hyperkzg_prove(h, P, n, point, flags, tr, None, com, com_inf, v, w, w_inf)
    A = _lib.E_ARG
    assert call(P=None) == A and call(point=None) == A and call(tr=null_fn) == A and call(com=None) == A and call(v=None) == A and call(w=None) == A
    for n in (0, 1, 3, 6, 12, (1 << 20) + 1):
        assert call(n=n) == A, n
    for fl in (_lib.BASES_DEVICE, _lib.OUT_PARTIAL, _lib.SCALARS_SHARDED, _lib.IPA_B_IS_POINT, 1 << 20):
        assert call(flags=fl) == A, fl
    assert call(n=1 << 31) == _lib.E_TOO_LARGE
    assert (buf == before).all() and not seen, "a refused call wrote something or reached the callback"
    # well-formed: every flag that applies, NULL identity outputs, NULL out_com at ell = 1 -- without a device what stops the call is
    # NMX_E_NO_DEVICE and nothing else; with one, the handle is not a registered key
    stop = _lib.E_HANDLE if L.nmx_device_count() > 0 else _lib.E_NO_DEVICE
    assert call() == stop and call(flags=_lib.SCALARS_MONT | _lib.BASES_MONT | _lib.ASYNC) == stop
    assert call(com_inf=None, w_inf=None) == stop and call(n=2, com=None) == stop
    assert (buf == before).all() and not seen


# ---- (3) the kernels' lane bodies under the emulation --------------------------------------------------------------------------------
EMUL_SRC = os.path.join(ROOT, "tests", "host_emul", "hyperkzg_emul.cpp")
EMUL_SO = os.path.join(ROOT, "tests", "host_emul", "libnmx_hyperkzg_emul.so")
RI = 1 << 261          # the internal residue form: x * 2^261 mod p (nova_amd/csrc/fp.hpp)
R256 = 1 << 256        # the Montgomery form of NMX_SCALARS_MONT
W256 = (1 << 256) - 1


@pytest.fixture(scope="module")
def E():
    deps = [EMUL_SRC, os.path.join(ROOT, "tests", "host_emul", "simt.hpp")] + [os.path.join(CSRC, f) for f in ("fp.hpp", "hyperkzg.hpp", "host_fp4.hpp",
                                                                                                            "spmv_row.hpp", "msm_partition.hpp")]
    if not os.path.exists(EMUL_SO) or os.path.getmtime(EMUL_SO) < max(os.path.getmtime(x) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", EMUL_SO, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_SO)
    vp, u32, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    lib.emul_lincomb_quotients.argtypes = [i, u32, i, vp, vp, u32, vp, vp, u32, u32, vp]
    return lib


def emul(E, fid, polys, q, points, chunk=0, scratch=0):
    """the pass under the emulation -> m lists of integers; the powers of q and of the points are handed over in the internal form"""
    p = fc.FIELDS[fid]
    k, m = len(polys), len(points)
    n_out = max(len(f) for f in polys)
    K, ns = hk.lq_plan(n_out, chunk)
    arrs = [fc.vec(f).copy() if len(f) else np.zeros((1, 32), np.uint8) for f in polys]
    ptrs = (ctypes.c_void_p * k)(*[a.ctypes.data for a in arrs])
    lens = np.array([len(f) for f in polys], np.uint32)
    w = fc.vec([pow(q, i, p) * RI % p for i in range(k)]).copy()
    up = fc.vec([pow(u, e, p) * RI % p for u in points for e in hk.lq_point_power_exponents(K, len(ns))]).copy()
    outs = [np.full((n_out + 1, 32), 0xEE, np.uint8) for _ in range(m)]      # (one element of slack: nothing may land there)
    optr = (ctypes.c_void_p * m)(*[o.ctypes.data for o in outs])
    rc = E.emul_lincomb_quotients(fid, chunk, scratch, ptrs, lens.ctypes.data, k, w.ctypes.data, up.ctypes.data, m, len(ns), optr)
    assert rc == 0, {-2: "the plan's level count differs from the restatement", -3: "a store past the end of a workspace vector"}.get(rc, rc)
    for o in outs:
        assert (o[n_out] == 0xEE).all(), "a store past the end of an output"
    return [fc.ints(o[:n_out]) for o in outs]


def check(E, fid, polys, q, points, **kw):
    p = fc.FIELDS[fid]
    got = emul(E, fid, polys, q, points, **kw)
    assert got == hk.lincomb_quotients(p, polys, q, points), (fid, [len(f) for f in polys], kw)


def rand_polys(p, lens, seed):
    rng = random.Random(seed)
    return [[rng.choice([0, 1, p - 1]) if rng.random() < 0.1 else rng.randrange(p) for _ in range(n)] for n in lens]


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
def test_emulated_pass_at_its_chunk_and_level_sizes(E, fid):
    """one lane's chunk (4, or 8 by option), one chunk of the level above (16 chunks), two levels above -- and one either side of each"""
    p = fc.FIELDS[fid]
    rng = random.Random(fid)
    for chunk, sizes in ((8, (1, 7, 8, 9, 127, 128, 129, 2047, 2048, 2049)), (0, (3, 4, 5, 63, 64, 65, 1023, 1024, 1025))):
        for n in sizes:
            m = 1 + n % 3
            polys = rand_polys(p, (n, max(n // 2, 1), n - 1), 10 * n + fid)
            check(E, fid, polys, rng.randrange(p), [rng.randrange(p) for _ in range(m)], chunk=chunk, scratch=n % 2)


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
def test_emulated_pass_on_proves_halving_lengths(E, fid):
    p = fc.FIELDS[fid]
    rng = random.Random(50 + fid)
    for ell in range(1, 13):
        if ell > 8 and ell % 4 != fid:       # the long shapes: each on one field (every field runs 1 .. 8 and one of 9 .. 12)
            continue
        r = rng.randrange(p)
        polys = rand_polys(p, [1 << (ell - i) for i in range(ell)], 7 * ell + fid)
        check(E, fid, polys, rng.randrange(p), [r, (-r) % p, r * r % p], scratch=ell % 2)


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
@pytest.mark.parametrize("k", [1, 2, 5, 20, 40])
def test_emulated_pass_on_ragged_shapes_and_every_point_count(E, fid, k):
    """ragged lengths, a first vector that is not the longest, empty vectors; k = 40: the descriptors come from memory, not the arguments"""
    p = fc.FIELDS[fid]
    rng = random.Random(k + 100 * fid)
    base = [1000, 37, 999, 1, 0]
    lens = {1: [300], 2: [37, 1000]}.get(k) or (base + [rng.randrange(0, 1100) for _ in range(k - 5)])
    polys = rand_polys(p, lens, k + fid)
    for m in (1, 2, 3):
        check(E, fid, polys, rng.randrange(p), [rng.randrange(p) for _ in range(m)], chunk=8 if (m + k) % 2 else 0, scratch=m % 2)


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
def test_emulated_pass_at_value_edges(E, fid):
    p = fc.FIELDS[fid]
    rng = random.Random(9 + fid)
    lens = (150, 75, 150, 9, 20, 33, 150)                                  # seven vectors reach the low chunks: more than one normalisation
    r = rng.randrange(p)
    top = [[p - 1] * n for n in lens]
    check(E, fid, top, p - 1, [p - 1] * 3, chunk=8)                               # every coefficient p - 1 with q = u_j = p - 1
    check(E, fid, [[0] * n for n in lens], r, [r, 0, 1])                    # all zero
    check(E, fid, [[W256] * n for n in lens], p - 1, [p - 1, r, 0])         # words 2^256 - 1: read mod p
    check(E, fid, [[W256] * n for n in lens[:1]], 1, [1], scratch=1)
    mixed = rand_polys(p, lens, 77 + fid)
    mixed[2][5], mixed[0][149], mixed[6][0] = W256, p, p + 1
    check(E, fid, mixed, r, [0, 0, 0])                                      # u_j = 0 (r = 0 gives u = [0, 0, 0]): the quotient is B[1..]
    check(E, fid, mixed, 0, [r, (-r) % p, r * r % p])                       # q = 0: B = f_0
    check(E, fid, mixed, r, [r, r, r], chunk=8, scratch=1)                             # equal points
    # Montgomery words (NMX_SCALARS_MONT): the stored words are x 2^256 mod p, the outputs come back in the same form
    vals = rand_polys(p, lens, 78 + fid)
    q, us = rng.randrange(p), [rng.randrange(p) for _ in range(3)]
    got = emul(E, fid, [[x * R256 % p for x in f] for f in vals], q, us)
    assert got == [[x * R256 % p for x in o] for o in hk.lincomb_quotients(p, vals, q, us)]


# ---- (4) the host-side plan, a stand-alone program built with the sanitizers ----------------------------------------------------------
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "hyperkzg_plan_test.cpp")
PLAN_BIN = os.path.join(ROOT, "tests", "cpp", "hyperkzg_plan_test.bin")


@pytest.fixture(scope="module")
def plan():
    """built with the sanitizers: a stand-alone program with its own main, host code only"""
    deps = [PLAN_SRC] + [os.path.join(CSRC, f) for f in ("fp.hpp", "hyperkzg.hpp", "host_fp4.hpp")]
    if not os.path.exists(PLAN_BIN) or os.path.getmtime(PLAN_BIN) < max(os.path.getmtime(x) for x in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", PLAN_BIN, PLAN_SRC])
    return lambda *a: subprocess.run([PLAN_BIN] + [str(x) for x in a], capture_output=True, text=True, check=True).stdout.split()


def test_plan_program_agrees_with_python(plan):
    assert plan("self")[-1] == "ok"
    for opt in (0, 4, 8):
        for n in (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1000, 2048, 2049, 1 << 14, 1 << 20, (1 << 20) + 1, (1 << 31) - 1):
            K, ns = hk.lq_plan(n, opt)
            assert [int(x) for x in plan("plan", n, opt)] == [K, len(ns)] + ns, (n, opt)
            assert ns[-1] <= (K if len(ns) == 1 else 16) and len(ns) <= 12
    rng = random.Random(4)
    for fid, p in fc.FIELDS.items():
        for u in (0, 1, p - 1, rng.randrange(p)):
            for n, opt in ((1, 0), (9, 0), (129, 0), (1 << 20, 0), (1 << 20, 4), (70, 4)):
                K, ns = hk.lq_plan(n, opt)
                want = [pow(u, e, p) for e in hk.lq_point_power_exponents(K, len(ns))]
                assert [int(x, 16) for x in plan("upow", fid, "%064x" % u, n, opt)] == want, (fid, u, n, opt)
            assert [int(x, 16) for x in plan("qpow", fid, "%064x" % u, 21)] == [pow(u, i, p) for i in range(21)]
