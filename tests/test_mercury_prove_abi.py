"""nmx_mercury_prove and nmx_mercury_s_poly without a GPU.
(1) The yardstick (tests/mercury_prove_common.py: EvaluationEngineTrait::prove, src/provider/mercury.rs:891-1268, make_s_polynomial in the
reference's FFT form, :391-475, generate_batch_evaluate_arg, :567-770, and ::verify up to the pairing, :1270-1486, in Python integers): the
restated verifier accepts the restated proof at ell = 2 .. 8 and rejects it after any one of its fourteen elements is changed; the FFT form
equals the correlation the kernel computes on the three fields that have the roots of unity.  ONLY THESE pass without the feature: every
test of (2)-(4) fails on the parent at the missing symbol, header section, emulation source or host program.
(2) The surface: the two declarations, exported and bound in Python / C++ / Rust, the header sections cite the reference lines used, every
argument error returns with no device present and writes nothing, a well-formed call stops only at NMX_E_NO_DEVICE.
(3) The kernels of nmx_mercury_s_poly (nova_amd/csrc/mercury_s.hpp) whole under tests/host_emul/simt.hpp -- the conversion, the tiled kernel
with its LDS staging and barriers on the plan's own grid, the finish -- with limb bounds asserted (-DNMX_DEBUG_BOUNDS), against the
definition byte for byte.
(4) The host algebra of the batch opening (nova_amd/csrc/mercury_host.hpp) as a stand-alone g++ -fsanitize=address,undefined program
against the restatement.
What the emulation does NOT run: the launches themselves, staging of host operands, the arena, and nmx_mercury_prove's sequence (the
passes, the commitments, the callback): tests/test_gpu_mercury_prove.py covers those."""
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
from tests import mercury_common as MC
from tests import mercury_prove_common as MP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nova_amd", "csrc")
S_PARAMS = ["int field_id", "const void* a1", "const void* b1", "const void* a2", "const void* b2", "size_t b", "const void* gamma", "uint32_t flags",
            "void* out_s"]
PROVE_PARAMS = ["uint64_t ck_handle", "const void* poly", "size_t n", "const void* point", "uint32_t flags", "nmx_transcript_fn_kzg transcript",
                "void* ctx", "uint8_t* out_comms", "uint8_t* out_is_inf", "uint8_t* out_evals"]
W256 = (1 << 256) - 1
RI = 1 << 261          # the internal residue form: x * 2^261 mod p (nova_amd/csrc/fp.hpp)
R256 = 1 << 256        # the Montgomery form of NMX_SCALARS_MONT


@pytest.fixture(scope="module")
def L():
    from nova_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- (1) the yardstick: passes without the feature ---------------------------------------------------------------------------------
def honest(c, ell, seed):
    rng = random.Random(seed)
    p = c.r
    tau = rng.randrange(2, p)
    poly = [rng.randrange(p) for _ in range(1 << ell)]
    x = [rng.randrange(p) for _ in range(ell)]
    comms, evals, trace = MP.prove(c, tau, poly, x, MP.Sha3Transcript(p))
    return tau, poly, x, comms, evals, trace


@pytest.mark.parametrize("ell", [2, 3, 4, 5, 6, 7, 8])
def test_restated_verifier_accepts_an_honest_restated_proof_and_rejects_a_changed_one(ell):
    """passes without the feature: it checks the yardstick itself"""
    for c in (R.BN254_G1, R.PALLAS, R.GRUMPKIN) if ell in (2, 3) else (R.BN254_G1,):
        p = c.r
        tau, poly, x, comms, evals, trace = honest(c, ell, 100 + ell)
        C, y = MP.commit_tau(c, tau, poly), R.mle_evaluate(p, poly, x)
        b = 1 << ((ell + 1) // 2)
        assert len(trace["W"]) == len(trace["W_prime"]) == len(trace["s"]) == b - 1 and len(trace["h"]) == len(trace["g"]) == b
        MC.check_h_against_eval(p, trace["eq_row"], trace["h"], y)                        # the reference's debug identities (:972-984, :1053-1065)
        MC.check_g_against_h_alpha(p, trace["eq_col"], trace["g"], trace["h"], trace["alpha"])
        assert MP.verify(c, tau, C, x, y, comms, evals, MP.Sha3Transcript(p), prover_trace=trace) == (True, True, True)
        for i in range(8):                                                                # each of the eight commitments moved by G
            bad = list(comms)
            bad[i] = R.add(c, bad[i], (c.gx, c.gy))
            assert MP.verify(c, tau, C, x, y, bad, evals, MP.Sha3Transcript(p)) != (True, True, True), MP.COMM_NAMES[i]
        for i in range(6):                                                                # each of the six evaluations plus one
            bad = list(evals)
            bad[i] = (bad[i] + 1) % p
            assert MP.verify(c, tau, C, x, y, comms, bad, MP.Sha3Transcript(p)) != (True, True, True), MP.EVAL_NAMES[i]
        assert MP.verify(c, tau, C, x, (y + 1) % p, comms, evals, MP.Sha3Transcript(p)) != (True, True, True)
        assert MP.verify(c, tau, R.add(c, C, (c.gx, c.gy)), x, y, comms, evals, MP.Sha3Transcript(p)) != (True, True, True)


def test_fft_form_equals_the_correlation_on_the_fields_that_have_the_roots():
    """passes without the feature: make_s_polynomial line by line (four forward FFTs, one inverse, :391-475) against the definition of
    nmx_mercury_s_poly; BN254 Fq has 2-adicity 1 and no root of order 2b"""
    assert MP.root_of_unity(fc.FIELDS[0], 4) is None and (fc.FIELDS[0] - 1) % 4 == 2
    for fid in (1, 2, 3):
        p = fc.FIELDS[fid]
        rng = random.Random(fid)
        for log_b in (1, 2, 3, 4, 5):
            b = 1 << log_b
            a1, a2, b1, b2 = ([rng.randrange(p) for _ in range(b)] for _ in range(4))
            for gamma in (0, 1, p - 1, rng.randrange(p)):
                want = MP.s_definition(p, a1, b1, a2, b2, gamma)
                assert MP.make_s_polynomial_fft(p, (a1, a2), (b1, b2), log_b, gamma) == MC.trimmed(p, want), (fid, log_b, gamma)
            half = [0] * (b // 2)                                                          # the odd-ell shape: zero upper halves
            a2h, b2h = a2[:b - b // 2] + half, b2[:b - b // 2] + half
            want = MP.s_definition(p, a1, b1, a2h, b2h, gamma)
            assert MP.make_s_polynomial_fft(p, (a1, a2h), (b1, b2h), log_b, gamma) == MC.trimmed(p, want)
        with pytest.raises(AssertionError):                                               # the corner where the reference's drain(..b) panics
            MP.make_s_polynomial_fft(p, ([0] * 4, [0] * 4), ([0] * 4, [0] * 4), 2, 5)
        assert MP.s_definition(p, [0] * 4, [0] * 4, [0] * 4, [0] * 4, 5) == [0, 0, 0]


def test_closed_interpolants_equal_the_linear_solve_and_coinciding_points_have_no_solution():
    """passes without the feature"""
    p = fc.FIELDS[1]
    rng = random.Random(6)
    xs, ys = [rng.randrange(p) for _ in range(3)], [rng.randrange(p) for _ in range(3)]
    for n in (1, 2, 3):
        f = MP.from_evals_with_xs(p, xs[:n], ys[:n])
        assert len(f) == n and [MC.UniPoly(f, p).evaluate(x) for x in xs[:n]] == ys[:n]
    with pytest.raises(ValueError):
        MP.from_evals_with_xs(p, [xs[0], xs[1], xs[0]], ys)


# ---- (2) the surface ----------------------------------------------------------------------------------------------------------------
def _params(text):
    return [x.strip() for x in re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text)).split(",")]


def test_header_declares_library_exports_and_python_binds_the_same_types(L):
    from nova_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nova_mi355x.h")).read()

    def ctype_of(d):
        if d.startswith("nmx_transcript_fn_kzg"):
            return _lib.KZG_TRANSCRIPT_FN
        if "*" in d:
            return ctypes.c_void_p
        return {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}[d.split()[0]]
    for name, want in (("nmx_mercury_s_poly", S_PARAMS), ("nmx_mercury_prove", PROVE_PARAMS)):
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert m, "the header does not declare " + name
        assert _params(m.group(1)) == want
        assert hasattr(L, name)
        assert list(getattr(L, name).argtypes) == [ctype_of(d) for d in want]
    sect = hdr.split("Mercury's evaluation argument (the second evaluation engine of the primary curve)")[1].split("int nmx_mercury_prove(")[0]
    for needle in ("mercury.rs:891-1268", ":567-770", ":914", ":911-931", ":919-923", ":905-907", ":937-938", ":966", ":987", ":995", ":1046-1049", ":1068",
                   ":1072-1077", ":1113-1120", ":1123-1126", ":1132", ":1134", ":1136-1159", ":1203-1208", ":1163-1180", ":1177", ":1212-1217", ":586",
                   ":592-614", ":619-665", ":668-674", ":677", ":678-682", ":687-751", ":754-761", ":764", ":1249", ":1250",
                   "STAGE 0", "STAGE 1", "STAGE 2", "STAGE 3", "STAGE 4", "STAGE 5", "STAGE 6", "NMX_E_HANDLE", "NMX_E_SCALAR_RANGE", "NMX_E_ARG",
                   "NMX_E_ZERO", "NMX_E_TOO_LARGE", "NMX_BASES_MONT", "NMX_SCALARS_MONT", "NMX_SCALARS_DEVICE", "NMX_ASYNC",
                   "MUST NOT synchronise the device", "Never modified", "alpha = 0, gamma = 0, beta = 0 and any z", "kzg_fused_quotients",
                   "verify, G2 and tau_H stay the caller's", "sharded", "comm_h, comm_g, comm_q, comm_s, comm_d,", "g_zeta, g_zeta_inv, h_zeta, h_zeta_inv, s_zeta, s_zeta_inv"):
        assert needle in sect, needle
    sect = hdr.split("make_s_polynomial((a1, a2), (b1, b2), log_b, gamma)")[1].split("int nmx_mercury_s_poly(")[0]
    for needle in ("mercury.rs:391-475", ":1072-1077", "2-adicity 1", "UNTRIMMED", "drain(..b) panics", "NMX_E_TOO_LARGE", "NMX_E_SCALAR_RANGE", "NMX_E_ARG",
                   "overlapping", "mercury_s_tile", "never changes a byte", "b == 1", "no power of two", "nothing written"):
        assert needle in sect, needle
    ffi = open(os.path.join(ROOT, "bindings", "rust", "nova-mi355x-sys", "src", "ffi.rs")).read()
    assert "pub fn nmx_mercury_prove(" in ffi and "pub fn nmx_mercury_s_poly(" in ffi and "stage 6: 1 point  (comm_w_prime)" in ffi, \
        "ffi.rs: regenerate with scripts/gen_rust_sys.py"
    assert subprocess.run(["python3", os.path.join(ROOT, "scripts", "gen_rust_sys.py"), "--check"]).returncode == 0, "ffi.rs is stale"


def test_python_and_cpp_wrappers_exist():
    import nova_amd
    from nova_amd import fieldvec as fv
    assert list(inspect.signature(nova_amd.mercury_prove).parameters) == ["ck", "poly", "point", "transcript", "ctx", "mont"]
    assert list(inspect.signature(fv.mercury_s_poly).parameters) == ["field", "a1", "b1", "a2", "b2", "gamma", "mont", "async_"]
    assert "must not synchronise the device" in nova_amd.mercury_prove.__doc__
    hpp = open(os.path.join(ROOT, "include", "nova_mi355x.hpp")).read()
    res = hpp.split("namespace resident {")[1]
    for decl in ("inline void mercury_s_poly(int field", "inline mercury::EvaluationArgument mercury_prove(const CommitmentKey& ck"):
        assert decl in res, decl
    ns = hpp.split("namespace mercury {")[1].split("}  // namespace mercury")[0]
    assert "EvaluationArgument prove(const CommitmentKey& ck, const std::vector<Scalar>& poly" in ns
    assert "ck.mont() ? NMX_BASES_MONT : 0u" in ns, "the key's form must reach the call"
    # ... and the header compiles as C++17 with a transcript type of the documented shape
    prog = ('#include "nova_mi355x.hpp"\nstruct T { nova::provider::Scalar stage(int, const uint8_t*, size_t, const uint8_t*) { return {}; } };\n'
            "int main() { nova::provider::CommitmentKey* ck = nullptr; T t; std::vector<nova::provider::Scalar> p(4), x(2);\n"
            "  if (ck) { auto a = nova::mercury::prove(*ck, p, x, t); auto b = nova::resident::mercury_prove(*ck, nullptr, 4, x, nullptr, nullptr);\n"
            "            (void)a.comm_quot_f; (void)b.s_zeta_inv; nova::resident::mercury_s_poly(1, nullptr, nullptr, nullptr, nullptr, 4, {}, nullptr); }\n"
            "  return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"], input=prog, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr


def test_the_option_is_known(L):
    """nmx_set_option applies the environment's defaults first and so needs a device: without one only the refusal can be checked here
    (tests/test_gpu_mercury_prove.py sets the option and requires identical bytes at every value)"""
    from nova_amd import _lib
    ok = 0 if L.nmx_device_count() > 0 else _lib.E_NO_DEVICE
    assert L.nmx_set_option(b"mercury_s_tile", 32) == ok and L.nmx_set_option(b"mercury_s_tile", 0) == ok
    assert L.nmx_set_option(b"mercury_s_tiles", 32) != 0
    assert 'n == "mercury_s_tile"' in open(os.path.join(CSRC, "capi.hip")).read()


def test_s_poly_argument_errors_need_no_device_and_write_nothing(L):
    from nova_amd import _lib
    fid = 1
    p = fc.FIELDS[fid]
    buf = np.ascontiguousarray(fc.rand_vec(fid, 64, 3).copy())          # a1 = [0, 8), b1 = [8, 16), a2 = [16, 24), b2 = [24, 32), out = [32, 39)
    before = buf.copy()
    at = lambda i: buf.ctypes.data + 32 * i  # noqa: E731
    g5 = fc.vec([5]).copy()

    def call(field=fid, a1=at(0), b1=at(8), a2=at(16), b2=at(24), b=8, gamma=g5.ctypes.data, flags=0, out=at(32)):
        return L.nmx_mercury_s_poly(field, a1, b1, a2, b2, b, gamma, flags, out)
    A = _lib.E_ARG
    assert call(a1=None) == A and call(b1=None) == A and call(a2=None) == A and call(b2=None) == A and call(gamma=None) == A and call(out=None) == A
    assert call(field=4) == A and call(field=-1) == A and call(b=0) == A
    for fl in (_lib.BASES_MONT, _lib.BASES_DEVICE, _lib.OUT_PARTIAL, 1 << 20):
        assert call(flags=fl) == A, fl
    assert call(b=(1 << 16) + 1) == _lib.E_TOO_LARGE
    assert call(gamma=fc.vec([p]).copy().ctypes.data) == _lib.E_SCALAR_RANGE and b"gamma" in L.nmx_last_error()
    for out in (at(0), at(7), at(12), at(23), at(31)):                  # out_s with each input, by one element at either end
        assert call(out=out) == A and b"overlap" in L.nmx_last_error(), out
    assert call(a1=at(33)) == A and call(b2=at(38)) == A
    assert (buf == before).all(), "a refused call wrote something"
    ok = 0 if L.nmx_device_count() > 0 else _lib.E_NO_DEVICE
    # well-formed calls get past every check: what stops them without a device is NMX_E_NO_DEVICE, nothing else
    assert call() == ok and call(flags=_lib.SCALARS_MONT) == ok and call(b=3) == ok and call(out=at(39), a1=at(8)) == ok
    assert call(b=1, out=None) == 0                                     # an empty output: no device needed
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

    def call(h=0xdeadbeef, P=at(0), n=8, point=at(8), flags=0, tr=fn, comms=at(16), infs=at(40), evals=at(48)):
        return L.nmx_mercury_prove(h, P, n, point, flags, tr, None, comms, infs, evals)
    A = _lib.E_ARG
    assert call(P=None) == A and call(point=None) == A and call(tr=null_fn) == A and call(comms=None) == A and call(evals=None) == A
    for n in (0, 1, 2, 3, 6, 12, (1 << 20) + 1):                         # ell < 2 (assert!(log_n > 1)) or no power of two
        assert call(n=n) == A, n
    for fl in (_lib.BASES_DEVICE, _lib.OUT_PARTIAL, _lib.SCALARS_SHARDED, _lib.IPA_B_IS_POINT, 1 << 20):
        assert call(flags=fl) == A, fl
    assert call(n=1 << 31) == _lib.E_TOO_LARGE
    assert (buf == before).all() and not seen, "a refused call wrote something or reached the callback"
    # well-formed: every flag that applies, a NULL out_is_inf, the smallest n -- without a device what stops the call is NMX_E_NO_DEVICE and
    # nothing else; with one, the handle is not a registered key
    stop = _lib.E_HANDLE if L.nmx_device_count() > 0 else _lib.E_NO_DEVICE
    assert call() == stop and call(flags=_lib.SCALARS_MONT | _lib.BASES_MONT | _lib.ASYNC) == stop
    assert call(infs=None) == stop and call(n=4) == stop
    assert (buf == before).all() and not seen


# ---- (3) the kernels under the emulation ---------------------------------------------------------------------------------------------
EMUL_SRC = os.path.join(ROOT, "tests", "host_emul", "mercury_s_emul.cpp")
EMUL_SO = os.path.join(ROOT, "tests", "host_emul", "libnmx_mercury_s_emul.so")


@pytest.fixture(scope="module")
def E():
    deps = [EMUL_SRC, os.path.join(ROOT, "tests", "host_emul", "simt.hpp")] + [os.path.join(CSRC, f) for f in ("fp.hpp", "mercury_s.hpp", "spmv_row.hpp",
                                                                                                            "msm_partition.hpp")]
    if not os.path.exists(EMUL_SO) or os.path.getmtime(EMUL_SO) < max(os.path.getmtime(x) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", EMUL_SO, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_SO)
    vp, u32, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    lib.emul_mercury_s.argtypes = [i, vp, vp, vp, vp, u32, vp, u32, u32, vp, vp]
    return lib


def s_plan(b, opt):
    """mercury_s_plan restated: (tile, ktiles, chunks, cpt)"""
    tile = opt or (64 if b >= 8192 else 32 if b >= 512 else 16)
    tiles = (b - 1 + tile - 1) // tile
    want = min(min(32, (1024 + tiles - 1) // tiles), tiles)
    cpt = (tiles + want - 1) // want
    return tile, tiles, (tiles + cpt - 1) // cpt, cpt


def emul(E, fid, ops, gamma, tile=0, mont=False):
    """the three launches under the emulation -> b - 1 integers; gamma is handed over in the internal form"""
    p = fc.FIELDS[fid]
    b = len(ops[0])
    arrs = [fc.vec(v).copy() for v in ops]
    gi = fc.vec([gamma * RI % p]).copy()
    out = np.full((b, 32), 0xEE, np.uint8)                                 # (one element of slack: nothing may land there)
    plan = np.zeros(4, np.uint32)
    rc = E.emul_mercury_s(fid, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, arrs[3].ctypes.data, b, gi.ctypes.data, int(mont), tile,
                          out.ctypes.data, plan.ctypes.data)
    assert rc == 0, {-1: "bad arguments", -3: "a store past the end of the partials"}.get(rc, rc)
    assert (out[b - 1] == 0xEE).all(), "a store past the end of the output"
    assert tuple(int(x) for x in plan) == s_plan(b, tile), "the plan differs from its restatement"
    return fc.ints(out[:b - 1])


def biased(p, n, rng, wide=True):
    """the 0 / 1 / p - 1 / p - 2 bias of tests/test_mercury_abi.py, and words at or above p"""
    edge = [0, 1, p - 1, p - 2] + ([p, p + 1, W256] if wide else [])
    return [rng.choice(edge) if rng.random() < 0.2 else rng.randrange(p) for _ in range(n)]


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
@pytest.mark.parametrize("b", [1, 2, 3, 4, 5, 8, 17, 64, 65, 130])
def test_emulated_s_kernel_equals_the_definition(E, fid, b):
    p = fc.FIELDS[fid]
    rng = random.Random(1000 * fid + b)
    if b == 1:
        assert E.emul_mercury_s(fid, None, None, None, None, 1, None, 0, 0, None, None) == -1, "b = 1 never reaches a kernel: the entry point returns first"
        assert MP.s_definition(p, [5], [6], [7], [8], 9) == []
        return
    for gamma in (0, 1, p - 1, rng.randrange(p)):
        ops = [biased(p, b, rng) for _ in range(4)]
        want = MP.s_definition(p, ops[0], ops[1], ops[2], ops[3], gamma)
        for tile in (16, 64):                                              # two values of the option: the same bytes
            assert emul(E, fid, ops, gamma, tile) == want, (fid, b, gamma, tile)
    assert emul(E, fid, [[p - 1] * b] * 4, p - 1, 0) == MP.s_definition(p, [p - 1] * b, [p - 1] * b, [p - 1] * b, [p - 1] * b, p - 1)
    assert emul(E, fid, [[W256] * b] * 4, p - 1, 32) == MP.s_definition(p, [W256] * b, [W256] * b, [W256] * b, [W256] * b, p - 1)
    assert emul(E, fid, [[0] * b] * 4, 7, 0) == [0] * (b - 1)
    # Montgomery words (NMX_SCALARS_MONT): the stored words are x 2^256 mod p, the output comes back in the same form
    vals = [biased(p, b, rng, wide=False) for _ in range(4)]
    m = lambda x: x * R256 % p  # noqa: E731
    assert emul(E, fid, [[m(x) for x in v] for v in vals], gamma, 16, mont=True) == [m(x) for x in MP.s_definition(p, vals[0], vals[1], vals[2], vals[3], gamma)]


def test_emulated_s_kernel_with_several_chunks_of_index_tiles(E):
    """b = 600 at tile 16: 38 x 38 tiles, 27 chunks of up to two index tiles -- the finish adds only the live chunks of an output"""
    fid, b = 1, 600
    p = fc.FIELDS[fid]
    rng = random.Random(600)
    ops = [biased(p, b, rng) for _ in range(4)]
    ops[2][b // 2:] = [0] * (b - b // 2)
    gamma = rng.randrange(p)
    assert s_plan(b, 16)[2] > 1 and s_plan(b, 16)[3] > 1
    assert emul(E, fid, ops, gamma, 16) == MP.s_definition(p, ops[0], ops[1], ops[2], ops[3], gamma)


# ---- (4) the host algebra of the batch opening, a stand-alone program built with the sanitizers -------------------------------------------
HOST_SRC = os.path.join(ROOT, "tests", "cpp", "mercury_host_test.cpp")
HOST_BIN = os.path.join(ROOT, "tests", "cpp", "mercury_host_test.bin")


@pytest.fixture(scope="module")
def opening():
    """built with the sanitizers: a stand-alone program with its own main, host code only"""
    deps = [HOST_SRC] + [os.path.join(CSRC, f) for f in ("fp.hpp", "mercury_host.hpp", "host_fp4.hpp")]
    if not os.path.exists(HOST_BIN) or os.path.getmtime(HOST_BIN) < max(os.path.getmtime(x) for x in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", HOST_BIN, HOST_SRC])

    def run(fid, g, h, s, zeta, alpha, beta, z, mont=False):
        inp = "\n".join("%064x" % v for v in list(g) + list(h) + list(s) + [zeta, alpha, beta, z])
        return subprocess.run([HOST_BIN, "open", str(fid), str(len(g)), str(int(mont))], input=inp, capture_output=True, text=True, check=True).stdout.split()
    run.self_test = lambda: subprocess.run([HOST_BIN, "self"], capture_output=True, text=True, check=True).stdout.split()
    return run


def restated_opening(p, g, h, s, zeta, alpha, beta, z):
    d = g[::-1]
    zi = pow(zeta, -1, p)
    E_ = lambda f, x: MC.UniPoly(f, p).evaluate(x)  # noqa: E731
    names = ("g_zeta", "g_zeta_inv", "h_zeta", "h_zeta_inv", "h_alpha", "s_zeta", "s_zeta_inv", "d_zeta")
    vals = (E_(g, zeta), E_(g, zi), E_(h, zeta), E_(h, zi), E_(h, alpha), E_(s, zeta), E_(s, zi), E_(d, zeta))
    ev = dict(zip(names, vals), zeta=zeta, zeta_inv=zi, alpha=alpha)
    _, _, W, Wp = MP.generate_batch_evaluate_arg(p, lambda f: None, ev, (g, h, s, d), beta, lambda cw: z)
    return list(vals), W, Wp


@pytest.mark.parametrize("b", [2, 4, 8, 64])
def test_host_algebra_equals_the_restated_batch_opening(opening, b):
    for fid, p in sorted(fc.FIELDS.items()):
        rng = random.Random(10 * b + fid)
        g, h = [rng.randrange(p) for _ in range(b)], [rng.randrange(p) for _ in range(b // 2)] + [0] * (b - b // 2)
        s = [rng.randrange(p) for _ in range(b - 1)]
        zeta, alpha = rng.randrange(2, p - 1), rng.randrange(p)
        zi = pow(zeta, -1, p)
        for beta, z in ((rng.randrange(p), rng.randrange(p)), (0, rng.randrange(p)), (rng.randrange(p), alpha), (1, zeta), (p - 1, zi), (0, 0)):
            for al in (alpha, 0):
                vals, W, Wp = restated_opening(p, g, h, s, zeta, al, beta, z)
                out = opening(fid, g, h, s, zeta, al, beta, z)
                iw, ip = out.index("W"), out.index("Wp")
                assert [int(x, 16) for x in out[:iw]] == vals
                assert [int(x, 16) for x in out[iw + 1:ip]] == W and [int(x, 16) for x in out[ip + 1:]] == Wp, (fid, b, beta, z, al)
                assert len(W) == len(Wp) == b - 1
        # Montgomery words in, Montgomery words out
        m = lambda x: x * R256 % p  # noqa: E731
        vals, W, Wp = restated_opening(p, g, h, s, zeta, alpha, beta, z)
        out = opening(fid, [m(x) for x in g], [m(x) for x in h], [m(x) for x in s], m(zeta), m(alpha), m(beta), m(z), mont=True)
        assert [int(x, 16) for x in out if x not in ("W", "Wp")] == [m(x) for x in vals + W + Wp]


def test_host_algebra_refuses_the_degenerate_challenges(opening):
    assert opening.self_test()[-1] == "ok"
    fid, b = 1, 4
    p = fc.FIELDS[fid]
    rng = random.Random(4)
    g, h, s = ([rng.randrange(p) for _ in range(n)] for n in (b, b, b - 1))
    z7 = 777
    for zeta, alpha in ((0, 5), (1, 5), (p - 1, 5), (z7, z7), (z7, pow(z7, -1, p))):
        assert opening(fid, g, h, s, zeta, alpha, 3, 4) == ["degenerate"], (zeta, alpha)
    for zeta, alpha in ((z7, 0), (z7, 1), (2, p - 1)):                          # alpha = 0 and alpha = +-1 are fine when zeta is not
        assert opening(fid, g, h, s, zeta, alpha, 3, 4)[0] != "degenerate"
