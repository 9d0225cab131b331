"""nmx_mercury_h_poly / nmx_mercury_divide_by_binomial without a GPU.  (1) The yardstick first: tests/mercury_common (the reference's
compute_h_poly, divide_by_binomial with expand / transpose / trim, and the quot_f block, restated line by line in Python integers) against
the closed forms of the header and against the reference's own debug identities -- these tests exercise tests/mercury_common.py alone, do
not touch the library and so pass without the feature; they are there because every other check leans on that file.  (2) Both entry points are declared with the header's
parameter lists, exported, bound in Python / C++ / Rust, and every argument error of the header returns with no device present and
nothing written.  (3) The lane bodies of the kernels (nova_amd/csrc/mercury.hpp) run thread by thread under tests/host_emul/simt.hpp with
limb bounds asserted, against the restatement byte for byte: the three division passes with the kernels' own thread -> (segment, column)
map at several segment lengths, the lane sums of h, and the prologue's conversion of eq_col.  (4) The host-side plan of the division
(mercury_plan, mercury_alpha_pow) as a stand-alone g++ program (tests/cpp/mercury_mirror_test.cpp) against Python.
What the emulation does NOT run: the wave reduction of k_mercury_h (shuffles: the lane sums are added up here in Python), its LDS staging
of the table, the launches and the host half of the calls (staging, the choice of the segment length); tests/test_gpu_mercury.py covers
those."""
import ctypes
import inspect
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests import fv_common as fc
from tests import mercury_common as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nova_amd", "csrc")
H_PARAMS = ["int field_id", "const void* f", "size_t n_rows", "size_t n_cols", "const void* eq_col", "uint32_t flags", "void* out_h"]
D_PARAMS = ["int field_id", "const void* f", "size_t n_rows", "size_t n_cols", "const void* alpha", "uint32_t flags", "void* out_q", "void* out_g"]
SHAPES = [(1, 1), (1, 4), (2, 1), (2, 4), (3, 5), (5, 3), (4, 4), (4, 8), (8, 8), (17, 65)]


@pytest.fixture(scope="module")
def L():
    from nova_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def instance(p, n_rows, n_cols, seed, fill=None):
    rng = random.Random(seed)
    val = (lambda: fill) if fill is not None else (lambda: rng.choice([0, 1, p - 1, p - 2]) if rng.random() < 0.15 else rng.randrange(p))
    return [val() for _ in range(n_rows * n_cols)], [val() for _ in range(n_cols)]


# ---- (1) the yardstick -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows,n_cols", SHAPES)
def test_restatement_equals_the_closed_forms_and_the_references_identities(n_rows, n_cols):
    p = fc.FIELDS[1]
    f, eq = instance(p, n_rows, n_cols, 7 * n_rows + n_cols)
    for alpha in (random.Random(n_rows).randrange(p), 0, 1, p - 1):
        h, q, g = mc.restate(p, f, n_rows, n_cols, eq, alpha)           # (checks f(r) = (r^b - alpha) q(r) + g(r) and <eq_col, g> = h(alpha))
        assert g == [sum(f[j * n_cols + c] * pow(alpha, j, p) for j in range(n_rows)) % p for c in range(n_cols)]
        assert q == [sum(f[j * n_cols + c] * pow(alpha, j - k - 1, p) for j in range(k + 1, n_rows)) % p for k in range(n_rows - 1) for c in range(n_cols)]
        assert len(q) == (n_rows - 1) * n_cols and len(g) == n_cols and len(h) == n_rows
        zeta = random.Random(n_cols).randrange(1, p)
        g_zeta = mc.UniPoly(g, p).evaluate(zeta)
        quot, rem = mc.quot_f(p, f, mc.trimmed(p, q), zeta, n_cols, alpha, g_zeta)
        mc.check_quot_f(p, f, q, quot, rem, zeta, n_cols, alpha, g_zeta, random.Random(5).randrange(p))
        # ... and the form the library composes it in: suffix Horner of f - (zeta^b - alpha) q, whose out[0] is g(zeta)
        t = list(f)
        for i, x in enumerate(q):
            t[i] = (t[i] - (pow(zeta, n_cols, p) - alpha) * x) % p
        out = [0] * (len(t) + 1)
        for i in reversed(range(len(t))):
            out[i] = (t[i] + zeta * out[i + 1]) % p
        assert out[0] == g_zeta and out[1:len(t)] == quot


def test_eval_identity_of_h_on_the_references_shapes():
    p = fc.FIELDS[1]
    for log_n in (4, 5):                                                  # even, and odd: b_row = b / 2 (mercury.rs:919-931)
        rng = random.Random(log_n)
        point = [rng.randrange(p) for _ in range(log_n)]
        f = [rng.randrange(p) for _ in range(1 << log_n)]
        ev = sum(a * b for a, b in zip(f, mc.eq_evals(p, point))) % p
        pt = ([0] + point) if log_n % 2 else point
        log_b = len(pt) // 2
        b, b_row = 1 << log_b, (1 << log_n) >> log_b
        eq_row, eq_col = mc.eq_evals(p, pt[:log_b]), mc.eq_evals(p, pt[log_b:])
        mc.check_h_against_eval(p, eq_row, mc.compute_h_poly(p, f, eq_col, b_row, b), ev)


# ---- (2) the surface ----------------------------------------------------------------------------------------------------------------
def test_header_declares_library_exports_and_python_binds_the_same_types(L):
    hdr = open(os.path.join(ROOT, "include", "nova_mi355x.h")).read()
    ctype_of = lambda d: (ctypes.c_int if d.startswith("int ") else ctypes.c_size_t if d.startswith("size_t") else ctypes.c_uint32  # noqa: E731
                          if d.startswith("uint32_t") else ctypes.c_void_p)
    for name, want in (("nmx_mercury_h_poly", H_PARAMS), ("nmx_mercury_divide_by_binomial", D_PARAMS)):
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert m, "the header does not declare " + name
        assert [re.sub(r"/\*.*?\*/", "", x).strip() for x in re.sub(r"\s+", " ", m.group(1)).split(",")] == want
        assert hasattr(L, name)
        assert list(getattr(L, name).argtypes) == [ctype_of(d) for d in want]
    sect = hdr.split("Mercury's prover passes")[1].split("int nmx_eq_evals_from_points(")[0]
    for needle in ("mercury.rs:369-386", "mercury.rs:319-356", ":281-288", ":291-312", "mercury.rs:1163-1180", "AFTER its transpose", "(n_rows - 1) * n_cols",
                   "trim()", "out_q or out_g with f", "out_q with out_g", "out_h", "NMX_E_ARG", "NMX_E_TOO_LARGE", "NMX_E_SCALAR_RANGE", "NMX_ASYNC",
                   "NMX_SCALARS_MONT", "always a host pointer", "nothing is written", "mercury_seg_rows", "canonical"):
        assert needle in sect, needle
    assert '"mercury_seg_rows"' in hdr.split("int nmx_set_option(")[0].rsplit("/*", 1)[1]
    ffi = open(os.path.join(ROOT, "bindings", "rust", "nova-mi355x-sys", "src", "ffi.rs")).read()
    assert "pub fn nmx_mercury_h_poly(" in ffi and "pub fn nmx_mercury_divide_by_binomial(" in ffi, "ffi.rs: regenerate with scripts/gen_rust_sys.py"


def test_python_and_cpp_wrappers_exist():
    from nova_amd import fieldvec as fv
    assert list(inspect.signature(fv.mercury_h_poly).parameters) == ["field", "f", "n_rows", "n_cols", "eq_col", "mont", "async_"]
    assert list(inspect.signature(fv.mercury_divide_by_binomial).parameters) == ["field", "f", "n_rows", "n_cols", "alpha", "mont", "async_"]
    assert list(inspect.signature(fv.mercury_quot_f).parameters) == ["field", "f", "q", "zeta_b_minus_alpha", "zeta", "mont"]
    assert fv.FIELD_MODULUS == fc.FIELDS
    res = open(os.path.join(ROOT, "include", "nova_mi355x.hpp")).read().split("namespace resident {")[1]
    for decl in ("inline void mercury_h_poly(int field", "inline void mercury_divide_by_binomial(int field", "inline Scalar mercury_quot_f(int field"):
        assert decl in res, decl


def test_the_option_is_known(L):
    """nmx_set_option applies the environment's defaults first and so needs a device: without one only the refusal can be checked here
    (tests/test_gpu_mercury.py sets the option and requires identical bytes at every value)"""
    from nova_amd import _lib
    ok = 0 if L.nmx_device_count() > 0 else _lib.E_NO_DEVICE
    assert L.nmx_set_option(b"mercury_seg_rows", 4) == ok and L.nmx_set_option(b"mercury_seg_rows", 0) == ok
    assert L.nmx_set_option(b"mercury_seg_cols", 4) != 0
    assert 'n == "mercury_seg_rows"' in open(os.path.join(CSRC, "capi.hip")).read()


def test_argument_errors_need_no_device_and_write_nothing(L):
    from nova_amd import _lib
    fid, R_, C_ = 1, 3, 4
    p = fc.FIELDS[fid]
    buf = np.ascontiguousarray(fc.rand_vec(fid, 64, 3).copy())      # f = [0, 12), eq = [12, 16), h = [16, 19), q = [20, 28), g = [28, 32)
    before = buf.copy()
    at = lambda i: buf.ctypes.data + 32 * i  # noqa: E731
    al = fc.vec([5]).copy()

    def h(field=fid, f=at(0), r=R_, c=C_, eq=at(12), flags=0, out=at(16)):
        return L.nmx_mercury_h_poly(field, f, r, c, eq, flags, out)

    def d(field=fid, f=at(0), r=R_, c=C_, alpha=al.ctypes.data, flags=0, q=at(20), g=at(28)):
        return L.nmx_mercury_divide_by_binomial(field, f, r, c, alpha, flags, q, g)
    A, TL = _lib.E_ARG, _lib.E_TOO_LARGE
    assert h(f=None) == A and h(eq=None) == A and h(out=None) == A
    assert d(f=None) == A and d(alpha=None) == A and d(g=None) == A and d(q=None) == A
    assert h(r=0) == A and h(c=0) == A and d(r=0) == A and d(c=0) == A
    assert h(field=4) == A and h(field=-1) == A and d(field=4) == A and d(field=-1) == A
    assert b"bad field id" in L.nmx_last_error()
    for fl in (_lib.BASES_MONT, _lib.BASES_DEVICE, _lib.OUT_PARTIAL, 1 << 20):
        assert h(flags=fl) == A and d(flags=fl) == A, fl
    assert h(r=1 << 16, c=1 << 16) == TL and d(r=1 << 16, c=1 << 16) == TL              # n_rows * n_cols = 2^32
    assert h(r=1 << 33, c=1 << 33) == TL and d(r=(1 << 63) + 1, c=2) == TL              # ... and overflowing size_t
    big = fc.vec([p]).copy()
    assert d(alpha=big.ctypes.data) == _lib.E_SCALAR_RANGE
    assert b"alpha" in L.nmx_last_error()
    big = fc.vec([(1 << 256) - 1]).copy()
    assert d(alpha=big.ctypes.data) == _lib.E_SCALAR_RANGE
    # overlaps: out_q or out_g with f, out_q with out_g, out_h with f or with eq_col -- by one element at either end, and in place
    assert d(q=at(0)) == A and d(q=at(11)) == A and d(g=at(0)) == A and d(g=at(11)) == A
    assert b"overlap" in L.nmx_last_error()
    assert d(f=at(32), q=at(25), g=at(50)) == A                         # q's last element is f's first
    assert d(q=at(20), g=at(27)) == A and d(q=at(20), g=at(17)) == A   # g over q's tail / g's tail over q's head
    assert h(out=at(0)) == A and h(out=at(11)) == A and h(out=at(12)) == A and h(out=at(15)) == A and h(f=at(18)) == A
    # n_rows == 1: q is empty -- a NULL out_q is fine and an out_q "inside" f overlaps nothing
    with_device = L.nmx_device_count() > 0
    ok = 0 if with_device else _lib.E_NO_DEVICE
    assert (buf == before).all(), "a refused call wrote something"
    assert d(r=1, q=None) == ok and d(r=1, q=at(0)) == ok
    # well-formed calls get past every check: what stops them without a device is NMX_E_NO_DEVICE, nothing else
    assert h() == ok and d() == ok and h(flags=_lib.SCALARS_MONT) == ok and d(flags=_lib.ASYNC) == ok
    if not with_device:
        assert (buf == before).all()


# ---- (3) the kernels' lane bodies under the emulation --------------------------------------------------------------------------------
EMUL_SRC = os.path.join(ROOT, "tests", "host_emul", "mercury_emul.cpp")
EMUL_SO = os.path.join(ROOT, "tests", "host_emul", "libnmx_mercury_emul.so")
RI = 1 << 261          # the internal residue form: x * 2^261 mod p (nova_amd/csrc/fp.hpp)
R256 = 1 << 256        # the Montgomery form of NMX_SCALARS_MONT


@pytest.fixture(scope="module")
def E():
    deps = [EMUL_SRC, os.path.join(ROOT, "tests", "host_emul", "simt.hpp")] + [os.path.join(CSRC, f) for f in ("fp.hpp", "mercury.hpp", "spmv_row.hpp",
                                                                                                            "msm_partition.hpp")]
    if not os.path.exists(EMUL_SO) or os.path.getmtime(EMUL_SO) < max(os.path.getmtime(x) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", EMUL_SO, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_SO)
    vp, u32, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    lib.emul_mercury_div.argtypes = [i, vp, u32, u32, u32, vp, vp, vp, vp, vp]
    lib.emul_mercury_h.argtypes = [i, vp, u32, u32, vp, vp]
    lib.emul_mercury_eq.argtypes = [i, vp, u32, u32, vp]
    return lib


def words(vals):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in vals) or bytes(32), np.uint32).copy()


def emul_div(E, fid, f, n_rows, n_cols, alpha, seg_rows):
    p = fc.FIELDS[fid]
    segs = (n_rows + seg_rows - 1) // seg_rows
    fw, aw, asw = words(f), words([alpha * RI % p]), words([pow(alpha, seg_rows, p) * RI % p])
    q = np.full(8 * max((n_rows - 1) * n_cols, 1) + 8, 0xdeadbeef, np.uint32)   # (one element of slack: nothing may land there)
    g = np.full(8 * n_cols + 8, 0xdeadbeef, np.uint32)
    tot = np.zeros(8 * segs * n_cols, np.uint32)
    assert E.emul_mercury_div(fid, fw.ctypes.data, n_rows, n_cols, seg_rows, aw.ctypes.data, asw.ctypes.data, q.ctypes.data, g.ctypes.data, tot.ctypes.data) == 0
    nq = (n_rows - 1) * n_cols
    assert (q[8 * nq:] == 0xdeadbeef).all() and (g[8 * n_cols:] == 0xdeadbeef).all(), "a store past the end of q / g"
    return fc.ints(q[:8 * nq].view(np.uint8)) if nq else [], fc.ints(g[:8 * n_cols].view(np.uint8))


def emul_h(E, fid, f, n_rows, n_cols, eq, mont=False):
    p = fc.FIELDS[fid]
    fw, ew = words(f), words(eq)
    eqi = np.zeros(8 * n_cols, np.uint32)
    assert E.emul_mercury_eq(fid, ew.ctypes.data, n_cols, 1 if mont else 0, eqi.ctypes.data) == 0
    form = R256 if mont else 1
    table = fc.ints(np.ascontiguousarray(eqi.reshape(8, n_cols).T).view(np.uint8))      # stored [word][column]
    assert table == [e * pow(form, -1, p) * RI % p for e in eq], "MercuryEqFn: the table in the internal form, canonical"
    lanes = np.zeros(8 * 64 * n_rows, np.uint32)
    assert E.emul_mercury_h(fid, fw.ctypes.data, n_rows, n_cols, eqi.ctypes.data, lanes.ctypes.data) == 0
    sums = fc.ints(lanes.view(np.uint8))
    assert all(s < p for s in sums), "a lane's sum is not the canonical representative"
    return [sum(sums[64 * r:64 * r + 64]) % p for r in range(n_rows)]


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
def test_emulated_division_at_every_segment_length(E, fid):
    p = fc.FIELDS[fid]
    n_rows, n_cols = 13, 300                                        # two column blocks, the second partial; 13 rows: a short top segment
    f, _eq = instance(p, n_rows, n_cols, 40 + fid)
    f[0], f[1], f[n_cols], f[-1] = 0, p - 1, p - 1, 0
    for alpha in (0, 1, p - 1, random.Random(fid).randrange(p)):
        qw, gw = mc.divide_by_binomial(p, f, n_rows, n_cols, alpha)
        want = (mc.q_in_abi_layout(qw, n_rows, n_cols), gw)
        for seg_rows in (1, 2, 4, 5, 12, 13, 64):
            assert emul_div(E, fid, f, n_rows, n_cols, alpha, min(seg_rows, n_rows)) == want, (alpha, seg_rows)


@pytest.mark.parametrize("n_rows,n_cols", [(1, 1), (1, 4), (2, 1), (2, 4), (3, 5), (5, 3), (17, 65), (33, 63), (16, 16), (8, 16), (40, 257)])
def test_emulated_division_shapes(E, n_rows, n_cols):
    for fid in (1, 2):
        p = fc.FIELDS[fid]
        f, _eq = instance(p, n_rows, n_cols, n_rows * 1000 + n_cols)
        alpha = random.Random(n_cols).randrange(p)
        qw, gw = mc.divide_by_binomial(p, f, n_rows, n_cols, alpha)
        want = (mc.q_in_abi_layout(qw, n_rows, n_cols), gw)
        for seg_rows in {1, 3, 8, n_rows}:                         # batches of eight rows with and without a remainder
            assert emul_div(E, fid, f, n_rows, n_cols, alpha, min(seg_rows, n_rows)) == want


def test_emulated_division_bounds_at_their_worst(E):
    """every coefficient p - 1 with alpha = p - 1, all zero, and words that are no field elements (2^256 - 1: the header allows any 256-bit word)"""
    for fid in sorted(fc.FIELDS):
        p = fc.FIELDS[fid]
        for fill, alpha in ((p - 1, p - 1), (0, p - 1), ((1 << 256) - 1, p - 1), ((1 << 256) - 1, 1)):
            f = [fill] * (19 * 70)
            qw, gw = mc.divide_by_binomial(p, [x % p for x in f], 19, 70, alpha)
            assert emul_div(E, fid, f, 19, 70, alpha, 19) == (mc.q_in_abi_layout(qw, 19, 70), gw)
            assert emul_div(E, fid, f, 19, 70, alpha, 4) == (mc.q_in_abi_layout(qw, 19, 70), gw)


def test_emulated_division_of_montgomery_words(E):
    fid = 1
    p = fc.FIELDS[fid]
    f, _eq = instance(p, 9, 20, 77)
    alpha = 123456789
    qw, gw = mc.divide_by_binomial(p, f, 9, 20, alpha)
    m = lambda v: [x * R256 % p for x in v]  # noqa: E731
    # the kernel is handed alpha in the internal form either way: Montgomery words in, Montgomery words out
    assert emul_div(E, fid, m(f), 9, 20, alpha, 4) == (m(mc.q_in_abi_layout(qw, 9, 20)), m(gw))


@pytest.mark.parametrize("n_rows,n_cols", [(1, 1), (2, 4), (5, 3), (4, 64), (3, 65), (2, 449), (6, 1024)])
def test_emulated_h_lanes(E, n_rows, n_cols):
    for fid in ((0, 1, 2, 3) if n_cols < 100 else (1,)):
        p = fc.FIELDS[fid]
        f, eq = instance(p, n_rows, n_cols, 3 * n_rows + n_cols + fid)
        assert emul_h(E, fid, f, n_rows, n_cols, eq) == mc.compute_h_poly(p, f, eq, n_rows, n_cols)
        fm, em = [x * R256 % p for x in f], [x * R256 % p for x in eq]
        assert emul_h(E, fid, fm, n_rows, n_cols, em, mont=True) == [x * R256 % p for x in mc.compute_h_poly(p, f, eq, n_rows, n_cols)]


def test_emulated_h_bounds_at_their_worst(E):
    """f AND eq_col may be any 256-bit words (the header): p - 1, 0 and 2^256 - 1 in either"""
    top = (1 << 256) - 1
    for fid in sorted(fc.FIELDS):
        p = fc.FIELDS[fid]
        for fill, efill in ((p - 1, p - 1), (0, p - 1), (top, p - 1), (top, top), (p - 1, top), (p, p + 1)):   # 15 terms per lane: the cadence of six
            f, eq = [fill] * (2 * 64 * 15), [efill] * (64 * 15)
            assert emul_h(E, fid, f, 2, 64 * 15, eq) == mc.compute_h_poly(p, [x % p for x in f], [x % p for x in eq], 2, 64 * 15), (fid, fill, efill)


# ---- (4) the host-side plan ----------------------------------------------------------------------------------------------------------
MIRROR_SRC = os.path.join(ROOT, "tests", "cpp", "mercury_mirror_test.cpp")
MIRROR_BIN = os.path.join(ROOT, "tests", "cpp", "mercury_mirror_test.bin")


@pytest.fixture(scope="module")
def mirror():
    """built with the sanitizers: a stand-alone program with its own main, host code only"""
    deps = [MIRROR_SRC] + [os.path.join(CSRC, f) for f in ("fp.hpp", "mercury.hpp")]
    if not os.path.exists(MIRROR_BIN) or os.path.getmtime(MIRROR_BIN) < max(os.path.getmtime(x) for x in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", MIRROR_BIN, MIRROR_SRC])
    return lambda *a: subprocess.run([MIRROR_BIN] + [str(x) for x in a], capture_output=True, text=True, check=True).stdout.split()


def py_plan(n_rows, n_cols, opt):
    """the plan restated: 2^16 lanes, at most 64 segments, at least 4 rows per segment unless the option says otherwise"""
    if opt:
        R_ = min(opt, n_rows)
    else:
        want = min(max((1 << 16) // n_cols, 1), 64)
        R_ = min(max(-(-n_rows // want), 4), n_rows)
    if -(-n_rows // R_) > 65535:
        R_ = -(-n_rows // 65535)
    S_ = -(-n_rows // R_)
    return [R_, S_, n_rows - (S_ - 1) * R_]


def test_plan_matches_python(mirror):
    assert mirror("self") == ["mercury", "mirror", "ok"]
    shapes = SHAPES + [(16, 16), (8, 16), (32, 32), (64, 64), (32, 64), (512, 1024), (1024, 1024), (2048, 2048), (1024, 2048), (64, 4), (4, 64), (33, 63),
                       (1 << 20, 1), (1, 1 << 20), (3, 1 << 17), (100000, 7)]
    for n_rows, n_cols in shapes:
        for opt in (0, 1, 3, 4, n_rows, n_rows + 1):
            got = [int(x) for x in mirror("plan", n_rows, n_cols, opt)]
            assert got == py_plan(n_rows, n_cols, opt), (n_rows, n_cols, opt)
            R_, S_, last = got
            assert (S_ - 1) * R_ + last == n_rows and 1 <= last <= R_ and S_ <= 65535
    assert [int(x) for x in mirror("plan", 1024, 1024, 0)] == [16, 64, 16]     # 2^20: 64 segments of 16 rows, 2^16 lanes
    assert [int(x) for x in mirror("plan", 512, 1024, 0)] == [8, 64, 8]        # 2^19, the odd-log_n shape


def test_alpha_powers_match_python(mirror):
    for fid in sorted(fc.FIELDS):
        p = fc.FIELDS[fid]
        for alpha in (0, 1, p - 1, random.Random(fid).randrange(p)):
            for e in (0, 1, 2, 4, 16, 1000, 65535, (1 << 32) - 1):
                assert int(mirror("pow", fid, "%064x" % alpha, e)[0], 16) == pow(alpha, e, p), (fid, alpha, e)
