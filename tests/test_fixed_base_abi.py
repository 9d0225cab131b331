"""nmx_bases_from_scalars / nmx_bases_setup_from_tau without a GPU.  (1) Both entry points are declared with the issue's parameter lists,
exported, bound in Python / C++ / Rust (the C++ wrappers also compiled and run, tests/cpp/fixed_base_mirror_test.cpp), and the header names
the reference's line ranges and every error code.  (2) Every refusal that needs no device returns its code with no device present and
leaves *handle untouched.  (3) The kernels of nova_amd/csrc/fixed_base.hpp run thread by thread under tests/host_emul/simt.hpp with limb
bounds asserted, bit-exact against pyref.mul(c, s % r, B) on all four curves: the table build at c = 4, 8 and 13, the multiplication pass
with its block normalisation at n = 1, 2, 255, 256, 257, the edge scalars, identity lanes, an all-identity block, tau mode with a shard's
`begin`, Montgomery words, and a scalar that is not below r.  What the emulation does NOT run: the launches, the staging of host scalars,
the key's own MSM tables, sharding; tests/test_gpu_fixed_base.py covers those."""
import ctypes
import inspect
import os
import random
import re
import subprocess

import numpy as np
import pytest

from oracle import pyref as R
from tests import fixed_base_common as fb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nova_amd", "csrc")
S_PARAMS = ["int curve", "const void* base_xy64", "const void* scalars", "size_t n", "uint32_t flags", "uint64_t* handle"]
T_PARAMS = ["int curve", "const void* tau32", "size_t n", "uint32_t flags", "uint64_t* handle"]
CURVE_IDS = [c.name for c in fb.CURVES]


@pytest.fixture(scope="module")
def L():
    from nova_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- (1) the surface ----------------------------------------------------------------------------------------------------------------
def test_header_declares_library_exports_and_python_binds_the_same_types(L):
    hdr = open(os.path.join(ROOT, "include", "nova_mi355x.h")).read()
    ctype_of = lambda d: (ctypes.c_int if d.startswith("int ") else ctypes.c_size_t if d.startswith("size_t") else ctypes.c_uint32  # noqa: E731
                          if d.startswith("uint32_t ") else ctypes.POINTER(ctypes.c_uint64) if d.startswith("uint64_t*") else ctypes.c_void_p)
    for name, want in (("nmx_bases_from_scalars", S_PARAMS), ("nmx_bases_setup_from_tau", T_PARAMS)):
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert m, "the header does not declare " + name
        assert [x.strip() for x in re.sub(r"\s+", " ", m.group(1)).split(",")] == want
        assert hasattr(L, name)
        assert list(getattr(L, name).argtypes) == [ctype_of(d) for d in want]
    assert hdr.index("int nmx_bases_generate(") < hdr.index("int nmx_bases_from_scalars(") < hdr.index("int nmx_bases_setup_from_tau(") < hdr.index("int nmx_msm(")
    doc = hdr.split("int nmx_bases_from_scalars(")[0].rsplit("/* ---- fixed-base keys", 1)[1]
    for needle in ("hyperkzg.rs:357-410", ":565-567", ":443-", "setup_from_tau_direct", "fixed_base_exp_comb_batch", "NMX_E_ARG", "NMX_E_POINT",
                   "NMX_E_SCALAR_RANGE", "NMX_SCALARS_MONT", "NMX_SCALARS_DEVICE", "NMX_BASES_MONT", "NMX_BASES_PRECOMPUTE", "*handle untouched",
                   "n >= 2^31", "identity", "from_label", "tau_H", "fixed_base_c", "begin"):
        assert needle in doc, needle
    assert '"fixed_base_c"' in hdr.split("int nmx_set_option(")[0].rsplit("/*", 1)[1]
    ffi = open(os.path.join(ROOT, "bindings", "rust", "nova-mi355x-sys", "src", "ffi.rs")).read()
    assert "pub fn nmx_bases_from_scalars(" in ffi and "pub fn nmx_bases_setup_from_tau(" in ffi, "ffi.rs: regenerate with scripts/gen_rust_sys.py"


def test_python_and_cpp_wrappers_exist():
    from nova_amd import provider as P
    assert list(inspect.signature(P.CommitmentKey.from_scalars).parameters) == ["curve", "scalars", "base", "h_xy64", "mont", "precompute"]
    assert list(inspect.signature(P.CommitmentKey.setup_from_tau).parameters) == ["curve", "n", "tau", "h_xy64", "mont", "precompute"]
    assert list(inspect.signature(P.CommitmentEngine.setup_from_tau).parameters)[:3] == ["self", "n", "tau"]
    hpp = open(os.path.join(ROOT, "include", "nova_mi355x.hpp")).read()
    key = hpp.split("class CommitmentKey {")[1].split("template <int CURVE> struct DlogGroupExt")[0]
    assert key.index("static CommitmentKey generate(") < key.index("static CommitmentKey from_scalars(") < key.index("static CommitmentKey setup_from_tau(")
    assert '#include "fixed_base.hpp"' in open(os.path.join(CSRC, "runtime.hpp")).read()
    assert "&generate, &fixed_base," in open(os.path.join(CSRC, "curve_impl.hpp")).read()


# ---- (2) refusals -----------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5EEDFACE0BADF00D


def _call(L, which, curve=0, base=None, scalars="ok", tau="ok", n=4, flags=0, handle="ok"):
    from nova_amd import _lib  # noqa: F401
    c = R.CURVES_BY_ID.get(curve, R.BN254_G1)
    h = ctypes.c_uint64(SENTINEL)
    hp = None if handle is None else ctypes.byref(h)
    if which == "scalars":
        sc = fb.scalar_rows(c, [5, 6, 7, 8]) if isinstance(scalars, str) else scalars
        rc = L.nmx_bases_from_scalars(curve, None if base is None else base.ctypes.data, None if sc is None else sc.ctypes.data, n, flags, hp)
    else:
        t = fb.scalar_rows(c, [9]) if isinstance(tau, str) else tau
        rc = L.nmx_bases_setup_from_tau(curve, None if t is None else t.ctypes.data, n, flags, hp)
    assert h.value == SENTINEL, "a refused call wrote *handle"
    return rc


def test_refusals_need_no_device_and_leave_the_handle_untouched(L):
    from nova_amd import _lib
    A, PT, SR = _lib.E_ARG, _lib.E_POINT, _lib.E_SCALAR_RANGE
    for which in ("scalars", "tau"):
        assert _call(L, which, n=0) == A and _call(L, which, n=1 << 31) == A and _call(L, which, n=(1 << 63) + 5) == A
        assert _call(L, which, handle=None) == A
        assert _call(L, which, curve=4) == A and _call(L, which, curve=-1) == A
        for fl in (_lib.BASES_DEVICE, _lib.OUT_PARTIAL, _lib.BASES_VALIDATE, _lib.ASYNC, 1 << 20, 1 << 31):
            assert _call(L, which, flags=fl) == A, (which, fl)
    assert _call(L, "scalars", scalars=None) == A and _call(L, "tau", tau=None) == A
    # flags that belong to the other call only
    assert _call(L, "tau", flags=_lib.SCALARS_DEVICE) == A and _call(L, "tau", flags=_lib.BASES_MONT) == A
    # the base: not canonical, off the curve, the identity -- in the form NMX_BASES_MONT names
    for c in fb.CURVES:
        G7 = R.mul(c, 7, (c.gx, c.gy))
        off = fb.base_bytes(c, (G7[0], (G7[1] + 1) % c.p))
        big = np.frombuffer(int(c.p).to_bytes(32, "little") + int(G7[1]).to_bytes(32, "little"), np.uint8).copy()
        for bad in (off, big, np.zeros(64, np.uint8)):
            assert _call(L, "scalars", curve=c.cid, base=bad) == PT, c.name
        assert _call(L, "scalars", curve=c.cid, base=fb.base_bytes(c, G7, mont=False), flags=_lib.BASES_MONT) == PT   # canonical bytes read as Montgomery
        assert _call(L, "scalars", curve=c.cid, base=np.zeros(64, np.uint8), flags=_lib.BASES_MONT) == PT
        # host scalars and tau at and above r, in either form, at either end
        for bad in (c.r, c.r + 1, (1 << 256) - 1):
            for pos in (0, 3):
                sc = fb.scalar_rows(c, [5, 6, 7, 8])
                sc[pos] = np.frombuffer(int(bad).to_bytes(32, "little"), np.uint8)
                for fl in (0, _lib.SCALARS_MONT):
                    assert _call(L, "scalars", curve=c.cid, scalars=sc, flags=fl) == SR, (c.name, hex(bad), pos)
            t = np.frombuffer(int(bad).to_bytes(32, "little"), np.uint8).copy()
            assert _call(L, "tau", curve=c.cid, tau=t) == SR and _call(L, "tau", curve=c.cid, tau=t, flags=_lib.SCALARS_MONT) == SR
    # a well-formed call gets past every check: what stops it without a device is NMX_E_NO_DEVICE, nothing else
    if L.nmx_device_count() <= 0:
        for c in fb.CURVES:
            G7 = R.mul(c, 7, (c.gx, c.gy))
            assert _call(L, "scalars", curve=c.cid) == _lib.E_NO_DEVICE and _call(L, "tau", curve=c.cid, flags=_lib.BASES_PRECOMPUTE) == _lib.E_NO_DEVICE
            assert _call(L, "scalars", curve=c.cid, base=fb.base_bytes(c, G7)) == _lib.E_NO_DEVICE
            assert _call(L, "scalars", curve=c.cid, base=fb.base_bytes(c, G7, mont=True), flags=_lib.BASES_MONT | _lib.SCALARS_MONT) == _lib.E_NO_DEVICE
        assert L.nmx_set_option(b"fixed_base_c", 8) == _lib.E_NO_DEVICE


# ---- (3) the kernels under the emulation -------------------------------------------------------------------------------------------------
EMUL_SRC = os.path.join(ROOT, "tests", "host_emul", "fixed_base_emul.cpp")
EMUL_SO = os.path.join(ROOT, "tests", "host_emul", "libnmx_fixed_base_emul.so")
RI = 1 << 261          # the internal residue form: x * 2^261 mod p (nova_amd/csrc/fp.hpp)
SLACK = 0xdeadbeef


@pytest.fixture(scope="module")
def E():
    deps = [EMUL_SRC, os.path.join(ROOT, "tests", "host_emul", "simt.hpp")] + [os.path.join(CSRC, f) for f in ("fp.hpp", "curve.hpp", "curves.hpp", "fixed_base.hpp",
                                                                                                            "msm_partition.hpp", "msm_kernels.hpp")]
    if not os.path.exists(EMUL_SO) or os.path.getmtime(EMUL_SO) < max(os.path.getmtime(x) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", EMUL_SO, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_SO)
    vp, u32, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    lib.emul_fb_table.argtypes = [i, u32, vp, vp, vp]
    lib.emul_fb_mul.argtypes = [i, u32, vp, vp, u32, vp, u32, u32, vp, vp]
    lib.emul_fb_geometry.argtypes = [i, u32, vp]
    return lib


def geometry(E, c, cw):
    g = np.zeros(4, np.uint32)
    E.emul_fb_geometry(c.cid, cw, g.ctypes.data)
    return [int(x) for x in g]


def points_from_internal(c, words):
    """(m x 16 words: x || y in the internal form, all zero = identity) -> affine tuples / INF"""
    inv = pow(RI, -1, c.p)
    rows = np.ascontiguousarray(words).view(np.uint8).reshape(-1, 64)
    out = []
    for row in rows:
        x, y = int.from_bytes(bytes(row[:32]), "little"), int.from_bytes(bytes(row[32:]), "little")
        assert x < c.p and y < c.p, "a stored coordinate is not canonical"
        out.append(R.INF if x == 0 and y == 0 else (x * inv % c.p, y * inv % c.p))
    return out


_tables = {}


def table(E, c, cw, B=None):
    """the emulated table for (curve, width, base) -> (words, flag word); built once"""
    key = (c.cid, cw, B)
    if key not in _tables:
        W, M, _e, _i = geometry(E, c, cw)
        assert W == fb.windows(c, cw) and M == (1 << cw) - 1
        t = np.full(W * M * 16 + 16, SLACK, np.uint32)
        flags = np.zeros(2, np.uint32)
        flags[1] = SLACK
        b16 = None if B is None else np.ascontiguousarray(fb.base_bytes(c, B)).view(np.uint32)
        assert E.emul_fb_table(c.cid, cw, None if b16 is None else b16.ctypes.data, t.ctypes.data, flags.ctypes.data) == 0
        assert (t[W * M * 16:] == SLACK).all() and flags[1] == SLACK, "a store past the end of the table or of the flag word"
        _tables[key] = (t, int(flags[0]))
    return _tables[key]


def emul_mul(E, c, cw, n, scalars=None, mont=False, tau=None, begin=0, B=None):
    """the multiplication pass over the emulated table -> (points, flag word)"""
    t, _f = table(E, c, cw, B)
    out = np.full(16 * n + 16, SLACK, np.uint32)
    flags = np.zeros(2, np.uint32)
    flags[1] = SLACK
    sc = None if scalars is None else np.ascontiguousarray(scalars).view(np.uint32)
    tw = None if tau is None else np.ascontiguousarray(fb.scalar_rows(c, [tau], mont)).view(np.uint32)
    assert E.emul_fb_mul(c.cid, cw, t.ctypes.data, None if sc is None else sc.ctypes.data, 1 if mont else 0, None if tw is None else tw.ctypes.data,
                         begin, n, out.ctypes.data, flags.ctypes.data) == 0
    assert (out[16 * n:] == SLACK).all() and flags[1] == SLACK, "a store past the end of the key or of the flag word"
    return points_from_internal(c, out[:16 * n]), int(flags[0])


@pytest.mark.parametrize("cw", fb.WIDTHS)
@pytest.mark.parametrize("c", fb.CURVES, ids=CURVE_IDS)
def test_emulated_table_is_every_multiple_of_every_window_base(E, c, cw):
    """T[w][d - 1] = d 2^(cw w) G: both ends and three random entries of EVERY window directly with pyref.mul, and every entry of a window by
    repeated addition of its base (pyref.add) -- in all windows at c = 4 and 8, in the first two, a middle one and the top one at c = 13
    (163 820 entries: the walk in Python integers is what takes the time, not the kernel)"""
    W, M, _e, ident_bit = geometry(E, c, cw)
    t, flags = table(E, c, cw)
    assert flags == 0, "no entry of the table is the identity"
    got = points_from_internal(c, t[:W * M * 16])
    assert R.INF not in got
    G = (c.gx, c.gy)
    rng = random.Random(cw)
    walked = range(W) if cw < 13 else (0, 1, W // 2, W - 1)
    for w in range(W):
        for d in [1, 2, M] + [rng.randrange(1, M + 1) for _ in range(3)]:
            assert got[w * M + d - 1] == R.mul(c, (d << (cw * w)) % c.r, G), (w, d)
        if w in walked:
            Pw, acc = got[w * M], R.INF
            for d in range(1, M + 1):
                acc = R.add(c, acc, Pw)
                assert got[w * M + d - 1] == acc, (w, d)


def test_emulated_table_over_a_callers_base(E):
    for c in (R.GRUMPKIN, R.PALLAS):
        B = R.mul(c, 7, (c.gx, c.gy))
        W, M, _e, _i = geometry(E, c, 4)
        got = points_from_internal(c, table(E, c, 4, B)[0][:W * M * 16])
        rng = random.Random(c.cid)
        for w, d in [(0, 1), (W - 1, M)] + [(rng.randrange(W), rng.randrange(1, M + 1)) for _ in range(40)]:
            assert got[w * M + d - 1] == R.mul(c, (7 * d << (4 * w)) % c.r, (c.gx, c.gy)), (w, d)


@pytest.mark.parametrize("cw", fb.WIDTHS)
@pytest.mark.parametrize("c", fb.CURVES, ids=CURVE_IDS)
def test_emulated_multiplication_of_the_scalar_set(E, c, cw):
    """n = 257 (two blocks, the second with one lane): random scalars, 0, 1, 2, r - 1, 2^cw - 1, the top window alone, every digit at its
    maximum, and lanes 0, 1 and 255 zero; canonical and Montgomery words"""
    _w, _m, err_bit, ident_bit = geometry(E, c, cw)
    s = fb.scalar_set(c, cw, 257)
    assert s[0] == s[1] == s[255] == 0 and s[2] == 0 and s[256] != 0 and set(fb.special_scalars(c, cw)) <= set(s)
    want = fb.expect_points(c, s)
    assert want[0] is R.INF and want[255] is R.INF and want[3] == (c.gx, c.gy) and want[5] == R.neg(c, (c.gx, c.gy))
    for mont in (False, True):
        got, flags = emul_mul(E, c, cw, 257, fb.scalar_rows(c, s, mont), mont)
        assert got == want, mont
        assert flags == ident_bit


@pytest.mark.parametrize("c", fb.CURVES, ids=CURVE_IDS)
def test_emulated_block_edges_and_identity_blocks(E, c):
    """n = 1, 2, 255, 256, 257 at c = 8; a block whose lanes 0, 1 and 255 are the identity; a block that is all identity, alone and beside
    a block that is not"""
    cw = 8
    _w, _m, err_bit, ident_bit = geometry(E, c, cw)
    rng = random.Random(77 + c.cid)
    base = [rng.randrange(1, c.r) for _ in range(257)]
    for n in (1, 2, 255, 256, 257):
        got, flags = emul_mul(E, c, cw, n, fb.scalar_rows(c, base[:n]))
        assert got == fb.expect_points(c, base[:n]) and flags == 0, n
    s = list(base[:256])
    s[0] = s[1] = s[255] = 0
    got, flags = emul_mul(E, c, cw, 256, fb.scalar_rows(c, s))
    assert got == fb.expect_points(c, s) and got[0] is R.INF and got[2] is not R.INF and flags == ident_bit
    for n in (1, 256):
        got, flags = emul_mul(E, c, cw, n, fb.scalar_rows(c, [0] * n))
        assert got == [R.INF] * n and flags == ident_bit
    s = [0] * 256 + [base[0]] + [0] * 30 + [base[1]]
    got, flags = emul_mul(E, c, cw, len(s), fb.scalar_rows(c, s))
    assert got == fb.expect_points(c, s) and flags == ident_bit


@pytest.mark.parametrize("c", fb.CURVES, ids=CURVE_IDS)
def test_emulated_tau_mode(E, c):
    """lane i multiplies the squarings the bits of begin + i select: tau = 0, 1, r - 1, 2 (past the point where 2^i wraps mod r) and random,
    canonical and Montgomery, from begin = 0 and from a shard's begin, at two widths"""
    G = (c.gx, c.gy)
    _w, _m, err_bit, ident_bit = geometry(E, c, 8)
    got, flags = emul_mul(E, c, 8, 5, tau=0)
    assert got == [G] + [R.INF] * 4 and flags == ident_bit
    assert emul_mul(E, c, 8, 5, tau=1) == ([G] * 5, 0)
    assert emul_mul(E, c, 8, 6, tau=c.r - 1, mont=True) == ([G, R.neg(c, G)] * 3, 0)
    got, flags = emul_mul(E, c, 13, 260, tau=2, begin=40)      # 2^(40 + i): one set bit through every position, reduced mod r from 2^254 / 2^255 on
    assert got == fb.expect_points(c, fb.tau_powers(c, 2, 260, 40)) and flags == 0
    tau = random.Random(5 + c.cid).randrange(2, c.r)
    for cw, n, begin, mont in ((8, 257, 0, False), (4, 40, 233, True), (13, 3, (1 << 31) - 4, False)):
        got, flags = emul_mul(E, c, cw, n, tau=tau, begin=begin, mont=mont)
        assert got == fb.expect_points(c, fb.tau_powers(c, tau, n, begin)) and flags == 0, (cw, n, begin, mont)


def test_emulated_scalar_not_below_r_raises_the_flag_and_reads_as_zero(E):
    for c in fb.CURVES:
        _w, _m, err_bit, ident_bit = geometry(E, c, 8)
        for bad in (c.r, (1 << 256) - 1):
            s = fb.scalar_rows(c, [3, 4, 5, 6, 7])
            s[3] = np.frombuffer(int(bad).to_bytes(32, "little"), np.uint8)
            for mont in (False, True):
                got, flags = emul_mul(E, c, 8, 5, s, mont)
                assert flags == err_bit | ident_bit and got[3] is R.INF, (c.name, hex(bad), mont)


def test_emulated_multiples_of_a_callers_base(E):
    c = R.GRUMPKIN
    B = R.mul(c, 7, (c.gx, c.gy))
    s = fb.scalar_set(c, 4, 40)
    got, _flags = emul_mul(E, c, 4, 40, fb.scalar_rows(c, s), B=B)
    assert got == fb.expect_points(c, s, B)


# ---- the C++ wrappers --------------------------------------------------------------------------------------------------------------------
def test_cpp_wrappers_compile_and_refuse_with_the_librarys_codes(L):
    """tests/cpp/fixed_base_mirror_test.cpp: nova::provider::CommitmentKey::from_scalars / setup_from_tau built with g++ against the product
    library; everything it checks is decided before a device is leased, so it runs the same with and without a GPU"""
    src = os.path.join(ROOT, "tests", "cpp", "fixed_base_mirror_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "fixed_base_mirror_test.bin")
    deps = [src, os.path.join(ROOT, "include", "nova_mi355x.hpp"), os.path.join(ROOT, "include", "nova_mi355x.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, src, "-L" + os.path.join(ROOT, "nova_amd"), "-lnova_mi355x",
                               "-Wl,-rpath," + os.path.join(ROOT, "nova_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "fixed base mirror ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
