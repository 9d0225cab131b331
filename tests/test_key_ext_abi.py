"""nmx_bases_concat / nmx_bases_fold / nmx_bases_scale without a GPU.  (1) The entry points are declared with the issue's parameter lists behind
nmx_bases_derive_by_address and before nmx_msm, exported, bound in Python / C++ / Rust (the C++ wrappers also compiled and run,
tests/cpp/key_ext_mirror_test.cpp), and the header block names the reference's line ranges, every error code and the flags.  (2) Every refusal
that needs no device returns its code with no device present and leaves *handle untouched.  (3) The host recoding (ke_recode of
nova_amd/csrc/key_ext.hpp, plain C++) gives back the weights it was given, never longer than BITS + 1 positions, on both scalar widths.
(4) k_key_lincomb runs under tests/host_emul with limb bounds asserted, bit-exact against pyref on all four curves: 1, 255, 256 and 257
outputs, the digit-edge weights and pairs, equal and opposite rows, identity rows on either side and on both, one weight at 0 and r - 1.
What the emulation does NOT run: the launch, build_key, the key's window tables, the concat copies; tests/test_gpu_key_ext.py covers those."""
import ctypes
import inspect
import os
import random
import re
import subprocess

import numpy as np
import pytest

from oracle import pyref as R
from tests import derive_key_common as dk
from tests import fixed_base_common as fb
from tests import key_ext_common as kx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nova_amd", "csrc")
CURVE_IDS = [c.name for c in kx.CURVES]
PARAMS = {
    "nmx_bases_concat": ["const uint64_t* ck_handles", "const size_t* offsets", "const size_t* lens", "size_t k", "uint32_t flags", "uint64_t* handle"],
    "nmx_bases_fold": ["uint64_t ck_handle", "size_t offset", "size_t n", "const void* w1", "const void* w2", "uint32_t flags", "uint64_t* handle"],
    "nmx_bases_scale": ["uint64_t ck_handle", "size_t offset", "size_t n", "const void* r", "uint32_t flags", "uint64_t* handle"],
}


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
    u64p, szp = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_size_t)
    ctype_of = {"const uint64_t* ck_handles": u64p, "const size_t* offsets": szp, "const size_t* lens": szp, "size_t k": ctypes.c_size_t,
                "uint64_t ck_handle": ctypes.c_uint64, "size_t offset": ctypes.c_size_t, "size_t n": ctypes.c_size_t, "const void* w1": ctypes.c_void_p,
                "const void* w2": ctypes.c_void_p, "const void* r": ctypes.c_void_p, "uint32_t flags": ctypes.c_uint32, "uint64_t* handle": u64p}
    ffi = open(os.path.join(ROOT, "bindings", "rust", "nova-mi355x-sys", "src", "ffi.rs")).read()
    for name, params in PARAMS.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert m, "the header does not declare " + name
        assert [x.strip() for x in re.sub(r"\s+", " ", m.group(1)).split(",")] == params
        assert hasattr(L, name)
        assert list(getattr(L, name).argtypes) == [ctype_of[d] for d in params], name
        assert "pub fn %s(" % name in ffi, "ffi.rs: regenerate with scripts/gen_rust_sys.py"
    assert hdr.index("int nmx_bases_derive_by_address(") < hdr.index("/* ---- key algebra") < hdr.index("int nmx_bases_concat(") < hdr.index(
        "int nmx_bases_fold(") < hdr.index("int nmx_bases_scale(") < hdr.index("int nmx_msm(")
    doc = hdr.split("int nmx_bases_concat(")[0].rsplit("/* ---- key algebra", 1)[1]
    for needle in ("pedersen.rs:430-529", "ipa_pc.rs:183,194,212-227,255,", "294,310,353-363,380", "pedersen.rs:484-497", "pedersen.rs:500-512",
                   "msm.rs:247-249", "CommitmentKeyExtTrait", "split_at", "combine", "reinterpret_commitments_as_ck", "nmx_bases_register",
                   "conservative", "NMX_E_ARG", "NMX_E_SCALAR_RANGE", "NMX_E_HANDLE", "NMX_E_HIP", "NMX_SCALARS_MONT", "NMX_BASES_PRECOMPUTE", "NMX_ASYNC",
                   "*handle untouched", ">= 2^31", "k > 8", "n < 2", "sharded", "different curves", "different devices", "last point is ignored",
                   "joint sparse form", "offsets == NULL", "lens == NULL"):
        assert needle in doc, needle


def test_python_and_cpp_wrappers_exist():
    from nova_amd import provider as P
    K = P.CommitmentKey
    assert list(inspect.signature(K.split_at).parameters) == ["self", "n"]
    assert list(inspect.signature(K.combine).parameters) == ["self", "other"]
    assert list(inspect.signature(K.concat).parameters)[:2] == ["self", "parts"]
    sig = inspect.signature(K.fold)
    assert list(sig.parameters) == ["self", "w1", "w2", "mont", "precompute"]
    assert sig.parameters["mont"].default is False and sig.parameters["precompute"].default is False
    sig = inspect.signature(K.scale)
    assert list(sig.parameters) == ["self", "r", "mont", "precompute"]
    assert sig.parameters["mont"].default is False and sig.parameters["precompute"].default is False
    hpp = open(os.path.join(ROOT, "include", "nova_mi355x.hpp")).read()
    key = hpp.split("class CommitmentKey {")[1].split("template <int CURVE> struct DlogGroupExt")[0]
    at = [key.index(s) for s in ("CommitmentKey derive_by_address(", "CommitmentKey concat(const std::vector<Part>& parts, bool precompute = false) const",
                                 "std::pair<CommitmentKey, CommitmentKey> split_at(size_t n) const", "CommitmentKey combine(const CommitmentKey& other) const",
                                 "CommitmentKey fold(const Scalar& w1, const Scalar& w2, bool mont = false, bool precompute = false) const",
                                 "CommitmentKey scale(const Scalar& r, bool mont = false, bool precompute = false) const")]
    assert at == sorted(at)
    assert '#include "key_ext.hpp"' in open(os.path.join(CSRC, "runtime.hpp")).read()
    assert "&derive, &key_lincomb," in open(os.path.join(CSRC, "curve_impl.hpp")).read()


def test_cpp_wrappers_compile_and_run(L):
    """tests/cpp/key_ext_mirror_test.cpp built with g++ against the product library: the wrappers' types, the refusals decided before a
    device is leased and, where a device is present, results whose expected points are points of the source key"""
    src = os.path.join(ROOT, "tests", "cpp", "key_ext_mirror_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "key_ext_mirror_test.bin")
    deps = [src, os.path.join(ROOT, "include", "nova_mi355x.hpp"), os.path.join(ROOT, "include", "nova_mi355x.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, src, "-L" + os.path.join(ROOT, "nova_amd"), "-lnova_mi355x",
                               "-Wl,-rpath," + os.path.join(ROOT, "nova_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "key ext mirror ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


# ---- (2) refusals -----------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5EEDFACE0BADF00D
NO_KEY = 0x7fffffff12345  # never a registered handle: what the checks below decide, they decide before the key is looked up
ONE = (1).to_bytes(32, "little")


def _concat(L, handles=(NO_KEY, NO_KEY + 1), offsets=None, lens=(2, 1), k=None, flags=0, handle="ok"):
    k = (len(handles) if handles is not None else 2) if k is None else k
    hs = None if handles is None else (ctypes.c_uint64 * max(len(handles), 1))(*handles)
    offs = None if offsets is None else (ctypes.c_size_t * len(offsets))(*offsets)
    ln = None if lens is None else (ctypes.c_size_t * len(lens))(*lens)
    h = ctypes.c_uint64(SENTINEL)
    rc = L.nmx_bases_concat(hs, offs, ln, k, flags, None if handle is None else ctypes.byref(h))
    assert h.value == SENTINEL, "a refused call wrote *handle"
    return rc


def _fold(L, n=4, w1=ONE, w2=ONE, flags=0, handle="ok", offset=0):
    h = ctypes.c_uint64(SENTINEL)
    rc = L.nmx_bases_fold(NO_KEY, offset, n, w1, w2, flags, None if handle is None else ctypes.byref(h))
    assert h.value == SENTINEL, "a refused call wrote *handle"
    return rc


def _scale(L, n=4, r=ONE, flags=0, handle="ok", offset=0):
    h = ctypes.c_uint64(SENTINEL)
    rc = L.nmx_bases_scale(NO_KEY, offset, n, r, flags, None if handle is None else ctypes.byref(h))
    assert h.value == SENTINEL, "a refused call wrote *handle"
    return rc


def test_refusals_need_no_device_and_leave_the_handle_untouched(L):
    from nova_amd import _lib
    A, H = _lib.E_ARG, _lib.E_HANDLE
    not_ours = (_lib.BASES_MONT, _lib.BASES_DEVICE, _lib.SCALARS_DEVICE, _lib.OUT_PARTIAL, _lib.BASES_VALIDATE, _lib.ASYNC, 1 << 20, 1 << 31)
    # concat
    assert _concat(L, handle=None) == A and _concat(L, handles=None) == A
    assert _concat(L, k=0) == A and _concat(L, handles=(NO_KEY,) * 9, lens=(1,) * 9) == A
    assert _concat(L, lens=(0, 0)) == A
    assert _concat(L, lens=(1 << 31, 1)) == A and _concat(L, lens=(1 << 30, 1 << 30)) == A and _concat(L, lens=((1 << 64) - 1, 2)) == A
    for fl in not_ours + (_lib.SCALARS_MONT,):
        assert _concat(L, flags=fl) == A, fl
    assert _concat(L) == H and _concat(L, flags=_lib.BASES_PRECOMPUTE, offsets=(3, 4)) == H and _concat(L, lens=None) == H
    assert _concat(L, handles=(NO_KEY,) * 8, lens=(1,) * 8) == H
    # fold
    assert _fold(L, handle=None) == A and _fold(L, w1=None) == A and _fold(L, w2=None) == A
    assert _fold(L, n=0) == A and _fold(L, n=1) == A and _fold(L, n=1 << 31) == A and _fold(L, n=(1 << 63) + 4) == A
    for fl in not_ours:
        assert _fold(L, flags=fl) == A, fl
    assert _fold(L) == H and _fold(L, n=2) == H and _fold(L, flags=_lib.SCALARS_MONT | _lib.BASES_PRECOMPUTE) == H
    # scale
    assert _scale(L, handle=None) == A and _scale(L, r=None) == A
    assert _scale(L, n=0) == A and _scale(L, n=1 << 31) == A
    for fl in not_ours:
        assert _scale(L, flags=fl) == A, fl
    assert _scale(L) == H and _scale(L, n=1) == H and _scale(L, flags=_lib.SCALARS_MONT | _lib.BASES_PRECOMPUTE) == H
    # (a weight's range is the KEY's scalar field: with no key there is none to check against -- tests/test_gpu_key_ext.py)
    assert _scale(L, r=b"\xff" * 32) == H and _fold(L, w2=b"\xff" * 32) == H


# ---- (3) the recoding, (4) the kernel under the emulation -------------------------------------------------------------------------------------
EMUL_SRC = os.path.join(ROOT, "tests", "host_emul", "key_ext_emul.cpp")
EMUL_SO = os.path.join(ROOT, "tests", "host_emul", "libnmx_key_ext_emul.so")
SLACK = 0xdeadbeef


@pytest.fixture(scope="module")
def E():
    deps = [EMUL_SRC, os.path.join(ROOT, "tests", "host_emul", "simt.hpp")] + [os.path.join(CSRC, f) for f in (
        "fp.hpp", "curve.hpp", "curves.hpp", "key_ext.hpp", "fixed_base.hpp", "msm_pipeline.hpp", "msm_partition.hpp", "msm_seg.hpp", "msm_kernels.hpp")]
    if not os.path.exists(EMUL_SO) or os.path.getmtime(EMUL_SO) < max(os.path.getmtime(x) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", EMUL_SO, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_SO)
    vp, u32, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    lib.emul_ke_recode.argtypes = [vp, vp, vp]
    lib.emul_key_lincomb.argtypes = [i, vp, vp, u32, vp, vp, vp, vp]
    lib.emul_ke_geometry.argtypes = [vp]
    g = np.zeros(8, np.uint32)
    lib.emul_ke_geometry(g.ctypes.data)
    lib.NAMES, lib.IDENT, lib.MAXPOS, lib.THREADS = tuple(int(x) for x in g[:5]), int(g[5]), int(g[6]), int(g[7])
    return lib


def _words(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint32).copy()


def recode(E, w1, w2=None):
    """-> (codes, length) of ke_recode"""
    a, b = _words(w1), None if w2 is None else _words(w2)
    codes = np.full(E.MAXPOS + 8, 0xee, np.uint8)
    n = E.emul_ke_recode(a.ctypes.data, None if b is None else b.ctypes.data, codes.ctypes.data)
    assert (codes[E.MAXPOS:] == 0xee).all()
    return codes[:E.MAXPOS], n


@pytest.mark.parametrize("c", [R.BN254_G1, R.PALLAS], ids=["254_bits", "255_bits"])
def test_recoding_gives_the_weights_back_and_stays_within_bits_plus_one(E, c):
    assert E.MAXPOS == 256 and E.NAMES == (1, 2, 3, 4, 8)
    B = kx.bits(c)
    for w in kx.edge_weights(c):
        codes, n = recode(E, w)
        assert 0 <= n <= B + 1 and kx.decode(codes, n, E.NAMES) == (w, 0) and not codes[n:].any(), hex(w)
        assert n == 0 or codes[n - 1] != 0
        sel = codes[:n] & 7
        assert set(sel.tolist()) <= {0, E.NAMES[0]}                      # one weight: only +-P0 ...
        assert not (sel[1:] != 0)[sel[:-1] != 0].any(), hex(w)           # ... and no two adjacent: the non-adjacent form
    assert recode(E, 0)[1] == 0 and recode(E, 1)[1] == 1 and recode(E, 0, 0)[1] == 0
    dens = []
    for w1, w2 in kx.all_pairs(c) + [(random.Random(i).randrange(c.r), random.Random(-i - 1).randrange(c.r)) for i in range(40)]:
        codes, n = recode(E, w1, w2)
        assert 0 <= n <= B + 1 and kx.decode(codes, n, E.NAMES) == (w1, w2) and not codes[n:].any(), (hex(w1), hex(w2))
        if min(w1, w2) > 1 << 200:
            dens.append(np.count_nonzero(codes[:n]) / n)
    assert 0.42 < sum(dens) / len(dens) < 0.58                           # Solinas: the joint weight is 1/2 of the length on average
    # the form is canonical whichever side a weight stands on
    codes, n = recode(E, 0, 5)
    assert kx.decode(codes, n, E.NAMES) == (0, 5) and set((codes[:n] & 7).tolist()) <= {0, E.NAMES[1]}


def lincomb(E, c, sL, sR, w1, w2=None):
    """the emulated kernel over L[i] = sL[i] G (and R[i] = sR[i] G) -> (points, flag word)"""
    m = len(sL)
    p0 = dk.internal_rows(c, fb.expect_points(c, sL))
    p1 = None if w2 is None else dk.internal_rows(c, fb.expect_points(c, sR))
    a, b = _words(w1), None if w2 is None else _words(w2)
    out = np.full(16 * m + 16, SLACK, np.uint32)
    flags = np.full(3, SLACK, np.uint32)
    rc = E.emul_key_lincomb(c.cid, p0.ctypes.data, None if p1 is None else p1.ctypes.data, m, a.ctypes.data, None if b is None else b.ctypes.data,
                            out.ctypes.data, flags.ctypes.data)
    assert rc == 0
    assert (out[16 * m:] == SLACK).all() and flags[2] == SLACK, "a store past the end of the key or of the flag words"
    return dk.points_from_internal(c, out[:16 * m]), int(flags[0])


def check_fold(E, c, s, w1, w2):
    h = len(s) // 2
    want = kx.points(c, kx.fold_scalars(c, s, w1, w2))
    got, flags = lincomb(E, c, s[:h], s[h:2 * h], w1, w2)
    assert got == want, (hex(w1), hex(w2))
    assert flags == (E.IDENT if R.INF in want else 0)


def check_scale(E, c, s, r):
    want = kx.points(c, kx.scale_scalars(c, s, r))
    got, flags = lincomb(E, c, s, None, r)
    assert got == want, hex(r)
    assert flags == (E.IDENT if R.INF in want else 0)


@pytest.mark.parametrize("c", kx.CURVES, ids=CURVE_IDS)
def test_emulated_output_counts_around_the_block(E, c):
    """1, 255, 256 and 257 outputs of a fold and of a scale; from 5 outputs on the source holds an equal pair, an opposite pair and identity rows
    on either side and on both"""
    assert E.THREADS == 256
    w1, w2, r = kx.random_weight(c, 1), kx.random_weight(c, 2), kx.random_weight(c, 3)
    for m in (1, 255, 256, 257):
        check_fold(E, c, kx.source_scalars(c, 2 * m, seed=m), w1, w2)
    for m in (1, 257):
        check_scale(E, c, kx.source_scalars(c, m, seed=m), r)


@pytest.mark.parametrize("c", kx.CURVES, ids=CURVE_IDS)
def test_emulated_digit_edge_weights_and_pairs(E, c):
    """every edge weight alone (scale) and every edge pair (fold) over a 12-point key with the group-law edge rows"""
    s = kx.source_scalars(c, 12, seed=3)
    for r in kx.edge_weights(c):
        check_scale(E, c, s, r)
    for w1, w2 in kx.all_pairs(c):
        check_fold(E, c, s, w1, w2)


@pytest.mark.parametrize("c", kx.CURVES, ids=CURVE_IDS)
def test_emulated_group_law_edges(E, c):
    G = (c.gx, c.gy)
    w = kx.random_weight(c, 5)
    # P0 == P1 with w1 == w2: S is a doubling, D the identity
    got, flags = lincomb(E, c, [7], [7], w, w)
    assert got == [R.mul(c, 14 * w % c.r, G)] and flags == 0
    # P0 == P1 with w2 = r - w1: the identity
    got, flags = lincomb(E, c, [7, 9], [7, 9], w, c.r - w)
    assert got == [R.INF, R.INF] and flags == E.IDENT
    # P1 == -P0: S the identity, D a doubling
    got, flags = lincomb(E, c, [7], [c.r - 7], w, w)
    assert got == [R.INF] and flags == E.IDENT
    got, flags = lincomb(E, c, [7], [c.r - 7], w, 3)
    assert got == [R.mul(c, 7 * (w - 3) % c.r, G)] and flags == 0
    # an identity row in L, in R, in both, next to an ordinary row
    got, flags = lincomb(E, c, [0, 5, 0, 5], [6, 0, 0, 6], w, 3)
    assert got == [R.mul(c, 18, G), R.mul(c, 5 * w % c.r, G), R.INF, R.mul(c, (5 * w + 18) % c.r, G)] and flags == E.IDENT
    # one weight at 0 and at r - 1
    got, flags = lincomb(E, c, [5, 0, 9], None, 0)
    assert got == [R.INF] * 3 and flags == E.IDENT
    got, flags = lincomb(E, c, [5, 0, 9], None, c.r - 1)
    assert got == [R.mul(c, c.r - 5, G), R.INF, R.mul(c, c.r - 9, G)] and flags == E.IDENT
    got, flags = lincomb(E, c, [5, 9], None, c.r - 1)
    assert got == [R.mul(c, c.r - 5, G), R.mul(c, c.r - 9, G)] and flags == 0
