"""nmx_pow_split_evals / nmx_neutron_fold_sums / nmx_neutron_relation_sum / nmx_neutron_fold_witness without a GPU.  (0) The yardstick
first: tests/neutron_common.py against identities that do not go through it twice.  (1) The four entry points are declared with the
header's parameter lists, exported, bound in Python / C++ / Rust, and the header names the reference's line ranges and every error code.
(2) Every argument error returns its code with no device present and leaves the caller's buffers byte-identical; a well-formed call is
stopped by NMX_E_NO_DEVICE and nothing else.  (3) The lane bodies of the kernels (nova_amd/csrc/neutron.hpp) run thread by thread with the
kernels' own thread -> (tile, lane) map and limb bounds asserted (NMX_DEBUG_BOUNDS), against tests/neutron_common.py, on all four fields,
canonical and Montgomery words.  What the emulation does NOT run: the block sum (shuffles) and the one-block finish of the two sums (the
threads' totals are added up here), the launches, the staging and the host half of the calls; tests/test_gpu_neutron.py covers those."""
import ctypes
import inspect
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests import fv_common as fc
from tests import neutron_common as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nova_amd", "csrc")
PARAMS = {
    "nmx_pow_split_evals": ["int field_id", "const void* tau", "size_t left", "size_t right", "uint32_t flags", "void* out"],
    "nmx_neutron_fold_sums": ["int field_id", "size_t left", "size_t right", "const void* E1", "const void* Az1", "const void* Bz1", "const void* Cz1",
                              "const void* E2", "const void* Az2", "const void* Bz2", "const void* Cz2", "const void* rho", "uint32_t flags",
                              "uint8_t* out160"],
    "nmx_neutron_relation_sum": ["int field_id", "size_t left", "size_t right", "const void* E", "const void* Az", "const void* Bz", "const void* Cz",
                                 "uint32_t flags", "uint8_t* out32"],
    "nmx_neutron_fold_witness": ["int field_id", "const void* w1", "const void* w2", "size_t n_w", "const void* e1", "const void* e2", "size_t n_e",
                                 "const void* r_b", "uint32_t flags", "void* w", "void* e"],
}


@pytest.fixture(scope="module")
def L():
    from nova_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- (0) the yardstick ------------------------------------------------------------------------------------------------------------------
def test_yardstick_identities():
    p, rng = fc.FIELDS[1], random.Random(5)
    # from_evals interpolates: the polynomial goes through its evaluations, and a known polynomial comes back
    co = [rng.randrange(p) for _ in range(6)]
    assert nc.from_evals(p, [nc.poly_eval(p, co, x) for x in range(6)]) == co
    ev = [rng.randrange(p) for _ in range(6)]
    assert [nc.poly_eval(p, nc.from_evals(p, ev), x) for x in range(6)] == ev
    # split_evals: e[j] f[i] = tau^(i left + j), the power polynomial's table over k = i left + j; and the reference's [1, t] layers at left = 2
    tau, left, right = rng.randrange(p), 3, 5
    E = nc.pow_split_evals(p, tau, left, right)
    assert [E[left + i] * E[j] % p for i in range(right) for j in range(left)] == [pow(tau, k, p) for k in range(left * right)]
    assert nc.pow_split_evals(p, tau, 2, 1) == [1, tau, 1] and nc.pow_split_evals(p, 0, 2, 2) == [1, 0, 1, 0]
    # the five fold sums are the zero-fold's round polynomial: degree 5 in t (e f (A B - C) has degree 4, c_t degree 1), so the value at
    # t = 1 follows from the other five, and it is rho times the relation sum of instance 2
    c = nc.random_case(1, 3, 5, seed=9)
    s = c.want_fold(False)
    rel2 = c.want_relation(False, which=2)
    one = c.rho * rel2 % p
    co = nc.from_evals(p, [s[0], one, s[1], s[2], s[3], s[4]])
    v = [nc.values(p, w, False) for w in c.vecs]
    for t in (6, 7, p - 1):
        want = ((1 - c.rho) + t * (2 * c.rho - 1)) * nc.relation_sum(p, 3, 5, *[nc.at(p, a, b, t) for a, b in zip(v[:4], v[4:])]) % p
        assert nc.poly_eval(p, co, t) == want
    assert s[0] == (1 - c.rho) * c.want_relation(False) % p
    # the fold is the line through the two witnesses
    assert nc.fold_witness(p, [5], [9], [p - 1], [0], 0) == ([5], [p - 1]) and nc.fold_witness(p, [5], [9], [p - 1], [0], 1) == ([9], [0])
    # layouts
    assert nc.values(p, nc.words(p, [1, p - 1, 7], True), True) == [1, p - 1, 7] and nc.values(p, [p, p + 1], False) == [0, 1]


# ---- (1) the surface ----------------------------------------------------------------------------------------------------------------
def test_header_declares_library_exports_and_python_binds_the_same_types(L):
    hdr = open(os.path.join(ROOT, "include", "nova_mi355x.h")).read()
    ctype_of = lambda d: (ctypes.c_int if d.startswith("int ") else ctypes.c_size_t if d.startswith("size_t") else ctypes.c_uint32  # noqa: E731
                          if d.startswith("uint32_t") else ctypes.c_void_p)
    for name, want in PARAMS.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert m, "the header does not declare " + name
        plist = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert [x.strip() for x in re.sub(r"\s+", " ", plist).split(",")] == want
        assert hasattr(L, name)
        assert list(getattr(L, name).argtypes) == [ctype_of(d) for d in want]
    sect = hdr.split("NeutronNova's folding step")[1].split("int nmx_eq_evals_from_points(")[0]
    for needle in ("nifs.rs:200-289", "power.rs:62-86", "nifs.rs:29-186", "relation.rs:83-97", "relation.rs:131-156", "out of bounds", "NMX_E_ARG", "NMX_E_TOO_LARGE",
                   "NMX_E_SCALAR_RANGE", "NMX_ASYNC", "NMX_SCALARS_MONT", "NMX_SCALARS_DEVICE", "always host pointers", "nothing is written", "OPERAND WORDS",
                   "canonical", "neutron_max_blocks", "0, 2, 3, 4, 5", "9 rho - 4", "in-place", "logical device 0", "thread-safe"):
        assert needle in sect, needle
    assert '"neutron_max_blocks"' in hdr.split("int nmx_set_option(")[0].rsplit("/*", 1)[1]
    ffi = open(os.path.join(ROOT, "bindings", "rust", "nova-mi355x-sys", "src", "ffi.rs")).read()
    for name in PARAMS:
        assert "pub fn %s(" % name in ffi, "ffi.rs: regenerate with scripts/gen_rust_sys.py"


def test_python_and_cpp_wrappers_exist():
    from nova_amd import fieldvec as fv
    assert list(inspect.signature(fv.pow_split_evals).parameters) == ["field", "tau", "left", "right", "mont", "device", "async_"]
    assert list(inspect.signature(fv.neutron_fold_sums).parameters) == ["field", "left", "right", "E1", "Az1", "Bz1", "Cz1", "E2", "Az2", "Bz2", "Cz2", "rho", "mont"]
    assert list(inspect.signature(fv.neutron_relation_sum).parameters) == ["field", "left", "right", "E", "Az", "Bz", "Cz", "mont"]
    assert list(inspect.signature(fv.neutron_fold_witness).parameters) == ["field", "w1", "w2", "e1", "e2", "r_b", "mont", "async_", "inplace"]
    res = open(os.path.join(ROOT, "include", "nova_mi355x.hpp")).read().split("namespace resident {")[1]
    for decl in ("inline void pow_split_evals(int field", "inline std::array<Scalar, 5> neutron_fold_sums(int field", "inline Scalar neutron_relation_sum(int field",
                 "inline void neutron_fold_witness(int field"):
        assert decl in res, decl
    assert '#include "neutron.hpp"' in open(os.path.join(CSRC, "sumcheck.hip")).read()


def test_the_option_is_known(L):
    from nova_amd import _lib
    ok = 0 if L.nmx_device_count() > 0 else _lib.E_NO_DEVICE
    assert L.nmx_set_option(b"neutron_max_blocks", 1) == ok and L.nmx_set_option(b"neutron_max_blocks", 0) == ok
    assert L.nmx_set_option(b"neutron_min_blocks", 1) != 0


# ---- (2) argument errors --------------------------------------------------------------------------------------------------------------
BAD_FLAGS = lambda lib: (lib.BASES_MONT, lib.BASES_DEVICE, lib.OUT_PARTIAL, 1 << 20)  # noqa: E731


def test_argument_errors_need_no_device_and_write_nothing(L):
    from nova_amd import _lib
    fid, left, right = 1, 3, 2
    p = fc.FIELDS[fid]
    n = left * right
    buf = np.ascontiguousarray(fc.rand_vec(fid, 128, 3).copy())    # vector j of the calls at element 8 j; outputs from element 96
    before = buf.copy()
    at = lambda i: buf.ctypes.data + 32 * i  # noqa: E731
    A, TL, SR = _lib.E_ARG, _lib.E_TOO_LARGE, _lib.E_SCALAR_RANGE
    ok = 0 if L.nmx_device_count() > 0 else _lib.E_NO_DEVICE
    ch = lambda x: fc.vec([x]).copy()  # noqa: E731

    # -- nmx_pow_split_evals
    def pw(field=fid, tau=5, l_=left, r_=right, flags=0, out=at(96), null=False):
        t = ch(tau)
        return L.nmx_pow_split_evals(field, None if null else t.ctypes.data, l_, r_, flags, out)
    assert pw(null=True) == A and pw(out=None) == A
    assert pw(l_=0) == A and pw(r_=0) == A and pw(l_=1 << 31) == A and pw(l_=1 << 30, r_=1 << 30) == A and pw(l_=(1 << 63) + 1, r_=(1 << 63) + 1) == A
    assert pw(field=4) == A and pw(field=-1) == A
    assert b"bad field id" in L.nmx_last_error()
    for fl in BAD_FLAGS(_lib):
        assert pw(flags=fl) == A, fl
    assert pw(tau=p) == SR and pw(tau=p + 1) == SR and pw(tau=(1 << 256) - 1) == SR and pw(tau=p, flags=_lib.SCALARS_MONT) == SR

    # -- nmx_neutron_fold_sums
    def fs(field=fid, l_=left, r_=right, rho=7, flags=0, out=at(96), null=None):
        v = [None if null == j else at(8 * j) for j in range(8)]
        r = ch(rho)
        return L.nmx_neutron_fold_sums(field, l_, r_, *v, None if null == "rho" else r.ctypes.data, flags, out)
    for j in list(range(8)) + ["rho"]:
        assert fs(null=j) == A, j
    assert fs(out=None) == A
    assert fs(l_=0) == A and fs(r_=0) == A
    assert fs(l_=1 << 31, r_=1) == TL and fs(l_=1 << 16, r_=1 << 15) == TL and fs(l_=(1 << 63) + 1, r_=2) == TL and fs(l_=1 << 32, r_=1 << 32) == TL
    assert fs(field=4) == A and fs(field=-1) == A
    for fl in BAD_FLAGS(_lib) + (_lib.ASYNC, _lib.ASYNC | _lib.SCALARS_DEVICE):
        assert fs(flags=fl) == A, fl
    assert fs(rho=p) == SR and fs(rho=(1 << 256) - 1) == SR and fs(rho=p + 1, flags=_lib.SCALARS_MONT) == SR

    # -- nmx_neutron_relation_sum
    def rs(field=fid, l_=left, r_=right, flags=0, out=at(96), null=None):
        v = [None if null == j else at(8 * j) for j in range(4)]
        return L.nmx_neutron_relation_sum(field, l_, r_, *v, flags, out)
    for j in range(4):
        assert rs(null=j) == A, j
    assert rs(out=None) == A and rs(l_=0) == A and rs(r_=0) == A and rs(field=4) == A
    assert rs(l_=1 << 31, r_=1) == TL and rs(l_=1 << 16, r_=1 << 15) == TL
    for fl in BAD_FLAGS(_lib) + (_lib.ASYNC, _lib.ASYNC | _lib.SCALARS_DEVICE):
        assert rs(flags=fl) == A, fl

    # -- nmx_neutron_fold_witness: w1 = [0, 6), w2 = [8, 14), e1 = [16, 21), e2 = [24, 29); w = [96, 102), e = [104, 109)
    def fw(field=fid, w1=at(0), w2=at(8), n_w=6, e1=at(16), e2=at(24), n_e=5, r_b=9, flags=0, w=at(96), e=at(104), null=False):
        r = ch(r_b)
        return L.nmx_neutron_fold_witness(field, w1, w2, n_w, e1, e2, n_e, None if null else r.ctypes.data, flags, w, e)
    assert fw(w1=None) == A and fw(w2=None) == A and fw(e1=None) == A and fw(e2=None) == A and fw(w=None) == A and fw(e=None) == A and fw(null=True) == A
    assert fw(field=4) == A and fw(field=-1) == A
    for fl in BAD_FLAGS(_lib):
        assert fw(flags=fl) == A, fl
    assert fw(n_w=1 << 31) == TL and fw(n_w=1 << 30, n_e=1 << 30) == TL and fw(n_e=(1 << 63) + 1) == TL
    assert fw(r_b=p) == SR and fw(r_b=(1 << 256) - 1) == SR and fw(n_w=0, n_e=0, r_b=p) == SR
    # overlaps other than element-wise in place: shifted by one element, an output over the other family, the two outputs
    assert fw(w=at(1)) == A and fw(w=at(13)) == A and fw(e=at(20)) == A and fw(e=at(23)) == A
    assert b"overlap" in L.nmx_last_error()
    assert fw(w=at(16)) == A and fw(e=at(0)) == A and fw(e=at(101)) == A and fw(w=at(108)) == A
    assert (buf == before).all(), "a refused call wrote something"

    # -- both lengths zero is NMX_OK with no launch; a well-formed call gets past every check: what stops it is NMX_E_NO_DEVICE, nothing else
    assert fw(n_w=0, n_e=0) == 0 and fw(n_w=0, n_e=0, w1=None, w2=None, e1=None, e2=None, w=None, e=None) == 0
    calls = [pw, lambda: pw(flags=_lib.SCALARS_MONT), lambda: pw(l_=1, r_=1), fs, lambda: fs(flags=_lib.SCALARS_MONT), lambda: fs(l_=1, r_=1), rs,
             lambda: rs(flags=_lib.SCALARS_MONT), fw, lambda: fw(flags=_lib.SCALARS_MONT), lambda: fw(n_w=0, w1=None, w2=None, w=None),
             lambda: fw(n_e=0, e1=None, e2=None, e=None), lambda: fw(w=at(0), e=at(16)), lambda: fw(w=at(8), e=at(24))]
    if ok:                                                          # no device: every one of them is stopped there, with nothing written
        for f in calls:
            assert f() == ok
        assert (buf == before).all()
    else:                                                           # with a device they run (on copies of the buffer's state)
        for f in calls:
            assert f() == 0, L.nmx_last_error()


# ---- (3) the kernels' lane bodies under the emulation --------------------------------------------------------------------------------
EMUL_SRC = os.path.join(ROOT, "tests", "host_emul", "neutron_emul.cpp")
EMUL_SO = os.path.join(ROOT, "tests", "host_emul", "libnmx_neutron_emul.so")
RI = 1 << 261          # the internal residue form: x * 2^261 mod p (nova_amd/csrc/fp.hpp)
R256 = nc.R256         # the Montgomery form of NMX_SCALARS_MONT
SLACK = 0xdeadbeef


@pytest.fixture(scope="module")
def E():
    deps = [EMUL_SRC, os.path.join(ROOT, "tests", "host_emul", "simt.hpp")] + [os.path.join(CSRC, f) for f in ("fp.hpp", "neutron.hpp", "spmv_row.hpp",
                                                                                                            "msm_partition.hpp")]
    if not os.path.exists(EMUL_SO) or os.path.getmtime(EMUL_SO) < max(os.path.getmtime(x) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", EMUL_SO, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_SO)
    vp, u32, u64, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    lib.emul_neutron_sums.argtypes = [i, i, vp, vp, u32, u32, u32, vp]
    lib.emul_neutron_blocks.argtypes = [u64, u64, u32]
    lib.emul_neutron_blocks.restype = u32
    lib.emul_neutron_fold.argtypes = [i, vp, vp, u32, vp, vp, u32, vp, vp, vp]
    lib.emul_neutron_pow.argtypes = [i, vp, vp, vp, u32, u32, vp]
    return lib


def words(vals):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in vals) or bytes(32), np.uint32).copy()


def emul_sums(E, case, mont, points, opt=0, which=1):
    """the threads' totals added up and brought back from the kernel's scale (x Fm^4 / R'^3) -> `points` values"""
    p, left, right = case.p, case.left, case.right
    fm = R256 % p if mont else 1
    vecs = case.vecs[4:] + case.vecs[4:] if which == 2 else case.vecs
    arrs = [words(v) for v in vecs]
    tab = (ctypes.c_void_p * 8)(*[a.ctypes.data for a in arrs])
    blocks = E.emul_neutron_blocks(left, right, opt)
    tiles = right * -(-left // 256)
    assert blocks == min(-(-tiles // 4), opt if 0 < opt < 2048 else 2048)
    tot = np.full(8 * blocks * 256 * points + 8, SLACK, np.uint32)
    assert E.emul_neutron_sums(case.fid, points, tab, words([(p - fm) % p]).ctypes.data, left, right, blocks, tot.ctypes.data) == 0
    assert (tot[-8:] == SLACK).all(), "a store past the end of the totals"
    t = fc.ints(tot[:-8].view(np.uint8))
    assert all(x < p for x in t), "a thread's total is not the canonical representative"
    back = pow(RI, 3, p) * pow(fm, -4, p) % p
    return [sum(t[s::points]) * back % p for s in range(points)]


def bare_fold(case, mont):
    """the five sums without c_t(rho)"""
    p = case.p
    v = [nc.values(p, w, mont) for w in case.vecs]
    return [nc.relation_sum(p, case.left, case.right, *[nc.at(p, a, b, t) for a, b in zip(v[:4], v[4:])]) for t in nc.POINTS]


def check_sums(E, case, mont, opt=0):
    assert emul_sums(E, case, mont, 5, opt) == bare_fold(case, mont), (case.name, case.fid, mont, case.left, case.right, opt)
    assert emul_sums(E, case, mont, 1, opt) == [case.want_relation(mont)], (case.name, case.fid, mont, case.left, case.right, opt)


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
@pytest.mark.parametrize("mont", [False, True])
def test_emulated_sums(E, fid, mont):
    """every shape of the issue; the forced grids at (8, 4) and (65, 7): one block (a wave loops over tiles) and two"""
    for left, right in nc.SMALL_SHAPES + nc.LARGE_SHAPES:
        check_sums(E, nc.random_case(fid, left, right), mont)
    for left, right in ((8, 4), (65, 7)):
        for opt in (1, 2):
            check_sums(E, nc.random_case(fid, left, right), mont, opt)


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
def test_emulated_sums_edge_contents(E, fid):
    for left, right in ((3, 5), (65, 7)):
        for case in nc.edge_cases(fid, left, right):
            check_sums(E, case, False)
            check_sums(E, case, True)


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
def test_emulated_sums_bounds_at_their_worst(E, fid):
    """every word p - 1 (the largest canonical operands: the largest differences and walked points) and every word 2^256 - 1 (the largest
    words), at the longest accumulations a lane can see: a full tile (four columns per lane) and, with the grid forced to one block, 75 tiles
    per wave -- the lazy sums return below p after every sixth term, so nothing grows with the length and the bound asserts must hold"""
    p = fc.FIELDS[fid]
    for left, right, opt in ((1024, 3, 0), (1024, 3, 1), (4, 300, 1), (300, 4, 1)):
        sz = nc.sizes(left, right)
        for w, rho in ((p - 1, p - 1), (nc.R256 - 1, 1)):
            case = nc.Case("worst", fid, left, right, [[w] * m for m in sz], rho)
            check_sums(E, case, False, opt)
            check_sums(E, case, True, opt)
        # instance 2 at p - 1 against instance 1 at 0 and the reverse: the differences at their extremes, the walk at its longest
        for w1, w2 in ((0, p - 1), (p - 1, 0), (1, 0)):
            case = nc.Case("worst", fid, left, right, [[w1] * m for m in sz[:4]] + [[w2] * m for m in sz[4:]], 3)
            check_sums(E, case, fid % 2 == 1, opt)


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
@pytest.mark.parametrize("mont", [False, True])
def test_emulated_fold_witness(E, fid, mont):
    p, rng = fc.FIELDS[fid], random.Random(3 * fid + mont)
    for n_w, n_e in ((0, 1), (1, 0), (63, 65), (64, 64), (65, 63), (1000, 1)):
        for r_b in (0, 1, p - 1, rng.randrange(p)):
            vs = [[rng.choice([0, p - 1, p, p + 1, R256 - 1]) if rng.random() < 0.2 else rng.randrange(p) for _ in range(m)] for m in (n_w, n_w, n_e, n_e)]
            arrs = [words(v) for v in vs]
            w, e = np.full(8 * n_w + 8, SLACK, np.uint32), np.full(8 * n_e + 8, SLACK, np.uint32)
            r = words([r_b * RI % p])
            assert E.emul_neutron_fold(fid, *[a.ctypes.data for a in arrs[:2]], n_w, *[a.ctypes.data for a in arrs[2:]], n_e, r.ctypes.data,
                                       w.ctypes.data, e.ctypes.data) == 0
            assert (w[8 * n_w:] == SLACK).all() and (e[8 * n_e:] == SLACK).all(), "a store past the end of an output"
            vals = [nc.values(p, v, mont) for v in vs]
            want = nc.fold_witness(p, *vals, r_b)
            assert (fc.ints(w[:8 * n_w].view(np.uint8)) if n_w else []) == nc.words(p, want[0], mont), (n_w, n_e, r_b)
            assert (fc.ints(e[:8 * n_e].view(np.uint8)) if n_e else []) == nc.words(p, want[1], mont), (n_w, n_e, r_b)
            # in place: the outputs over the first inputs
            if n_w and n_e:
                assert E.emul_neutron_fold(fid, arrs[0].ctypes.data, arrs[1].ctypes.data, n_w, arrs[2].ctypes.data, arrs[3].ctypes.data, n_e, r.ctypes.data,
                                           arrs[0].ctypes.data, arrs[2].ctypes.data) == 0
                assert fc.ints(arrs[0].view(np.uint8)) == nc.words(p, want[0], mont) and fc.ints(arrs[2].view(np.uint8)) == nc.words(p, want[1], mont)


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
@pytest.mark.parametrize("mont", [False, True])
def test_emulated_pow_split_evals(E, fid, mont):
    p, rng = fc.FIELDS[fid], random.Random(7 * fid + mont)
    for left, right in ((1, 1), (2, 1), (1, 2), (3, 5), (65, 7), (1024, 1024), (2048, 1024)):
        for tau in (0, 1, p - 1, rng.randrange(p)):
            if left + right > 2048 and tau in (0, 1):
                continue
            tl = pow(tau, left, p)
            sq_e = words([pow(tau, 1 << b, p) * RI % p for b in range(31)])
            sq_f = words([pow(tl, 1 << b, p) * RI % p for b in range(31)])
            n = left + right
            out = np.full(8 * n + 8, SLACK, np.uint32)
            assert E.emul_neutron_pow(fid, sq_e.ctypes.data, sq_f.ctypes.data, words([R256 % p if mont else 1]).ctypes.data, left, n, out.ctypes.data) == 0
            assert (out[8 * n:] == SLACK).all(), "a store past the end of out"
            assert fc.ints(out[:8 * n].view(np.uint8)) == nc.words(p, nc.pow_split_evals(p, tau, left, right), mont), (left, right, tau)
