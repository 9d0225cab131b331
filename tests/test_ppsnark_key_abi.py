"""nmx_ppsnark_spark_repr / nmx_masked_eq_evals without a GPU.  (1) Both entry points are declared with the header's parameter lists,
exported, bound in Python / C++ / Rust (the C++ wrappers also compiled and run, tests/cpp/ppsnark_key_mirror_test.cpp), and the header names the reference's line ranges and every error code.  (2) Every argument error
that can be reached without a registered matrix returns its code with no device present and leaves the caller's buffers byte-identical.
(3) The kernels of nova_amd/csrc/ppsnark_key.hpp run thread by thread under tests/host_emul/simt.hpp with limb bounds asserted, against the
definition in Python integers (tests/ppsnark_key_common.py) on all four fields, canonical and Montgomery words: the expansion pass, the
block-level column histogram (LDS table, barriers, fall-back) and the finish pass, over resident arrays built HERE (indices with their
class bits, data in the internal form).  What the emulation does NOT run: the launches, the staging, the registration, concurrent atomics;
tests/test_gpu_ppsnark_key.py covers those."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fv_common as fc
from tests import ppsnark_key_common as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nova_amd", "csrc")
S_PARAMS = ["const uint64_t* handles", "size_t k", "size_t n", "uint32_t flags", "void* out_row", "void* out_col", "void* const* out_vals",
            "void* out_ts_row", "void* out_ts_col"]
M_PARAMS = ["int field_id", "const void* r", "size_t ell", "size_t num_masked_vars", "uint32_t flags", "void* out"]


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
                          if d.startswith("uint32_t") else ctypes.c_void_p)
    for name, want in (("nmx_ppsnark_spark_repr", S_PARAMS), ("nmx_masked_eq_evals", M_PARAMS)):
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert m, "the header does not declare " + name
        plist = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert [x.strip() for x in re.sub(r"\s+", " ", plist).split(",")] == want
        assert hasattr(L, name)
        assert list(getattr(L, name).argtypes) == [ctype_of(d) for d in want]
    assert hdr.index("int nmx_ppsnark_mem_oracles(") < hdr.index("int nmx_ppsnark_spark_repr(") < hdr.index("int nmx_masked_eq_evals(")
    s_doc = hdr.split("int nmx_ppsnark_spark_repr(")[0].rsplit("/* ---- ppsnark's key tables", 1)[1]
    for needle in ("ppsnark.rs:117-190", "sparse.rs:332-390", "ppsnark.rs:123-128", "ppsnark.rs:129-151", "ppsnark.rs:154-167", "ppsnark.rs:170-174",
                   "ppsnark.rs:118-121", "NMX_E_ARG", "NMX_E_TOO_LARGE", "NMX_E_HANDLE", "NMX_SCALARS_MONT", "NMX_SCALARS_DEVICE", "NMX_ASYNC",
                   "NMX_PPS_TS_ROW", "NMX_PPS_TS_COL", "NMX_PPS_L_ROW", "NMX_PPS_L_COL", "NMX_PPS_VAL", "nothing written", "power of two", "NULL"):
        assert needle in s_doc, needle
    m_doc = hdr.split("int nmx_masked_eq_evals(")[0].rsplit("/* nmx_masked_eq_evals ==", 1)[1]
    for needle in ("masked_eq.rs:57-75", "ppsnark.rs:284-285", "NMX_PPS_MASKED_EQ", "NMX_E_ARG", "NMX_E_SCALAR_RANGE", "num_masked_vars > ell", "all-zero",
                   "nothing written"):
        assert needle in m_doc, needle
    ffi = open(os.path.join(ROOT, "bindings", "rust", "nova-mi355x-sys", "src", "ffi.rs")).read()
    assert "pub fn nmx_ppsnark_spark_repr(" in ffi and "pub fn nmx_masked_eq_evals(" in ffi, "ffi.rs: regenerate with scripts/gen_rust_sys.py"


def test_python_and_cpp_wrappers_exist():
    from nova_amd import fieldvec as fv
    assert list(inspect.signature(fv.ppsnark_spark_repr).parameters) == ["mats", "n", "mont", "device"]
    assert list(inspect.signature(fv.ppsnark_spark_size).parameters) == ["nnzs", "num_vars", "num_cons"]
    assert list(inspect.signature(fv.masked_eq_evals).parameters) == ["field", "r", "num_masked_vars", "mont", "device"]
    res = open(os.path.join(ROOT, "include", "nova_mi355x.hpp")).read().split("namespace resident {")[1]
    for decl in ("inline void ppsnark_spark_repr(const std::vector<uint64_t>& mats", "inline size_t ppsnark_spark_size(", "inline void masked_eq_evals(int field"):
        assert decl in res, decl
    assert '#include "ppsnark_key.hpp"' in open(os.path.join(CSRC, "fieldvec.hip")).read()


def test_spark_size_is_the_references_formula():
    """ppsnark.rs:118-121, in the Python wrapper and in the tests' restatement"""
    from nova_amd import fieldvec as fv
    for nnzs, nv, nc, want in (([0, 0, 0], 0, 0, 1), ([192, 192, 192], 64, 64, 1024), ([64, 64, 64], 128, 64, 256), ([1, 0, 0], 1, 3, 4),
                               ([100, 100, 56], 64, 64, 256), ([100, 100, 57], 64, 64, 512), ([5], 1, 1000, 1024)):
        assert fv.ppsnark_spark_size(nnzs, nv, nc) == kc.spark_size(nnzs, nv, nc) == want


# ---- (2) argument errors --------------------------------------------------------------------------------------------------------------
def test_spark_repr_argument_errors_need_no_device_and_touch_nothing(L):
    from nova_amd import _lib
    n = 4
    buf = np.ascontiguousarray(fc.rand_vec(1, 8 * n, 3).copy())     # vector j of 8 = [n j, n j + n)
    before = buf.copy()
    at = lambda j, off=0: buf.ctypes.data + 32 * (n * j + off)  # noqa: E731
    unknown = (ctypes.c_uint64 * 8)(*[(1 << 62) + j for j in range(8)])       # handles nothing was registered under

    def s(handles=unknown, k=3, n_=n, flags=0, row=at(0), col=at(1), vals=(at(2), at(3), at(4)), ts_row=at(5), ts_col=at(6)):
        v = None if vals is None else (ctypes.c_void_p * 8)(*(list(vals) + [None] * (8 - len(vals))))
        return L.nmx_ppsnark_spark_repr(handles, k, n_, flags, row, col, v, ts_row, ts_col)
    A, TL, H = _lib.E_ARG, _lib.E_TOO_LARGE, _lib.E_HANDLE
    assert s(handles=None) == A
    assert s(k=0) == A and s(k=9) == A
    for fl in (_lib.ASYNC, _lib.BASES_MONT, _lib.BASES_DEVICE, _lib.OUT_PARTIAL, 1 << 20, _lib.ASYNC | _lib.SCALARS_DEVICE):
        assert s(flags=fl) == A, fl                                            # (NMX_ASYNC: defined for other calls, not accepted here)
    assert s(n_=1 << 32) == TL and s(n_=(1 << 63) + 1) == TL and s(n_=1 << 40) == TL
    assert s(n_=0) == A and s(n_=3) == A and s(n_=6) == A and s(n_=(1 << 31) + 1) == A
    assert b"power of two" in L.nmx_last_error()
    # two outputs that overlap, by one element at either end, among every kind of output
    assert s(col=at(0)) == A and s(col=at(0, n - 1)) == A and s(ts_col=at(5, 1)) == A and s(vals=(at(2), at(2, 1), at(4))) == A
    assert b"overlap" in L.nmx_last_error()
    assert s(vals=(at(2), at(3), at(5, n - 1))) == A and s(ts_row=at(0, 1)) == A and s(row=at(6, n - 1)) == A
    assert b"overlap" in L.nmx_last_error()
    # past every check that needs no matrix: what stops the call is the handle -- with or without a device, with or without outputs
    assert s() == H and s(flags=_lib.SCALARS_MONT) == H and s(k=1) == H and s(k=8, vals=None) == H
    assert s(row=None, col=None, vals=None, ts_row=None, ts_col=None) == H and s(vals=(None, at(3), None)) == H
    assert b"unknown matrix handle" in L.nmx_last_error()
    assert (buf == before).all(), "a refused call wrote something"


def test_masked_eq_argument_errors_need_no_device_and_touch_nothing(L):
    from nova_amd import _lib
    fid, ell = 1, 3
    p = fc.FIELDS[fid]
    out = np.ascontiguousarray(fc.rand_vec(fid, 1 << ell, 4).copy())
    before = out.copy()

    def m(field=fid, r=(5, 6, 7), ell_=None, masked=1, flags=0, null=None):
        rw = fc.vec(list(r)).copy() if len(r) else np.zeros((1, 32), np.uint8)
        return L.nmx_masked_eq_evals(field, None if null == "r" else rw.ctypes.data, len(r) if ell_ is None else ell_, masked, flags,
                                     None if null == "out" else out.ctypes.data)
    A, SR = _lib.E_ARG, _lib.E_SCALAR_RANGE
    for bad in (p, p + 1, (1 << 256) - 1):
        for pos in range(ell):
            r = [5, 6, 7]
            r[pos] = bad
            assert m(r=r) == SR, (hex(bad), pos)
    assert m(masked=ell + 1) == A
    assert b"num_masked_vars > ell" in L.nmx_last_error()
    assert m(masked=1 << 40) == A and m(r=(), masked=1) == A
    assert m(r=[1] * 31) == A and m(r=[1] * 31, masked=31) == A and m(ell_=1 << 40) == A
    assert m(null="r") == A and m(null="out") == A
    assert m(field=4) == A and m(field=-1) == A
    assert b"bad field id" in L.nmx_last_error()
    for fl in (_lib.ASYNC, _lib.BASES_MONT, _lib.BASES_DEVICE, _lib.OUT_PARTIAL, 1 << 20, _lib.ASYNC | _lib.SCALARS_DEVICE):
        assert m(flags=fl) == A, fl
    assert (out == before).all(), "a refused call wrote something"
    # a well-formed call gets past every check: what stops it without a device is NMX_E_NO_DEVICE, nothing else
    ok = 0 if L.nmx_device_count() > 0 else _lib.E_NO_DEVICE
    assert m() == ok and m(masked=ell) == ok and m(masked=0, flags=_lib.SCALARS_MONT) == ok and m(r=(), masked=0) == ok
    if ok:
        assert (out == before).all()


# ---- (3) the kernels under the emulation -------------------------------------------------------------------------------------------------
EMUL_SRC = os.path.join(ROOT, "tests", "host_emul", "ppsnark_key_emul.cpp")
EMUL_SO = os.path.join(ROOT, "tests", "host_emul", "libnmx_ppsnark_key_emul.so")
RI = 1 << 261          # the internal residue form: x * 2^261 mod p (nova_amd/csrc/fp.hpp)
R256 = kc.R256         # the Montgomery form of NMX_SCALARS_MONT
COL_BITS = 28          # kSpmvColBits (nova_amd/csrc/spmv_row.hpp)
SLACK = 0xdeadbeef


@pytest.fixture(scope="module")
def E():
    deps = [EMUL_SRC, os.path.join(ROOT, "tests", "host_emul", "simt.hpp")] + [os.path.join(CSRC, f) for f in ("fp.hpp", "ppsnark_key.hpp", "ppsnark_oracles.hpp",
                                                                                                            "spmv_row.hpp", "msm_partition.hpp")]
    if not os.path.exists(EMUL_SO) or os.path.getmtime(EMUL_SO) < max(os.path.getmtime(x) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", EMUL_SO, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_SO)
    vp, u32, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    lib.emul_pps_key_expand.argtypes = [i, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.emul_pps_key_hist.argtypes = [u32, u32, vp, vp, vp, vp, vp, vp]
    lib.emul_pps_key_ts_col.argtypes = [i, vp, vp, u32, u32, vp]
    lib.emul_pps_key_geometry.argtypes = [vp]
    lib.emul_pps_key_slot.argtypes = [u32]
    lib.emul_pps_key_slot.restype = u32
    return lib


def words(vals):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in vals) or bytes(32), np.uint32).copy()


def coefficient_class(p, v):
    """SpmvClassifyFn (nova_amd/csrc/fieldvec.hip): 0 general, 1 +1, 2 -1, 3..8 +2..+7, 9..14 -2..-7"""
    if 1 <= v <= 7:
        return 1 if v == 1 else v + 1
    if 1 <= p - v <= 7:
        return 2 if p - v == 1 else p - v + 7
    return 0


def resident(p, mat):
    """what registration leaves in HBM: indptr, indices with the class bits (columns fit 28 bits here), data in the internal form"""
    ip, ix, vs = mat
    return (np.array(ip, np.uint32), np.array([c | (coefficient_class(p, v) << COL_BITS) for c, v in zip(ix, vs)] or [0], np.uint32),
            words([v * RI % p for v in vs]))


def emul_spark_repr(E, fid, mats, n, mont, skip=()):
    """the three passes over the resident form of mats -> (row, col, vals, ts_row, ts_col) as stored words (integers); outputs named in
    `skip` ("row", "col", "vals", "ts_row", "v1": the value vector of matrix 1) are passed as NULL and come back None"""
    p, k = fc.FIELDS[fid], len(mats)
    res = [resident(p, m) for m in mats]
    ptrs = lambda j: (ctypes.c_void_p * 8)(*[r[j].ctypes.data for r in res])  # noqa: E731
    nnz = np.array([len(m[1]) for m in mats], np.uint32)
    rows = np.array([len(m[0]) - 1 for m in mats], np.uint32)
    cols = np.array([max(list(m[1]) + [0]) + 1 for m in mats], np.uint32)
    form = R256 if mont else 1
    consts = words([form * RI % p, form % p])
    fresh = lambda: np.full(8 * n + 8, SLACK, np.uint32)  # noqa: E731
    row, col, ts_row, ts_col = fresh(), fresh(), fresh(), fresh()
    vals = [fresh() for _ in range(k)]
    vptr = (ctypes.c_void_p * 8)(*[None if ("v%d" % j) in skip else vals[j].ctypes.data for j in range(k)])
    assert E.emul_pps_key_expand(fid, k, n, ptrs(0), ptrs(1), ptrs(2), nnz.ctypes.data, rows.ctypes.data, cols.ctypes.data, consts.ctypes.data,
                                 None if "row" in skip else row.ctypes.data, None if "col" in skip else col.ctypes.data,
                                 None if "vals" in skip else vptr, None if "ts_row" in skip else ts_row.ctypes.data) == 0
    count = np.zeros(n + 1, np.uint32)
    count[n] = SLACK
    assert E.emul_pps_key_hist(k, n, ptrs(0), ptrs(1), nnz.ctypes.data, rows.ctypes.data, cols.ctypes.data, count.ctypes.data) == 0
    assert count[n] == SLACK, "a store past the end of the counters"
    assert int(count[:n].sum()) == int(nnz.sum())
    assert E.emul_pps_key_ts_col(fid, count.ctypes.data, ts_col.ctypes.data, n, int(nnz.sum()), consts.ctypes.data) == 0
    out = []
    for name, o in [("row", row), ("col", col)] + [("v%d" % j, v) for j, v in enumerate(vals)] + [("ts_row", ts_row), ("ts_col", ts_col)]:
        assert (o[8 * n:] == SLACK).all(), "a store past the end of " + name
        if name in skip or (name.startswith("v") and "vals" in skip):
            assert (o == SLACK).all(), "a NULL output was written: " + name
            out.append(None)
        else:
            out.append(fc.ints(o[:8 * n].view(np.uint8)))
    return out[0], out[1], out[2:2 + k], out[2 + k], out[3 + k]


def expect(p, mats, n, mont):
    row, col, vals, ts_row, ts_col = kc.spark_repr(mats, n)
    assert sum(ts_row) == n and sum(ts_col) == n
    f = lambda v: kc.to_form(p, v, mont)  # noqa: E731
    return f(row), f(col), [f(v) for v in vals], f(ts_row), f(ts_col)


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
@pytest.mark.parametrize("mont", [False, True])
def test_emulated_spark_repr_k3(E, fid, mont):
    """every shape of kc.shape_cases with three matrices: row counts 1 .. 1000 with empty leading and last rows, total == n and n - 1 with real
    entries in column n - 1 and row 0, nothing at all (n == 1), the heavy column, and a tile of 2048 distinct columns"""
    p = fc.FIELDS[fid]
    for name, mats, n in kc.shape_cases(fid, 3):
        assert emul_spark_repr(E, fid, mats, n, mont) == expect(p, mats, n, mont), name


@pytest.mark.parametrize("k", [1, 8])
def test_emulated_spark_repr_k1_and_k8(E, k):
    for fid, mont in ((1, False), (2, True)):
        p = fc.FIELDS[fid]
        for name, mats, n in kc.shape_cases(fid, k):
            assert emul_spark_repr(E, fid, mats, n, mont) == expect(p, mats, n, mont), (name, k)


def test_emulated_special_shapes_are_what_they_claim(E):
    """the shapes hit the edges they are there for: n == total, n == total + 1, ts = [1] at n == 1, real and padding counts on one address,
    an entry of the heavy column in every row, and a tile that cannot fit the block's table -- so the fall-back is taken"""
    geo = np.zeros(4, np.uint32)
    E.emul_pps_key_geometry(geo.ctypes.data)
    tile, slots, probes, threads = (int(x) for x in geo)
    assert tile == 8 * threads and probes >= 1
    cases = {name: (mats, n) for name, mats, n in kc.shape_cases(1, 3)}
    mats, n = cases["full"]
    assert sum(len(m[1]) for m in mats) == n and n - 1 in mats[0][1] and mats[0][0][1] > 0
    mats, n = cases["full-1"]
    row, col, _v, ts_row, ts_col = kc.spark_repr(mats, n)
    assert sum(len(m[1]) for m in mats) == n - 1 and ts_row[0] >= 2 and ts_col[n - 1] >= 2 and row[n - 1] == 0 and col[n - 1] == n - 1
    mats, n = cases["empty"]
    assert n == 1 and kc.spark_repr(mats, n) == ([0], [0], [[0]] * 3, [1], [1])
    mats, n = cases["heavy"]
    assert kc.spark_repr(mats, n)[4][0] >= 3 * 300
    mats, n = cases["distinct"]
    stream = [c for m in mats for c in m[1]]
    assert len(set(stream[:tile])) > slots, "the first tile holds more distinct columns than the table has slots"
    # and with probing bounded, even a tile that would fit can overflow a neighbourhood: count what the table cannot place, thread by thread
    key, lost = {}, 0
    for t in range(threads):
        for u in range(tile // threads):
            c = stream[u * threads + t]
            h = E.emul_pps_key_slot(c)
            for pr in range(probes):
                s = (h + pr) % slots
                if key.setdefault(s, c) == c:
                    break
            else:
                lost += 1
    assert lost >= tile - slots > 0


def test_emulated_mixed_coefficients_and_class_bits(E):
    """fv_common.mixed_coefficient_case: values 1, p - 1, small and general; their class bits sit above the column in the resident indices and
    must not reach col or ts_col, and the values come back whatever their class"""
    for fid in sorted(fc.FIELDS):
        p = fc.FIELDS[fid]
        for k in (1, 3):
            mats, n = kc.mixed_coefficient_mats(fid, k)
            assert any(coefficient_class(p, v) for v in mats[0][2]) and any(coefficient_class(p, v) == 0 for v in mats[0][2])
            for mont in (False, True):
                assert emul_spark_repr(E, fid, mats, n, mont) == expect(p, mats, n, mont)


def test_emulated_null_outputs_are_skipped(E):
    fid = 1
    p = fc.FIELDS[fid]
    _name, mats, n = kc.shape_cases(fid, 3)[4]
    want = expect(p, mats, n, False)
    for skip in (("row",), ("col", "ts_row"), ("vals",), ("v1",), ("row", "col", "v0", "v2", "ts_row")):
        got = emul_spark_repr(E, fid, mats, n, False, skip=skip)
        flat_g = [got[0], got[1]] + got[2] + [got[3], got[4]]
        flat_w = [want[0], want[1]] + want[2] + [want[3], want[4]]
        for g, w in zip(flat_g, flat_w):
            assert g is None or g == w, skip
        assert sum(g is None for g in flat_g) == (3 if "vals" in skip else len(skip))


def test_masked_table_definition_agrees_with_its_closed_form(L):
    """kc.masked_eq_table (masked_eq.rs:57-75), what nmx_masked_eq_evals is compared with, and kc.masked_eq_evaluate (:34-52), what the chained
    GPU test's final claim uses, describe one polynomial; identity_evaluate is the MLE of i"""
    import random
    assert hasattr(L, "nmx_masked_eq_evals")
    from tests.spartan_common import mle_eval
    for fid in (1, 2):
        p = fc.FIELDS[fid]
        rng = random.Random(fid)
        for ell in (1, 3, 5):
            r, x = [rng.randrange(p) for _ in range(ell)], [rng.randrange(p) for _ in range(ell)]
            for m in (0, 1, ell - 1, ell):
                assert mle_eval(p, kc.masked_eq_table(p, r, m), x) == kc.masked_eq_evaluate(p, r, m, x), (ell, m)
            assert mle_eval(p, list(range(1 << ell)), x) == kc.identity_evaluate(p, x)


# ---- the C++ wrappers --------------------------------------------------------------------------------------------------------------------
def test_cpp_wrappers_compile_and_refuse_with_the_librarys_codes(L):
    """tests/cpp/ppsnark_key_mirror_test.cpp: nova::resident::ppsnark_spark_size / ppsnark_spark_repr / masked_eq_evals built with g++ against
    the product library; everything it checks is decided before a device is leased, so it runs the same with and without a GPU"""
    src = os.path.join(ROOT, "tests", "cpp", "ppsnark_key_mirror_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "ppsnark_key_mirror_test.bin")
    deps = [src, os.path.join(ROOT, "include", "nova_mi355x.hpp"), os.path.join(ROOT, "include", "nova_mi355x.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, src, "-L" + os.path.join(ROOT, "nova_amd"), "-lnova_mi355x",
                               "-Wl,-rpath," + os.path.join(ROOT, "nova_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ppsnark key mirror ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
