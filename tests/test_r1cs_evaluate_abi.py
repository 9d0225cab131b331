"""nmx_r1cs_evaluate without a GPU.  (1) The yardstick first: tests/r1cs_eval_common.restate (the sum of snark.rs:325-353 in Python big
integers) agrees with oracle.pyref.spmv + oracle.pyref.mle_evaluate through M~(r_x, r_y) = mle_evaluate(M T_y, r_x).  (2) The entry
point is declared, exported and bound in Python / C++ / Rust with the header's argument types, and every argument error of the
header returns with no device present, nothing written.  (3) The kernel's lane body (nova_amd/csrc/r1cs_eval.hpp) runs thread by
thread under tests/host_emul/simt.hpp on matrices with every coefficient class, empty rows, a row count that is no power of two and
fewer columns than 2^ell_y, at several grid sizes, and must give the restatement byte for byte.  What the emulation covers is the
lane body and the partition of rows over lanes and blocks: the lane sums are added up here in Python.  The wave / block reduction
(shuffles), k_r1cs_eval_finish and the host half of the call (the folding of the upper variables into the tables, the split of T_x)
are NOT run on the CPU; tests/test_gpu_r1cs_evaluate.py covers them, at several grid sizes and against differently composed paths."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from oracle import pyref as R
from tests import fv_common as C
from tests import r1cs_eval_common as V
from tests.spmv_edges_common import coefficient_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "r1cs_eval_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "r1cs_eval_mirror_test.bin")
EMUL_SRC = os.path.join(ROOT, "tests", "host_emul", "r1cs_eval_emul.cpp")
EMUL_SO = os.path.join(ROOT, "tests", "host_emul", "libnmx_r1cs_eval_emul.so")
CSRC = os.path.join(ROOT, "nova_amd", "csrc")


@pytest.fixture(scope="module")
def L():
    from nova_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- (1) the yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", sorted(C.FIELDS))
@pytest.mark.parametrize("rows,cols,ell_x,ell_y", [(97, 83, 7, 7), (64, 64, 6, 6), (5, 3, 4, 2), (1, 1, 0, 0)])
def test_restatement_equals_spmv_then_mle_evaluate(fid, rows, cols, ell_x, ell_y):
    p = C.FIELDS[fid]
    mats = [V.classes_csr(fid, rows, cols, seed=3 + j + fid) for j in range(2)] + [C.random_csr(fid, rows, cols, seed=9 + fid)]
    rx, _ = V.point(fid, ell_x, 50 + fid)
    ry, _ = V.point(fid, ell_y, 60 + fid)
    got = V.restate(p, mats, rx, ry)
    assert got == V.restate_via_products(p, mats, 1 << ell_x, rx, ry)
    assert len(set(got)) > 1 or rows == 1


def test_restatement_on_a_hand_computed_instance():
    """the instance of tests/cpp/r1cs_eval_mirror_test.cpp: T_x = [2, -3, -4, 6], T_y[4] = -2, T_y[5] = 3"""
    p = C.FIELDS[1]
    A = ([0, 1, 3, 4], [0, 0, 1, 5], [1, 1, 1, 1])
    B = ([0, 1, 2, 3], [1, 4, 0], [1, 1, 1])
    Cm = ([0, 1, 2, 3], [2, 3, 4], [1, 1, 14])
    assert R.eq_evals(p, [2, 3]) == [2, p - 3, p - 4, 6]
    assert V.restate(p, [A, B, Cm], [2, 3], [1, 0, 3]) == [p - 12, 6, 112]
    assert V.restate(p, [A, B, Cm], [0, 1], [1, 0, 0]) == [0, 1, 0]


# ---- (2) the surface -------------------------------------------------------------------------------------------------------------
def test_header_declares_library_exports_and_python_binds_the_same_types(L):
    hdr = open(os.path.join(ROOT, "include", "nova_mi355x.h")).read()
    m = re.search(r"int nmx_r1cs_evaluate\(([^;]*)\);", hdr)
    assert m, "the header does not declare nmx_r1cs_evaluate"
    params = [re.sub(r"/\*.*?\*/", "", x).strip() for x in re.sub(r"\s+", " ", m.group(1)).split(",")]
    assert params == ["const uint64_t* handles", "size_t k", "const void* r_x", "size_t ell_x", "const void* r_y", "size_t ell_y",
                      "uint32_t flags", "uint8_t* out"]
    assert hasattr(L, "nmx_r1cs_evaluate")
    ctype_of = lambda d: ctypes.c_size_t if d.startswith("size_t") else ctypes.c_uint32 if d.startswith("uint32_t") else ctypes.c_void_p  # noqa: E731
    assert list(L.nmx_r1cs_evaluate.argtypes) == [ctype_of(d) for d in params]
    doc = hdr.split("int nmx_r1cs_evaluate(")[0].rsplit("/*", 1)[1]
    for needle in ("snark.rs:325-353", "NMX_E_HANDLE", "NMX_E_ARG", "rows <= 2^ell_x", "cols <= 2^ell_y", "NMX_SCALARS_MONT",
                   "nothing is written", "NMX_ASYNC", "logical device 0", "TRANSPOSED"):
        assert needle in doc, needle
    ffi = open(os.path.join(ROOT, "bindings", "rust", "nova-mi355x-sys", "src", "ffi.rs")).read()
    assert "pub fn nmx_r1cs_evaluate(" in ffi, "ffi.rs: regenerate with scripts/gen_rust_sys.py"


def test_python_and_cpp_wrappers_exist():
    import inspect
    from nova_amd import fieldvec as fv
    assert list(inspect.signature(fv.r1cs_evaluate).parameters) == ["mats", "r_x", "r_y", "mont"]
    hpp = open(os.path.join(ROOT, "include", "nova_mi355x.hpp")).read()
    assert "inline std::vector<Scalar> r1cs_evaluate(const uint64_t* mats, size_t k" in hpp.split("namespace resident {")[1]


def call(L, handles=(1, 2, 3), k=None, rx=True, ell_x=2, ry=True, ell_y=2, flags=0, out=True, hs_null=False):
    """-> (return code, whether the output buffer is untouched)"""
    hs = (ctypes.c_uint64 * 9)(*handles)
    pts = np.zeros((8, 32), np.uint8)
    pts[:, 0] = 1
    buf = np.full(9 * 32, 0x5a, np.uint8)
    rc = L.nmx_r1cs_evaluate(None if hs_null else ctypes.addressof(hs), len(handles) if k is None else k, pts.ctypes.data if rx else None, ell_x,
                             pts.ctypes.data if ry else None, ell_y, flags, buf.ctypes.data if out else None)
    return rc, bool((buf == 0x5a).all())


def test_argument_errors_need_no_device_and_write_nothing(L):
    from nova_amd import _lib
    A = (_lib.E_ARG, True)
    assert call(L, k=0) == A
    assert call(L, handles=(1,) * 9) == A                       # k = 9
    assert call(L, out=False)[0] == _lib.E_ARG
    assert call(L, hs_null=True) == A
    assert call(L, rx=False) == A and call(L, ry=False) == A   # null points with ell > 0
    for fl in (_lib.SCALARS_DEVICE, _lib.ASYNC, _lib.BASES_MONT, _lib.SCALARS_MONT | _lib.SCALARS_DEVICE, 1 << 20):
        assert call(L, flags=fl) == A, fl
    assert call(L, ell_x=31) == A and call(L, ell_y=31) == A   # as nmx_eq_evals_from_points
    assert b"1 .. 8 matrices" in (call(L, k=0), L.nmx_last_error())[1]
    # well-formed arguments get PAST the argument checks: what stops the call is the handle that was never registered -- NMX_E_HANDLE,
    # not NMX_E_ARG, with or without a device (handles are looked up before a device is needed); null points are fine with ell = 0
    for kw in (dict(), dict(flags=_lib.SCALARS_MONT), dict(handles=(7,)), dict(handles=(1,) * 8), dict(rx=False, ell_x=0, ry=False, ell_y=0)):
        assert call(L, **kw) == (_lib.E_HANDLE, True), kw
    assert b"unknown matrix handle" in L.nmx_last_error()


def build_cpp():
    import __graft_entry__
    __graft_entry__.build()
    deps = [SRC, os.path.join(ROOT, "include", "nova_mi355x.hpp"), os.path.join(ROOT, "include", "nova_mi355x.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", BIN, SRC, "-L" + os.path.join(ROOT, "nova_amd"), "-lnova_mi355x",
                               "-Wl,-rpath," + os.path.join(ROOT, "nova_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return BIN


def test_cpp_mirror_builds_and_passes_or_refuses_without_gpu(L):
    b = build_cpp()
    r = subprocess.run([b], capture_output=True, text=True)
    if L.nmx_device_count() > 0:
        assert r.returncode == 0 and "r1cs_eval mirror ok" in r.stdout, (r.returncode, r.stderr)
        return
    assert r.returncode == 3, (r.returncode, r.stderr)
    assert "no HIP device" in r.stderr


# ---- (3) the lane body under the emulation --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def E():
    deps = [EMUL_SRC, os.path.join(ROOT, "tests", "host_emul", "simt.hpp")] + [os.path.join(CSRC, f) for f in ("fp.hpp", "r1cs_eval.hpp", "spmv_row.hpp", "msm_partition.hpp")]
    if not os.path.exists(EMUL_SO) or os.path.getmtime(EMUL_SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", EMUL_SO, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_SO)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.emul_r1cs_eval.argtypes = [ctypes.c_int, u32, vp, vp, vp, vp, vp, vp, u32, vp, u32, vp]
    return lib


RI = 1 << 261  # the internal residue form: x * 2^261 mod p (nova_amd/csrc/fp.hpp)


def u32_words(vals):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in vals) or bytes(32), np.uint32).copy()


def emulate(E, fid, mats, rx, ry, bpm=0, tagged=True):
    """the device-side inputs exactly as the host half hands them over, computed here with big integers"""
    p = C.FIELDS[fid]
    k = len(mats)
    max_rows, max_cols = max(len(m[0]) - 1 for m in mats), max(max(int(c) for c in m[1]) + 1 if len(m[1]) else 1 for m in mats)
    effx, effy = max(max_rows - 1, 0).bit_length(), max(max_cols - 1, 0).bit_length()
    topx, topy = len(rx) - effx, len(ry) - effy
    assert topx >= 0 and topy >= 0
    top = 1
    for r in list(rx[:topx]) + list(ry[:topy]):
        top = top * (1 - r) % p
    sx = effx // 2
    xL = [e * top % p * RI % p for e in R.eq_evals(p, list(rx[topx:topx + effx - sx]))]
    xR = [e * RI % p for e in R.eq_evals(p, list(rx[topx + effx - sx:]))]
    ty = R.eq_evals(p, list(ry[topy:]))
    keep, ips, ixs, dts, rows = [], [], [], [], []
    for ip, ix, dt in mats:
        d = C.ints(dt)
        cls = [coefficient_class(p, v) if tagged else 0 for v in d]
        keep += [np.asarray(ip, np.uint32).copy(), np.array([int(c) | (t << 28) for c, t in zip(ix, cls)], np.uint32), u32_words([v * RI % p for v in d])]
        ips.append(keep[-3].ctypes.data), ixs.append(keep[-2].ctypes.data), dts.append(keep[-1].ctypes.data)
        rows.append(len(ip) - 1)
    arr = lambda ptrs: (ctypes.c_void_p * k)(*ptrs)  # noqa: E731
    a_ip, a_ix, a_dt, a_rows = arr(ips), arr(ixs), arr(dts), np.array(rows, np.uint32)
    wxL, wxR, wty = u32_words(xL), u32_words(xR), u32_words(ty)
    lanes = np.zeros(k * 1024 * 256 * 32 if not bpm else k * bpm * 256 * 32, np.uint8)
    g = E.emul_r1cs_eval(fid, k, ctypes.addressof(a_ip), ctypes.addressof(a_ix), ctypes.addressof(a_dt), a_rows.ctypes.data, wxL.ctypes.data,
                         wxR.ctypes.data, sx, wty.ctypes.data, bpm, lanes.ctypes.data)
    assert g >= 1
    sums = C.ints(lanes[:k * g * 256 * 32])
    assert all(s < p for s in sums), "a lane's result is not the canonical representative"
    return [sum(sums[j * g * 256:(j + 1) * g * 256]) % p for j in range(k)], g


@pytest.mark.parametrize("fid", sorted(C.FIELDS))
def test_emulated_lanes_give_the_restatement_at_two_grid_sizes(E, fid):
    p = C.FIELDS[fid]
    rows, cols, ell_x, ell_y = 700, 300, 10, 9   # rows no power of two, cols < 2^ell_y, empty rows, every class, a 40-entry row
    mats = [V.classes_csr(fid, rows, cols, seed=20 + fid), V.classes_csr(fid, rows - 187, cols - 45, seed=30 + fid, empty_every=3),
            C.random_csr(fid, rows, cols, seed=40 + fid)]
    classes = {coefficient_class(p, v) for v in C.ints(mats[0][2])}
    assert classes == set(range(15)), "the fixture must exercise every coefficient class"
    assert any(mats[0][0][i] == mats[0][0][i + 1] for i in range(rows))
    rx, _ = V.point(fid, ell_x, 70 + fid)
    ry, _ = V.point(fid, ell_y, 80 + fid)
    want = V.restate(p, mats, rx, ry)
    got, g = emulate(E, fid, mats, rx, ry)
    assert g == 3 and got == want
    got, g = emulate(E, fid, mats, rx, ry, bpm=1)   # one block per matrix: every lane walks three rows
    assert g == 1 and got == want
    got, _ = emulate(E, fid, mats, rx, ry, bpm=7)   # more blocks than rows need: the surplus lanes contribute zero
    assert got == want
    got, _ = emulate(E, fid, mats, rx, ry, tagged=False)  # the same matrices untagged (class 0 everywhere): the general product
    assert got == want


@pytest.mark.parametrize("fid", [1, 2])
def test_emulated_edge_shapes(E, fid):
    p = C.FIELDS[fid]
    rng = random.Random(5 + fid)
    one = (np.array([0, 1], np.uint64), np.array([0], np.uint64), C.vec([p - 2]))
    empty = (np.zeros(4, np.uint64), np.zeros(0, np.uint64), np.zeros((0, 32), np.uint8))
    assert emulate(E, fid, [one], [], [])[0] == [p - 2] == V.restate(p, [one], [], [])          # 1 x 1, ell_x = ell_y = 0
    assert emulate(E, fid, [empty, one], [3, 4], [])[0] == V.restate(p, [empty, one], [3, 4], [])  # no entries: 0
    # variables above the bits the shapes need, and coordinates 0 and 1 (eq collapses)
    mats = [V.classes_csr(fid, 37, 21, seed=3)]
    for rx, ry in (([rng.randrange(p) for _ in range(9)], [rng.randrange(p) for _ in range(8)]),
                   ([0, 0, 0, 1, 0, 0, 1, 0, 0], [0, 0, 0, 1, 0, 1, 0, 0]),
                   ([1] + [rng.randrange(p) for _ in range(8)], [rng.randrange(p) for _ in range(8)])):
        assert emulate(E, fid, mats, rx, ry)[0] == V.restate(p, mats, rx, ry)
