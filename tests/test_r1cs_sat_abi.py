"""nmx_r1cs_is_sat without a GPU: the entry point is exported and bound in Python and C++, refuses to compute without a device, and
the instance builder the GPU tests use (tests/r1cs_sat_common.py) is itself right according to oracle.pyref -- constructed instances
have an all-zero oracle residual and every corruption makes exactly the claimed rows non-zero -- so a failure of
tests/test_gpu_r1cs_sat.py cannot be the test's own arithmetic.  R1CSShape::is_sat / is_sat_relaxed: src/r1cs/mod.rs:474-574."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import pyref as R
from tests import fv_common as C
from tests import r1cs_sat_common as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "r1cs_sat_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "r1cs_sat_mirror_test.bin")


@pytest.fixture(scope="module")
def L():
    from nova_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def build_cpp():
    """tests/cpp/r1cs_sat_mirror_test.cpp with g++ against the header, the product library and the oracle (as tests/test_cpp_mirror.py)."""
    import __graft_entry__
    __graft_entry__.build()
    deps = [SRC, os.path.join(ROOT, "include", "nova_mi355x.hpp"), os.path.join(ROOT, "include", "nova_mi355x.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", BIN, SRC,
                               "-L" + os.path.join(ROOT, "nova_amd"), "-lnova_mi355x",
                               "-L" + os.path.join(ROOT, "oracle"), "-lnova_ref",
                               "-Wl,-rpath," + os.path.join(ROOT, "nova_amd"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
                               "-Wl,-rpath,/opt/rocm/lib"])
    return BIN


def test_symbol_is_exported_and_bound(L):
    from nova_amd import _lib
    assert hasattr(L, "nmx_r1cs_is_sat")
    assert len(L.nmx_r1cs_is_sat.argtypes) == 22
    assert (_lib.UNSAT_EQ, _lib.UNSAT_COMM_W, _lib.UNSAT_COMM_E) == (1, 2, 4)
    hdr = open(os.path.join(ROOT, "include", "nova_mi355x.h")).read()
    assert "NMX_UNSAT_EQ = 1u << 0, NMX_UNSAT_COMM_W = 1u << 1, NMX_UNSAT_COMM_E = 1u << 2" in hdr


def test_python_wrappers_exist():
    import inspect
    from nova_amd import fieldvec as fv
    assert list(inspect.signature(fv.r1cs_is_sat).parameters)[:9] == ["A", "B", "C", "ck", "W", "X", "comm_W", "r_W", "h"]
    assert list(inspect.signature(fv.r1cs_is_sat_relaxed).parameters)[:13] == ["A", "B", "C", "ck", "W", "E", "u", "X", "comm_W", "comm_E", "r_W",
                                                                            "r_E", "h"]
    r = fv.SatResult(5, 3, 17)
    assert (r.ok, r.eq_ok, r.comm_W_ok, r.comm_E_ok, r.bad_rows, r.first_bad_row) == (False, False, True, False, 3, 17)
    r = fv.SatResult(0, 0, 2 ** 64 - 1)
    assert r.ok and r.eq_ok and r.comm_W_ok and r.comm_E_ok and r.first_bad_row is None and bool(r)


def test_refuses_without_a_device_and_leaves_the_verdict_alone(L):
    if L.nmx_device_count() > 0:
        return  # (a device is visible: tests/test_gpu_r1cs_sat.py covers the call)
    from nova_amd import _lib
    verdict, bad, first = ctypes.c_uint32(0xabcd), ctypes.c_uint64(77), ctypes.c_uint64(78)
    buf = np.zeros((4, 64), np.uint8)
    p = buf.ctypes.data
    rc = L.nmx_r1cs_is_sat(1, 2, 3, 4, p, 2, p, 2, p, p, 1, p, p, p, p, 0, p, 0, 0, ctypes.byref(verdict), ctypes.byref(bad), ctypes.byref(first))
    assert rc == _lib.E_NO_DEVICE
    assert b"no HIP device" in L.nmx_last_error()
    assert (verdict.value, bad.value, first.value) == (0xabcd, 77, 78)
    # the strict form and the equation-only form as well
    assert L.nmx_r1cs_is_sat(1, 2, 3, 0, p, 2, None, 0, None, p, 1, None, None, None, None, 0, None, 0, 0, ctypes.byref(verdict), None,
                             None) == _lib.E_NO_DEVICE
    assert verdict.value == 0xabcd
    assert L.nmx_r1cs_is_sat(1, 2, 3, 0, p, 2, None, 0, None, p, 1, None, None, None, None, 0, None, 0, 0, None, None, None) == _lib.E_ARG


def test_cpp_mirror_has_the_pair_and_refuses_without_gpu(L):
    hpp = open(os.path.join(ROOT, "include", "nova_mi355x.hpp")).read()
    assert "inline SatResult r1cs_is_sat(" in hpp and "inline SatResult r1cs_is_sat_relaxed(" in hpp
    assert "NMX_BASES_MONT" in hpp.split("inline SatResult r1cs_is_sat_relaxed(")[1].split("return s;")[0]
    b = build_cpp()
    if L.nmx_device_count() > 0:
        return  # (a device is visible: the binary runs in tests/test_gpu_r1cs_sat.py)
    r = subprocess.run([b], capture_output=True, text=True)
    assert r.returncode == 3, (r.returncode, r.stderr)
    assert "no HIP device" in r.stderr


# ---- the instance builder against the oracle ---------------------------------------------------------------------------------
SHAPES = [(97, 83), (64, 64)]


@pytest.mark.parametrize("fid", sorted(C.FIELDS))
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_constructed_instances_have_a_zero_oracle_residual(fid, rows, cols):
    for inst in (S.make_relaxed(fid, rows, cols, seed=3 + fid), S.make_strict(fid, rows, cols, seed=5 + fid)):
        assert inst.n_w + 1 + inst.n_io == cols
        assert inst.residual() == [0] * rows
        assert inst.bad_rows() == (0, 2 ** 64 - 1)
        # the same through the pure-Python product (oracle.pyref.spmv), independent of the C oracle
        z = C.ints(inst.z())
        prods = [R.spmv(inst.p, [int(x) for x in ip], [int(x) for x in ix], C.ints(dt), z) for ip, ix, dt in inst.csr]
        assert prods == inst.products()
    strict = S.make_strict(fid, rows, cols, seed=5 + fid)
    assert all(int(c) == strict.n_w for c in strict.csr[2][1]) and C.ints(strict.z())[strict.n_w] == 1


@pytest.mark.parametrize("fid", sorted(C.FIELDS))
def test_each_corruption_violates_exactly_the_claimed_rows(fid):
    rows, cols = 97, 83
    inst = S.make_relaxed(fid, rows, cols, seed=11 + fid)
    p = inst.p
    for j in (0, 63, 64, rows // 2, rows - 1):
        for bad in (S.corrupt_E_plus_one(inst, j), S.corrupt_E_minus_one(inst, j)):
            res = bad.residual()
            assert [i for i, t in enumerate(res) if t] == [j]
            assert bad.bad_rows() == (1, j)
        assert S.corrupt_E_plus_one(inst, j).residual()[j] == p - 1 and S.corrupt_E_minus_one(inst, j).residual()[j] == 1
    # a changed witness element violates the rows whose A, B or C read that column with a non-zero effect: count them independently
    k = S.column_of_row(inst, rows // 2)
    assert k is not None
    bad = S.corrupt_W(inst, k)
    az0, bz0, cz0 = inst.products()
    az1, bz1, cz1 = bad.products()
    u = C.ints(inst.u)[0]
    want = [i for i in range(rows) if (az1[i] * bz1[i] - u * cz1[i] - (az0[i] * bz0[i] - u * cz0[i])) % p]
    assert want and [i for i, t in enumerate(bad.residual()) if t] == want
    assert bad.bad_rows() == (len(want), want[0])
    # a wrong u
    bad = S.corrupt_u(inst)
    az, bz, cz = bad.products()
    e = C.ints(inst.E)
    want = [i for i in range(rows) if (az[i] * bz[i] - (u + 1) * cz[i] - e[i]) % p]
    assert want and bad.bad_rows() == (len(want), want[0])
    # strict: one changed witness element
    st = S.make_strict(fid, rows, cols, seed=13 + fid)
    k = S.column_of_row(st, rows // 2)  # (the 40-entry row: some rows of a random matrix are empty)
    assert k is not None
    n, first = S.corrupt_W(st, k).bad_rows()
    assert n >= 1 and first <= rows // 2


def test_montgomery_form_and_expected_commitments():
    inst = S.make_relaxed(1, 40, 37, seed=21)
    m = S.to_mont(inst)
    Rm = 1 << 256
    assert C.ints(m.W) == [x * Rm % inst.p for x in C.ints(inst.W)] and C.ints(m.u) == [C.ints(inst.u)[0] * Rm % inst.p]
    bases, h = S.key_points(inst)
    assert len(bases) == max(inst.n_w, inst.rows)
    r_W, r_E = C.rand_vec(1, 1, 31), C.rand_vec(1, 1, 32)
    cw, ce = S.expected_commitments(inst, bases, h, r_W, r_E)
    pts = [R.xy64_to_point(bytes(b)) for b in bases]
    want = R.commit(R.BN254_G1, pts, R.xy64_to_point(h), C.ints(inst.W), C.ints(r_W)[0])  # the pure-Python commitment agrees with the C oracle
    assert cw == (R.point_to_xy64(want), int(want is R.INF))
    assert cw != ce and cw[1] == 0 and ce[1] == 0
