"""nmx_r1cs_evaluate on the GPU: RelaxedR1CSSNARK::verify's multi_evaluate (src/spartan/snark.rs:325-353) as one call.  Small sizes
against the big-integer restatement (tests/r1cs_eval_common.py, itself checked on the CPU by tests/test_r1cs_evaluate_abi.py); 2^14
and 2^20 against BOTH composed identities over entry points that are oracle-tested on their own,
    mle_multi_evaluate(spmv_apply_many(T_y), r_x)      and      mle_multi_evaluate(spmv_apply_many(transposed, T_x), r_y);
edge shapes, errors, no transposed form, threads, ordering behind NMX_ASYNC, and the equation the call exists for (snark.rs:355).
Every comparison is byte equality of canonical field elements."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

from oracle import pyref as R
from tests import fv_common as C
from tests import r1cs_eval_common as V
from tests import r1cs_sat_common as S
from tests import spartan_common as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(nmx):
    from nova_amd import _lib
    return _lib.lib()


def register(fid, mats):
    from nova_amd import fieldvec as fv
    return [fv.SparseMatrix(fid, ip, ix, dt, cols) for (ip, ix, dt), cols in mats]


def close(ms):
    for m in ms:
        m.close()


def evaluate(ms, rxv, ryv, mont=False):
    from nova_amd import fieldvec as fv
    return [int.from_bytes(b, "little") for b in fv.r1cs_evaluate(ms, rxv, ryv, mont=mont)]


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", sorted(C.FIELDS))
@pytest.mark.parametrize("k", [1, 3, 8])
def test_small_sizes_against_the_restatement(nmx, L, fid, k):
    p = C.FIELDS[fid]
    shapes = [(1000, 600), (700, 300), (1024, 1024), (97, 83), (513, 257), (256, 1000), (300, 17), (64, 64)][:k]
    csr = [V.classes_csr(fid, r, c, seed=100 * k + 10 * j + fid) for j, (r, c) in enumerate(shapes)]
    ms = register(fid, [(m, c) for m, (_r, c) in zip(csr, shapes)])
    try:
        for ell_x, ell_y, seed in ((10, 10, 1), (12, 11, 2)):
            rx, rxv = V.point(fid, ell_x, 1000 + seed + fid)
            ry, ryv = V.point(fid, ell_y, 2000 + seed + fid)
            want = V.restate(p, csr, rx, ry)
            got = evaluate(ms, rxv, ryv)
            print(fid, k, ell_x, ell_y, "canonical", got == want)
            assert got == want
            got = evaluate(ms, V.to_mont_point(fid, rxv), V.to_mont_point(fid, ryv), mont=True)
            assert got == V.mont_ints(p, want)
    finally:
        close(ms)


# ---- 2. 2^14 and 2^20 against both composed identities -------------------------------------------------------------------------------
@pytest.mark.parametrize("fid,ell", [(1, 14), (0, 14), (3, 14), (1, 20), (0, 20)])
def test_large_sizes_against_both_composed_identities(nmx, L, fid, ell):
    import bench
    from nova_amd import fieldvec as fv
    n = 1 << ell
    csr = bench.spartan_like_matrices(fid, n, seed=900 + ell)   # num_cons = num_vars = n, columns [0, n + 2) of 2 n
    ms = register(fid, [(m, 2 * n) for m in csr])
    try:
        _, rxv = V.point(fid, ell, 31 + fid)
        _, ryv = V.point(fid, ell + 1, 32 + fid)
        for mont in (False, True):
            px, py = (V.to_mont_point(fid, rxv), V.to_mont_point(fid, ryv)) if mont else (rxv, ryv)
            got = fv.r1cs_evaluate(ms, px, py, mont=mont)
            T_y = fv.eq_evals_from_points(fid, py, mont=mont, device=True)
            fwd = fv.mle_multi_evaluate(fid, fv.multiply_vec_many(ms, T_y, mont=mont), px, mont=mont)
            T_x = fv.eq_evals_from_points(fid, px, mont=mont, device=True)
            bwd = fv.mle_multi_evaluate(fid, fv.multiply_vec_many(ms, T_x, transposed=True, mont=mont), py, mont=mont)
            print(fid, ell, "mont" if mont else "canonical", [g.hex()[:16] for g in got], got == fwd, got == bwd)
            assert got == fwd, "M~(r_x, r_y) != mle_evaluate(M T_y, r_x)"
            assert got == bwd, "M~(r_x, r_y) != mle_evaluate(M^T T_x, r_y)"
            assert len(set(got)) == 3 and all(any(g) for g in got)
            del T_x, T_y
    finally:
        close(ms)


# ---- 3. edge cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_edge_shapes_and_points(nmx, L, fid):
    p = C.FIELDS[fid]
    one = (np.array([0, 1], np.uint64), np.array([0], np.uint64), C.vec([p - 2]))
    empty = (np.zeros(38, np.uint64), np.zeros(0, np.uint64), np.zeros((0, 32), np.uint8))
    body = V.classes_csr(fid, 37, 21, seed=3 + fid)
    heavy = SC.heavy_column_csr(fid, 3000, 500, seed=4 + fid)   # the constant-one column: an entry in every row
    cases = [([(one, 1)], 0, 0), ([(one, 1)], 3, 0), ([(one, 1)], 0, 2),                 # 1 x 1; ell_x = 0 or ell_y = 0
             ([(empty, 21), (body, 21)], 6, 5),                                           # no entries: 0
             ([(heavy, 500)], 12, 9),
             ([(body, 21), (heavy, 500), (one, 1), (empty, 21)], 13, 10)]                 # different shapes in one call
    for mats, ell_x, ell_y in cases:
        ms = register(fid, mats)
        try:
            rx, rxv = V.point(fid, ell_x, 11 + fid)
            ry, ryv = V.point(fid, ell_y, 12 + fid)
            csr = [m for m, _c in mats]
            want = V.restate(p, csr, rx, ry)
            assert evaluate(ms, rxv, ryv) == want, (ell_x, ell_y)
            assert evaluate(ms, V.to_mont_point(fid, rxv), V.to_mont_point(fid, ryv), mont=True) == V.mont_ints(p, want)
            for j, m in enumerate(csr):
                if m is empty:
                    assert want[j] == 0
            # coordinates 0 and 1: eq collapses to a single row / column
            for zx, zy in ((0, 1), (1, 0)):
                if ell_x < 2 or ell_y < 2:
                    continue
                rx2, ry2 = list(rx), list(ry)
                rx2[ell_x - 1], rx2[ell_x - 2], ry2[ell_y - 1], ry2[0] = zx, 1 - zx, zy, 0
                assert evaluate(ms, C.vec(rx2), C.vec(ry2)) == V.restate(p, csr, rx2, ry2)
            if ell_x >= 6 and ell_y >= 5 and len(mats) == 2:   # every coordinate 0 or 1: the entries of one cell, summed
                bx, by = [0, 1, 0, 0, 1, 0], [1, 0, 0, 1, 1]    # row 18, column 19
                ip, ix, dt = body
                cell = sum(v for k, v in zip(range(int(ip[18]), int(ip[19])), C.ints(dt)[int(ip[18]):int(ip[19])]) if int(ix[k]) == 19) % p
                assert evaluate(ms, C.vec(bx), C.vec(by)) == [0, cell]
        finally:
            close(ms)


# ---- 4. errors: nothing is written ---------------------------------------------------------------------------------------------------
def raw(L, handles, rxv, ell_x, ryv, ell_y, flags=0):
    hs = (ctypes.c_uint64 * len(handles))(*handles)
    buf = np.full(32 * len(handles) + 32, 0x5a, np.uint8)
    rc = L.nmx_r1cs_evaluate(hs, len(handles), rxv.ctypes.data, ell_x, ryv.ctypes.data, ell_y, flags, buf.ctypes.data)
    return rc, bool((buf == 0x5a).all())


def test_shape_and_handle_errors_write_nothing(nmx, L):
    from nova_amd import _lib
    fid = 1
    ms = register(fid, [(V.classes_csr(fid, 37, 21, seed=1), 21), (V.classes_csr(fid, 64, 32, seed=2), 32)])
    try:
        hs = [m.handle for m in ms]
        _, pts = V.point(fid, 8, 5)
        assert raw(L, hs, pts, 6, pts, 5)[0] == 0
        assert raw(L, hs, pts, 5, pts, 5) == (_lib.E_ARG, True)          # 37 and 64 rows > 2^5
        msg = L.nmx_last_error()
        assert b"matrix 0" in msg and b"37 rows" in msg and b"32" in msg
        assert raw(L, hs[1:], pts, 5, pts, 5) == (_lib.E_ARG, True) and b"64 rows" in L.nmx_last_error()
        assert raw(L, hs, pts, 6, pts, 4) == (_lib.E_ARG, True)          # 21 and 32 columns > 2^4
        msg = L.nmx_last_error()
        assert b"matrix 0" in msg and b"21 columns" in msg and b"16" in msg
        assert raw(L, [hs[1], hs[0]], pts, 6, pts, 4) == (_lib.E_ARG, True) and b"32 columns" in L.nmx_last_error()
        assert raw(L, hs + [0xdeadbeef], pts, 6, pts, 5) == (_lib.E_HANDLE, True)
        other = register(0, [(V.classes_csr(0, 37, 21, seed=1), 21)])
        try:
            assert raw(L, hs + [other[0].handle], pts, 6, pts, 5) == (_lib.E_ARG, True)   # mixed fields
        finally:
            close(other)
        big = np.full((8, 32), 0xff, np.uint8)                                            # a coordinate >= the modulus
        assert raw(L, hs, big, 6, pts, 5) == (_lib.E_SCALAR_RANGE, True)
        assert raw(L, hs, pts, 6, big, 5) == (_lib.E_SCALAR_RANGE, True)
        gone = hs[0]
        ms[0].close()
        assert raw(L, [gone], pts, 6, pts, 5) == (_lib.E_HANDLE, True)                   # unregistered
    finally:
        close(ms)


# ---- 5. the transposed form is not built ---------------------------------------------------------------------------------------------
def test_no_transposed_form_is_built(nmx, L):
    """free device memory through the runtime's own query (hipMemGetInfo): unchanged by the call on a fresh registration once the
    workspace exists, and lower after the first transposed product of the same matrix -- which shows the query sees such a build"""
    import torch
    from nova_amd import fieldvec as fv
    fid, ell = 1, 16
    n = 1 << ell
    import bench
    csr = bench.spartan_like_matrices(fid, n, seed=77)
    warm = register(fid, [(m, 2 * n) for m in csr])
    _, rxv = V.point(fid, ell, 1)
    _, ryv = V.point(fid, ell + 1, 2)
    try:
        want = fv.r1cs_evaluate(warm, rxv, ryv)   # the context's workspace is allocated here
        T_x = fv.eq_evals_from_points(fid, rxv, device=True)
    finally:
        close(warm)
    ms = register(fid, [(m, 2 * n) for m in csr])   # fresh: nothing has asked for M^T
    try:
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        for _ in range(3):
            assert fv.r1cs_evaluate(ms, rxv, ryv) == want
        after = torch.cuda.mem_get_info()[0]
        nnz = sum(len(m[1]) for m in csr)
        print("free before / after the calls:", before, after, "nnz", nnz)
        assert before - after < 4 * nnz, "the call allocated device memory of the order of a transposed form"
        outs = fv.multiply_vec_many(ms, T_x, transposed=True)
        torch.cuda.synchronize()
        built = torch.cuda.mem_get_info()[0]
        print("free after the first transposed product:", built)
        assert after - built >= 4 * nnz
        assert fv.r1cs_evaluate(ms, rxv, ryv) == want
        del outs
    finally:
        close(ms)


# ---- 6. threads, ordering --------------------------------------------------------------------------------------------------------------
def test_three_threads_on_shared_matrices(nmx, L):
    from nova_amd import fieldvec as fv
    fid = 3
    p = C.FIELDS[fid]
    shapes = [(5000, 3000), (4096, 4096), (3000, 5000)]
    csr = [V.classes_csr(fid, r, c, seed=50 + j) for j, (r, c) in enumerate(shapes)]
    ms = register(fid, [(m, c) for m, (_r, c) in zip(csr, shapes)])
    try:
        pts = [(V.point(fid, 13, 60 + t), V.point(fid, 13, 70 + t)) for t in range(3)]
        want = [V.restate(p, csr, rx[0], ry[0]) for rx, ry in pts]
        got, errs = [None] * 3, []

        def work(t):
            try:
                for _ in range(20):
                    got[t] = evaluate(ms, pts[t][0][1], pts[t][1][1])
                    assert got[t] == want[t]
            except Exception as e:  # noqa: BLE001
                errs.append((t, repr(e)))

        th = [threading.Thread(target=work, args=(t,)) for t in range(3)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errs, errs
        assert got == want
        assert [int.from_bytes(b, "little") for b in fv.r1cs_evaluate(ms[::-1], pts[0][0][1], pts[0][1][1])] == want[0][::-1]
    finally:
        close(ms)


def test_is_ordered_behind_an_async_call_of_the_same_thread(nmx, L):
    """an NMX_ASYNC fold of 2^22 elements is still running when the evaluation is issued; the evaluation's answer is unaffected and,
    once it has returned, the asynchronous call's output is complete (a synchronous call completes the thread's asynchronous ones)"""
    import torch
    from nova_amd import fieldvec as fv
    fid = 1
    p = C.FIELDS[fid]
    csr = [V.classes_csr(fid, 3000, 2000, seed=5)]
    ms = register(fid, [(csr[0], 2000)])
    try:
        rx, rxv = V.point(fid, 12, 1)
        ry, ryv = V.point(fid, 11, 2)
        want = V.restate(p, csr, rx, ry)
        n = 1 << 22
        a = torch.from_numpy(np.tile(C.rand_vec(fid, 1 << 12, 3), (n >> 12, 1)).copy()).cuda()
        b = torch.from_numpy(np.tile(C.rand_vec(fid, 1 << 12, 4), (n >> 12, 1)).copy()).cuda()
        r = C.rand_vec(fid, 1, 6)
        torch.cuda.synchronize()
        ref = fv.axpy(fid, a, b, r)
        for _ in range(3):
            out = fv.axpy(fid, a, b, r, async_=True)
            assert evaluate(ms, rxv, ryv) == want      # no sync in between
            assert torch.equal(out, ref)
    finally:
        close(ms)


# ---- 7. the equation the call exists for (snark.rs:355) --------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", [0, 1])
def test_inner_sumcheck_final_claim_equals_the_evaluations_times_eval_Z(nmx, L, fid):
    """The inner sum-check of RelaxedR1CSSNARK::prove (snark.rs:175-215) on a satisfied instance: claim = Az(r_x) + r Bz(r_x) +
    r^2 Cz(r_x) over poly_ABC(y) = (A^T T_x + r B^T T_x + r^2 C^T T_x)[y] and z, proved by nmx_sumcheck_prove_quad_prod under the
    stand-in transcript; the verifier's side of snark.rs:355: its final claim == (eA + r eB + r^2 eC) * z~(r_y)."""
    from nova_amd import fieldvec as fv
    p = C.FIELDS[fid]
    rows, cols, ell_x, ell_y = 97, 83, 7, 7
    inst = S.make_relaxed(fid, rows, cols, seed=40 + fid)
    assert inst.bad_rows()[0] == 0
    rx, rxv = V.point(fid, ell_x, 41)
    r = C.ints(C.rand_vec(fid, 1, 42))[0]
    T_x = R.eq_evals(p, rx)
    z = C.ints(inst.z()) + [0] * ((1 << ell_y) - cols)
    tables = [SC.dense_transposed(p, ip, ix, dt, cols, C.vec(T_x[:rows])) + [0] * ((1 << ell_y) - cols) for ip, ix, dt in inst.csr]
    abc = [(a + r * b + r * r * c) % p for a, b, c in zip(*tables)]
    az, bz, cz = inst.products()
    claim = sum(T_x[i] * (az[i] + r * bz[i] + r * r * cz[i]) for i in range(rows)) % p   # snark.rs:175-178
    assert claim == sum(x * y for x, y in zip(abc, z)) % p
    tr = SC.StandInTranscript(p)
    import torch
    d_abc, d_z = (torch.from_numpy(C.vec(v).copy()).cuda() for v in (abc, z))
    torch.cuda.synchronize()
    polys, rs, _claims = fv.sumcheck_prove_quad_prod(fid, SC.le(claim), ell_y, d_abc, d_z, tr)
    polys_i = [[int.from_bytes(c, "little") for c in row] for row in polys]
    ry = [int.from_bytes(x, "little") for x in rs]
    assert ry == tr.rs
    claim_inner_final = SC.verify_rounds(p, claim, polys_i, ry, 2)
    ms = register(fid, [(m, cols) for m in inst.csr])
    try:
        eA, eB, eC = evaluate(ms, rxv, C.vec(ry))
    finally:
        close(ms)
    eval_Z = SC.mle_eval(p, z, ry)
    assert claim_inner_final == (eA + r * eB + r * r * eC) % p * eval_Z % p, "snark.rs:355"
    assert [eA, eB, eC] == V.restate(p, inst.csr, rx, ry)


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_on_gpu(nmx):
    from tests import test_r1cs_evaluate_abi as A
    b = A.BIN if os.path.exists(A.BIN) else A.build_cpp()
    r = subprocess.run([b], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "r1cs_eval mirror ok" in r.stdout
