"""nmx_ppsnark_spark_repr / nmx_masked_eq_evals on the GPU, byte for byte against the definitions in Python integers
(tests/ppsnark_key_common.py; the kernels alone run on the CPU in tests/test_ppsnark_key_abi.py): all four fields, both output forms,
matrices registered in canonical and in Montgomery form, host and HBM outputs, k = 1, 3 and 8, the shapes of the CPU test plus one of 2^12
rows at n = 2^14; NULL outputs; the matrices untouched; the refusals that need a registered matrix; the masked eq table against
nmx_eq_evals_from_points; and ppsnark's prove from three matrix handles to the end of prove_helper chained in HBM, accepted by the
reference's verifier equations (tests/ppsnark_sc_common.check_honest and ppsnark_key_common.final_claim_expected)."""
import ctypes
import random

import numpy as np
import pytest

from tests import fv_common as fc
from tests import ppsnark_key_common as kc
from tests import ppsnark_sc_common as pc
from tests.spartan_common import verify_rounds

pytestmark = pytest.mark.gpu
SENT = 0xA5


@pytest.fixture(scope="module")
def L(nmx):
    from nova_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def fv(nmx):
    from nova_amd import fieldvec
    return fieldvec


def gpu(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def err_code(fn):
    from nova_amd.provider import NmxError
    with pytest.raises(NmxError) as e:
        fn()
    return e.value.code, str(e.value)


def register(fv, fid, mats, reg_mont):
    p = fc.FIELDS[fid]
    out = []
    for ip, ix, vs in mats:
        ipn, ixn, dt = kc.to_numpy((ip, ix, kc.to_form(p, vs, reg_mont)))
        out.append(fv.SparseMatrix(fid, ipn, ixn, dt, max(list(ix) + [0]) + 1, mont=reg_mont))
    return out


def close_all(ms):
    for m in ms:
        m.close()


def expect_bytes(p, mats, n, mont):
    row, col, vals, ts_row, ts_col = kc.spark_repr(mats, n)
    assert sum(ts_row) == n and sum(ts_col) == n
    f = lambda v: fc.vec(kc.to_form(p, v, mont))  # noqa: E731
    return [f(row), f(col)] + [f(v) for v in vals] + [f(ts_row), f(ts_col)]


def flat(res):
    row, col, vals, ts_row, ts_col = res
    return [host(row), host(col)] + [host(v) for v in vals] + [host(ts_row), host(ts_col)]


def check_all_forms(fv, fid, mats, n, name):
    """registered in both forms x both output forms x host and HBM outputs, against ONE computation of the definition"""
    p = fc.FIELDS[fid]
    want = {mont: expect_bytes(p, mats, n, mont) for mont in (False, True)}
    for reg_mont in (False, True):
        ms = register(fv, fid, mats, reg_mont)
        try:
            for mont in (False, True):
                for device in (True, False):
                    got = flat(fv.ppsnark_spark_repr(ms, n, mont=mont, device=device))
                    for j, (g, w) in enumerate(zip(got, want[mont])):
                        assert (g == w).all(), (name, reg_mont, mont, device, j)
        finally:
            close_all(ms)


# ---- the Spark representation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
@pytest.mark.parametrize("k", [1, 3, 8])
def test_spark_repr_shapes(fv, fid, k):
    for name, mats, n in kc.shape_cases(fid, k):
        check_all_forms(fv, fid, mats, n, name)


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
def test_spark_repr_mixed_coefficients(fv, fid):
    for k in (1, 3):
        mats, n = kc.mixed_coefficient_mats(fid, k)
        check_all_forms(fv, fid, mats, n, "mixed")


def big_case(fid, k):
    """2^12 rows, n = 2^14: several blocks of every pass, several tiles of the histogram, and one column with an entry in every row"""
    p = fc.FIELDS[fid]
    mats = []
    for j in range(k):
        ip, ix, vs = kc.random_mat(p, 1 << 12, 1 << 12, 900 + j + fid, per_row=2, nnz_exact=(5000 if k == 3 else 9000))
        for r in range(1 << 12):
            if ip[r] < ip[r + 1]:
                ix[ip[r]] = 7
        mats.append((ip, ix, vs))
    return mats, 1 << 14


@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
@pytest.mark.parametrize("k", [1, 3])
def test_spark_repr_4096_rows(fv, fid, k):
    p = fc.FIELDS[fid]
    mats, n = big_case(fid, k)
    mont = bool(fid & 1)
    want = expect_bytes(p, mats, n, mont)
    ms = register(fv, fid, mats, not mont)
    try:
        for device in (True, False):
            for j, (g, w) in enumerate(zip(flat(fv.ppsnark_spark_repr(ms, n, mont=mont, device=device)), want)):
                assert (g == w).all(), (device, j)
    finally:
        close_all(ms)


def raw_call(L, ms, n, flags, row, col, vals, ts_row, ts_col):
    k = len(ms)
    hs = (ctypes.c_uint64 * 8)(*([m.handle for m in ms] + [0] * (8 - k)))
    v = None if vals is None else (ctypes.c_void_p * 8)(*(list(vals) + [None] * (8 - len(vals))))
    return L.nmx_ppsnark_spark_repr(hs, k, n, flags, row, col, v, ts_row, ts_col)


@pytest.mark.parametrize("device", [False, True])
def test_null_outputs_are_skipped_the_others_unchanged_and_the_matrices_untouched(fv, L, device):
    from nova_amd import _lib
    fid = 1
    p = fc.FIELDS[fid]
    _name, mats, n = kc.shape_cases(fid, 3)[5]                       # 257 rows
    want = expect_bytes(p, mats, n, False)
    ms = register(fv, fid, mats, False)
    try:
        z = [gpu(fc.rand_vec(fid, m.cols, 3 + j)) for j, m in enumerate(ms)]
        before = [host(m.multiply_vec(zz)) for m, zz in zip(ms, z)]
        flags = _lib.SCALARS_DEVICE if device else 0
        for null in ((0,), (1, 5), (2, 3, 4), (3,), (0, 1, 2, 4, 5, 6), (6,), (0, 1, 2, 3, 4, 5)):
            bufs = [np.full((n, 32), SENT, np.uint8) for _ in range(7)]
            if device:
                bufs = [gpu(b) for b in bufs]
            ptr = [None if j in null else (b.data_ptr() if device else b.ctypes.data) for j, b in enumerate(bufs)]
            vals = None if null == (2, 3, 4) else ptr[2:5]
            assert raw_call(L, ms, n, flags, ptr[0], ptr[1], vals, ptr[5], ptr[6]) == 0, L.nmx_last_error()
            for j, b in enumerate(bufs):
                assert (host(b) == (SENT if j in null else want[j])).all(), (null, j)
        assert raw_call(L, ms, n, flags, None, None, None, None, None) == 0
        after = [host(m.multiply_vec(zz)) for m, zz in zip(ms, z)]
        assert all((a == b).all() for a, b in zip(before, after)), "the matrices give the same products after the call as before"
    finally:
        close_all(ms)


def test_refusals_leave_the_buffers_untouched_and_the_next_call_works(fv, L):
    from nova_amd import _lib
    fid = 1
    p = fc.FIELDS[fid]
    mats = [kc.random_mat(p, 40, 60, 21 + j, nnz_exact=50) for j in range(3)]        # total 150, rows 40, columns up to 60
    for m in mats:
        m[1][0] = 59
    n = 256
    ms = register(fv, fid, mats, False)
    other = register(fv, 2, [kc.random_mat(fc.FIELDS[2], 8, 8, 5)], False)
    wide = register(fv, fid, [([0, 1], [299], [1])], False)                            # one row, 300 columns
    tall = register(fv, fid, [([0] * 300 + [1], [0], [1])], False)                     # 300 rows, one column
    try:
        bufs = [gpu(np.full((n, 32), SENT, np.uint8)) for _ in range(7)]
        D = _lib.SCALARS_DEVICE

        def call(mm=ms, n_=n, flags=D, shift=None):
            ptr = [b.data_ptr() for b in bufs]
            if shift is not None:
                ptr[shift[0]] = ptr[shift[1]] + 32 * shift[2]
            vals = (ptr[2:5] + [ptr[2]] * 8)[:len(mm)] if len(mm) <= 3 else None
            return raw_call(L, mm, n_, flags, ptr[0], ptr[1], vals, ptr[5], ptr[6])
        A = _lib.E_ARG
        assert call(n_=255) == A and call(n_=384) == A and b"power of two" in L.nmx_last_error()
        assert call(n_=128) == A and b"150 entries > n = 128" in L.nmx_last_error()
        assert call(mm=tall, n_=256) == A and b"300 rows > n = 256" in L.nmx_last_error()
        assert call(mm=wide, n_=256) == A and b"300 columns > n = 256" in L.nmx_last_error()
        assert call(n_=32) == A                                                        # below rows, columns and entries at once
        assert call(mm=[ms[0], other[0], ms[2]]) == A and b"different fields" in L.nmx_last_error()
        closed = register(fv, fid, mats[:1], False)[0]
        gone = closed.handle
        closed.close()
        closed.handle = gone
        assert call(mm=[ms[0], closed]) == _lib.E_HANDLE
        closed.handle = 0
        assert call(shift=(1, 0, n - 1)) == A and b"overlap" in L.nmx_last_error()      # col starts on row's last element
        assert call(shift=(6, 4, 1)) == A and call(shift=(3, 2, 0)) == A               # ts_col over a value vector; two value vectors as one
        for fl in (_lib.ASYNC | D, _lib.BASES_MONT | D, 1 << 20):
            assert call(flags=fl) == A, fl
        assert all((host(b) == SENT).all() for b in bufs), "a refused call wrote something"
        assert call() == 0                                                             # the next call on the thread succeeds
        for b, w in zip(bufs, expect_bytes(p, mats, n, False)):
            assert (host(b) == w).all()
    finally:
        close_all(ms + other + wide + tall)


# ---- the masked eq table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", sorted(fc.FIELDS))
@pytest.mark.parametrize("ell", [0, 1, 5, 10, 14])
def test_masked_eq_evals(fv, fid, ell):
    p = fc.FIELDS[fid]
    rng = random.Random(77 * fid + ell)
    r = [rng.randrange(p) for _ in range(ell)]
    for mont in (False, True):
        rw = fc.vec(kc.to_form(p, r, mont)).copy() if ell else np.zeros((0, 32), np.uint8)
        eq = host(fv.eq_evals_from_points(fid, rw, mont=mont))
        for m in sorted({0, 1, ell - 1, ell} & set(range(ell + 1))):
            for device in (False, True):
                got = host(fv.masked_eq_evals(fid, rw, m, mont=mont, device=device))
                assert got.shape == (1 << ell, 32)
                assert not got[:1 << m].any(), (ell, m, mont, device)
                assert (got[1 << m:] == eq[1 << m:]).all(), (ell, m, mont, device)
                if ell <= 5:                                                            # and the definition itself (masked_eq.rs:65-75: m = 0 masks one entry)
                    assert fc.ints(got) == kc.to_form(p, kc.masked_eq_table(p, r, m), mont)


def test_masked_eq_refusals_write_nothing_and_the_next_call_works(fv, L):
    from nova_amd import _lib
    fid, ell = 1, 6
    p = fc.FIELDS[fid]
    out = gpu(np.full((1 << ell, 32), SENT, np.uint8))
    r = fc.vec([3] * ell).copy()
    bad = fc.vec([3] * (ell - 1) + [p]).copy()
    D = _lib.SCALARS_DEVICE
    assert L.nmx_masked_eq_evals(fid, bad.ctypes.data, ell, 2, D, out.data_ptr()) == _lib.E_SCALAR_RANGE
    assert L.nmx_masked_eq_evals(fid, r.ctypes.data, ell, ell + 1, D, out.data_ptr()) == _lib.E_ARG
    assert L.nmx_masked_eq_evals(7, r.ctypes.data, ell, 2, D, out.data_ptr()) == _lib.E_ARG
    assert L.nmx_masked_eq_evals(fid, r.ctypes.data, ell, 2, D | _lib.ASYNC, out.data_ptr()) == _lib.E_ARG
    assert (host(out) == SENT).all()
    assert L.nmx_masked_eq_evals(fid, r.ctypes.data, ell, 2, D, out.data_ptr()) == 0
    assert fc.ints(host(out)) == kc.masked_eq_table(p, [3] * ell, 2)


# ---- prove, from three matrix handles to the end of prove_helper, in HBM -----------------------------------------------------------------------
@pytest.mark.parametrize("fid", [1, 2])
@pytest.mark.parametrize("shape", [(64, 64, 2, 3), (64, 128, 2, 1)])
def test_prove_chained_in_hbm_from_three_matrix_handles(fv, fid, shape):
    """(num_cons, num_vars, num_io, entries per row): random A, B, C, a random z = [W, u, X] and E = Az o Bz - u Cz, so the relaxed instance
    holds; every challenge from a seeded stand-in.  ppsnark.rs:1056-1246 step by step, every N-sized vector made in HBM; then (a) the
    reference's verifier on the sixteen tables, read back once, and (b) the last round's claim against claim_sc_inner_batched_expected
    (ppsnark.rs:1496-1598) with eval_row, eval_col and eval_val_* from the call's own outputs."""
    num_cons, num_vars, num_io, per_row = shape
    p = fc.FIELDS[fid]
    rng = random.Random(1000 * fid + num_vars + per_row)
    cols = num_vars + 1 + num_io
    mats = []
    for _ in range(3):
        ix = [rng.randrange(cols) for _ in range(num_cons * per_row)]
        vs = [rng.choice([1, p - 1, 2, rng.randrange(p)]) for _ in range(num_cons * per_row)]
        mats.append(([per_row * r for r in range(num_cons + 1)], ix, vs))
    for m in mats:
        m[1][-1] = cols - 1
    N = kc.spark_size([len(m[1]) for m in mats], num_vars, num_cons)
    assert fv.ppsnark_spark_size([len(m[1]) for m in mats], num_vars, num_cons) == N == {3: 1024, 1: 256}[per_row]
    l, lo, lv = N.bit_length() - 1, num_cons.bit_length() - 1, num_vars.bit_length() - 1
    ms = [fv.SparseMatrix(fid, *kc.to_numpy(m), cols) for m in mats]
    try:
        row, col, vals, ts_row, ts_col = fv.ppsnark_spark_repr(ms, N)                                  # the prover key, in HBM
        Wv, u, X = [rng.randrange(p) for _ in range(num_vars)], rng.randrange(p), [rng.randrange(p) for _ in range(num_io)]
        W_d = gpu(fc.vec(Wv))
        z_d = fv.concat(fid, [W_d, fc.vec([u] + X).copy()])                                             # z = [W, u, X] (:1076)
        Az_d, Bz_d, Cz_d = fv.multiply_vec_many(ms, z_d)                                               # (:1079)
        Az, Bz, Cz = (fc.ints(host(x)) for x in (Az_d, Bz_d, Cz_d))
        Ev = [(a * b - u * c) % p for a, b, c in zip(Az, Bz, Cz)]
        E_d = gpu(fc.vec(Ev))
        r_outer = [rng.randrange(p) for _ in range(lo)]                                                # (the outer sum-check's point)
        e_Az, e_Bz, e_Cz, e_E = (int.from_bytes(b, "little") for b in fv.mle_multi_evaluate(fid, [Az_d, Bz_d, Cz_d, E_d], fc.vec(r_outer)))
        r_pad = [rng.randrange(p) for _ in range(l - lo)]                                              # (:1132-1141)
        r_full = r_pad + r_outer
        factor = 1
        for x in r_pad:
            factor = factor * (1 - x) % p
        mem_row = fv.eq_evals_from_points(fid, fc.vec(r_full), device=True)                            # evaluation_oracles (:220-253)
        mem_col = fv.concat(fid, [z_d], n_out=N)
        W_pad, E_pad = fv.concat(fid, [W_d], n_out=N), fv.concat(fid, [E_d], n_out=N)                  # (:1144-1145)
        L_row, L_col = fv.gather(fid, mem_row, row), fv.gather(fid, mem_col, col)
        c, gamma, r = rng.randrange(p), rng.randrange(p), rng.randrange(p)
        val = fv.axpy2(fid, vals[0], vals[1], vals[2], fc.vec([c]))                                    # (:1177-1182)
        orc = fv.ppsnark_mem_oracles(fid, [mem_row, mem_col], [row, col], [L_row, L_col], [ts_row, ts_col], fc.vec([gamma]), fc.vec([r]))
        masked = fv.masked_eq_evals(fid, fc.vec(r_full), lv, device=True)                              # WitnessBoundSumcheck::new (:284-285)
        rho = [rng.randrange(p) for _ in range(l)]
        s = rng.randrange(1, p)
        coeffs = [pow(s, i, p) for i in range(9)]
        T = [None] * pc.NT
        for g in (0, 1):
            T[5 * g + pc.T_ROW], T[5 * g + pc.W_ROW], T[5 * g + pc.TINV_ROW], T[5 * g + pc.WINV_ROW] = orc[g]
        T[pc.TS_ROW], T[pc.TS_COL], T[pc.L_ROW], T[pc.L_COL] = ts_row, ts_col, L_row, L_col
        T[pc.VAL], T[pc.E], T[pc.W], T[pc.MASKED_EQ] = val, E_pad, W_pad, masked
        claims2 = [factor * (e_Az + c * e_Bz + c * c * e_Cz) % p, factor * e_E % p]                    # (:1185, :1189)
        tables_host = [host(t).copy() for t in T]
        inst = pc.Instance(fid, l, tables_host, rho, r_full, claims2, coeffs)

        def prove(fid_, _tables, rhos, r_o, c2, co, tr):
            return fv.sumcheck_prove_ppsnark(fid_, [t.clone() for t in T], rhos, r_o, c2, co, tr)

        polys, rs, finals = pc.check_honest(prove, inst)                                               # (a)
        r_inner = [int.from_bytes(x, "little") for x in rs]
        fin = [int.from_bytes(f, "little") for f in finals]
        e_last = verify_rounds(p, (coeffs[6] * claims2[0] + coeffs[7] * claims2[1]) % p,
                               [[int.from_bytes(x, "little") for x in rowp] for rowp in polys], r_inner, 3)
        key_ev = [int.from_bytes(b, "little") for b in fv.mle_multi_evaluate(fid, [row, col] + vals, fc.vec(r_inner))]
        ev = {"eval_row": key_ev[0], "eval_col": key_ev[1], "eval_val_A": key_ev[2], "eval_val_B": key_ev[3], "eval_val_C": key_ev[4],
              "eval_L_row": fin[pc.L_ROW], "eval_L_col": fin[pc.L_COL], "eval_E": fin[pc.E], "eval_W": fin[pc.W],
              "eval_t_plus_r_inv_row": fin[pc.TINV_ROW], "eval_w_plus_r_inv_row": fin[pc.WINV_ROW], "eval_ts_row": fin[pc.TS_ROW],
              "eval_t_plus_r_inv_col": fin[pc.TINV_COL], "eval_w_plus_r_inv_col": fin[pc.WINV_COL], "eval_ts_col": fin[pc.TS_COL]}
        assert e_last == kc.final_claim_expected(p, ev, rho, r_full, r_inner, lv, [u] + X, gamma, r, c, coeffs), "ppsnark.rs:1496-1598"   # (b)
    finally:
        close_all(ms)
