"""The yardstick of nmx_r1cs_evaluate: RelaxedR1CSSNARK::verify's multi_evaluate (src/spartan/snark.rs:325-353) restated with Python
big integers --
    evals[i] = sum over every entry (row, col, val) of M_i of T_x[row] * T_y[col] * val,
    T_x = oracle.pyref.eq_evals(r_x), T_y = oracle.pyref.eq_evals(r_y)
-- and the matrix sets the CPU and GPU tests share.  tests/test_r1cs_evaluate_abi.py checks this restatement itself against
oracle.pyref.spmv + oracle.pyref.mle_evaluate through M~(r_x, r_y) = mle_evaluate(M T_y, r_x)."""
import numpy as np

from oracle import pyref as R
from tests import fv_common as C
from tests import util


def restate(p, mats, r_x, r_y):
    """mats: (indptr, indices, data) triples, data (nnz, 32) bytes or a list of ints; r_x, r_y: lists of ints.  -> list of ints"""
    T_x, T_y = R.eq_evals(p, list(r_x)), R.eq_evals(p, list(r_y))
    out = []
    for ip, ix, dt in mats:
        d = dt if (isinstance(dt, list) and (not dt or isinstance(dt[0], int))) else C.ints(dt)
        acc = 0
        for row in range(len(ip) - 1):
            for k in range(int(ip[row]), int(ip[row + 1])):
                acc += T_x[row] * T_y[int(ix[k])] * d[k]  # (T_x[row_idx], T_y[col_idx]: an IndexError here is the reference's panic)
        out.append(acc % p)
    return out


def restate_via_products(p, mats, rows_pow2, r_x, r_y):
    """the same through oracle.pyref.spmv and oracle.pyref.mle_evaluate: (M T_y) zero-padded to 2^ell_x rows, evaluated at r_x"""
    T_y = R.eq_evals(p, list(r_y))
    out = []
    for ip, ix, dt in mats:
        mz = R.spmv(p, [int(x) for x in ip], [int(x) for x in ix], C.ints(dt), T_y)
        out.append(R.mle_evaluate(p, mz + [0] * (rows_pow2 - len(mz)), list(r_x)))
    return out


def point(fid, ell, seed):
    """ell random field elements as (ints, (ell, 32) bytes)"""
    v = C.rand_vec(fid, max(ell, 1), seed)[:ell].copy()
    return (C.ints(v) if ell else []), v


def classes_csr(fid, rows, cols, seed, empty_every=5):
    """rows x cols CSR that exercises every coefficient class (+1, -1, +-2..7, general, and a stored zero), has empty rows (every
    `empty_every`-th), one row of 40 entries and entries in the last row and the last column"""
    p = C.FIELDS[fid]
    rng = np.random.Generator(np.random.PCG64(seed))
    counts = rng.integers(1, 7, size=rows)
    counts[::empty_every] = 0
    counts[rows // 2] = 40
    counts[rows - 1] = 3
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    nnz = int(indptr[-1])
    indices = rng.integers(0, cols, size=nnz).astype(np.uint64)
    indices[nnz - 1] = cols - 1
    data = C.rand_vec(fid, nnz, seed + 1).copy()
    special = [1, p - 1] + list(range(2, 8)) + [p - k for k in range(2, 8)] + [0, 8, p - 8]
    kind = rng.integers(0, 3, size=nnz)
    for k in range(nnz):
        if kind[k] < 2:  # two thirds of the entries are small, as in an R1CS matrix
            data[k] = util.int_to_le32(special[(k * 7 + seed) % len(special)])
    return indptr, indices, data


def to_mont_point(fid, v):
    return util.to_mont_scalars(C.CURVE_WITH_SCALAR_FIELD[fid], v) if len(v) else v


def mont_ints(p, vals):
    return [x * (1 << 256) % p for x in vals]
