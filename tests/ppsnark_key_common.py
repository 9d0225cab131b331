"""The definitions behind nmx_ppsnark_spark_repr and nmx_masked_eq_evals in Python integers, shared by the CPU tests
(tests/test_ppsnark_key_abi.py), the GPU tests (tests/test_gpu_ppsnark_key.py) and smoke():
  spark_size / spark_repr     R1CSShapeSparkRepr::new                       src/spartan/ppsnark.rs:117-190 (N: :118-121)
  masked_eq_table             MaskedEqPolynomial::evals                     src/spartan/polys/masked_eq.rs:57-75
  masked_eq_evaluate          MaskedEqPolynomial::evaluate                  src/spartan/polys/masked_eq.rs:34-52
  identity_evaluate           IdentityPolynomial::evaluate                  src/spartan/polys/identity.rs:22-33
  final_claim_expected        claim_sc_inner_batched_expected of verify     src/spartan/ppsnark.rs:1496-1598
and the shapes the tests of the key tables share.  A matrix is (indptr, indices, values) in plain integers, CSR, entry e = storage index e
(the order of SparseMatrix::iter, src/r1cs/sparse.rs:332-390).  Everything is exact."""
import random

import numpy as np

from tests import fv_common as fc
from tests.batched_cubic_common import eq_table
from tests.spartan_common import eq_eval, mle_eval

R256 = 1 << 256
ROW_COUNTS = [1, 2, 63, 64, 65, 257, 1000]


def spark_size(nnzs, num_vars, num_cons):
    """ppsnark.rs:118-121: max(total_nz, 2 num_vars, num_cons).next_power_of_two()"""
    m = max(sum(nnzs), 2 * num_vars, num_cons, 1)
    return 1 << (m - 1).bit_length()


def spark_repr(mats, n):
    """-> (row, col, vals [one list per matrix], ts_row, ts_col), every list n integers (ppsnark.rs:123-167)"""
    row, col = [0] * n, [n - 1] * n
    vals = [[0] * n for _ in mats]
    i = 0
    for j, (indptr, indices, values) in enumerate(mats):
        for r in range(len(indptr) - 1):
            for e in range(int(indptr[r]), int(indptr[r + 1])):
                row[i], col[i], vals[j][i] = r, int(indices[e]), int(values[e])
                i += 1
    assert i <= n
    ts_row, ts_col = [0] * n, [0] * n
    for a in row:
        ts_row[a] += 1
    for a in col:
        ts_col[a] += 1
    return row, col, vals, ts_row, ts_col


def to_form(p, v, mont):
    return [x * R256 % p for x in v] if mont else [x % p for x in v]


def masked_eq_table(p, r, m):
    t = eq_table(p, list(r)) if len(r) else [1]
    return [0 if i < (1 << m) else t[i] for i in range(len(t))]


def masked_eq_evaluate(p, r, m, rx):
    split = len(r) - m
    eq_lo, eq_hi = eq_eval(p, r[:split], rx[:split]), eq_eval(p, r[split:], rx[split:])
    mask_lo = 1
    for a, b in zip(r[:split], rx[:split]):
        mask_lo = mask_lo * ((1 - a) * (1 - b) % p) % p
    return (eq_lo - mask_lo) * eq_hi % p


def identity_evaluate(p, rx):
    return sum(x << (len(rx) - 1 - i) for i, x in enumerate(rx)) % p


def final_claim_expected(p, ev, rho, r_outer_full, r_inner, log_num_vars, u_X, gamma, r, c, coeffs):
    """ppsnark.rs:1496-1598.  ev: the fifteen evaluations at r_inner by the reference's names (eval_row, eval_col, eval_L_row, eval_L_col,
    eval_val_A, eval_val_B, eval_val_C, eval_E, eval_W, eval_t_plus_r_inv_row, eval_w_plus_r_inv_row, eval_ts_row, and the three _col
    ones); u_X: the public IO [u] + X."""
    ell = len(r_inner)
    rand_eq = eq_eval(p, rho, r_inner)
    eq_ro = eq_eval(p, r_outer_full, r_inner)
    masked = masked_eq_evaluate(p, r_outer_full, log_num_vars, r_inner)
    ident = identity_evaluate(p, r_inner)
    t_row = (ident + gamma * eq_ro + r) % p
    w_row = (ev["eval_row"] + gamma * ev["eval_L_row"] + r) % p
    pad = ell - (log_num_vars + 1)                                            # N.log_2() - (2 num_vars).log_2()  (:1528)
    factor = 1
    for x in r_inner[:pad]:
        factor = factor * (1 - x) % p
    unpad = r_inner[pad:]
    # SparsePolynomial::new(len - 1, X).evaluate(unpad[1:]): the MLE of X padded with zeros -- an explicit small table stands in (:1540-1550)
    xt = list(u_X) + [0] * ((1 << (len(unpad) - 1)) - len(u_X))
    eval_X = mle_eval(p, xt, unpad[1:])
    eval_Z = (ev["eval_W"] + factor * unpad[0] * eval_X) % p
    t_col = (ident + gamma * eval_Z + r) % p
    w_col = (ev["eval_col"] + gamma * ev["eval_L_col"] + r) % p
    mem = (coeffs[0] * (ev["eval_t_plus_r_inv_row"] - ev["eval_w_plus_r_inv_row"]) + coeffs[1] * (ev["eval_t_plus_r_inv_col"] - ev["eval_w_plus_r_inv_col"])
           + coeffs[2] * rand_eq * (ev["eval_t_plus_r_inv_row"] * t_row - ev["eval_ts_row"]) + coeffs[3] * rand_eq * (ev["eval_w_plus_r_inv_row"] * w_row - 1)
           + coeffs[4] * rand_eq * (ev["eval_t_plus_r_inv_col"] * t_col - ev["eval_ts_col"]) + coeffs[5] * rand_eq * (ev["eval_w_plus_r_inv_col"] * w_col - 1))
    abc = coeffs[6] * ev["eval_L_row"] * ev["eval_L_col"] * (ev["eval_val_A"] + c * ev["eval_val_B"] + c * c * ev["eval_val_C"])
    return (mem + abc + coeffs[7] * eq_ro * ev["eval_E"] + coeffs[8] * masked * ev["eval_W"]) % p


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------------
def ints_of(indptr, indices, data):
    return [int(x) for x in indptr], [int(x) for x in indices], fc.ints(data)


def random_mat(p, rows, cols, seed, empty_rows=(), per_row=3, nnz_exact=None):
    """random CSR: 0 .. per_row entries per row, the rows in empty_rows none; values mixed 1, p - 1, small, general, 0.  nnz_exact: entries are
    added to (or taken from) the last non-empty-listed rows until the matrix holds exactly that many."""
    rng = random.Random(seed)
    counts = [0 if r in empty_rows else rng.randrange(per_row + 1) for r in range(rows)]
    if nnz_exact is not None:
        free = [r for r in range(rows) if r not in empty_rows] or [0]
        if nnz_exact:
            counts[free[0]] = max(counts[free[0]], 1)                         # the first listed row keeps an entry
        t = 0
        while sum(counts) < nnz_exact:
            counts[free[t % len(free)]] += 1
            t += 1
        while sum(counts) > nnz_exact:
            r = max(range(rows), key=lambda q: (counts[q], q))
            counts[r] -= 1
    indptr = [0]
    for c in counts:
        indptr.append(indptr[-1] + c)
    nnz = indptr[-1]
    indices = [rng.randrange(cols) for _ in range(nnz)]
    pool = [1, p - 1, 2, 7, p - 2, p - 7, 8, p - 8, 0]
    values = [rng.choice(pool) if rng.random() < 0.5 else rng.randrange(p) for _ in range(nnz)]
    return indptr, indices, values


def shape_cases(fid, k):
    """[(name, mats, n)] -- the shapes of the issue's A.3 for k matrices over field fid (values as integers)"""
    from tests import spartan_common as sc
    p = fc.FIELDS[fid]
    out = []
    for rows in ROW_COUNTS:
        empty = {0, 1, rows - 1} if rows >= 4 else ({rows - 1} if rows == 2 else set())      # leading rows and the last row hold nothing
        mats = [random_mat(p, rows, max(rows // 2, 1) + j, 100 * rows + j + fid, empty_rows=empty) for j in range(k)]
        out.append(("rows%d" % rows, mats, spark_size([len(m[1]) for m in mats], 1, rows + k)))
    # total == n and total == n - 1 (no padding, one padding element), cols == n with entries in column n - 1 and in row 0
    for name, short in (("full", 0), ("full-1", 1)):
        n = 256
        per = [(n - short) // k + (1 if j < (n - short) % k else 0) for j in range(k)]
        mats = []
        for j in range(k):
            ip, ix, vs = random_mat(p, 40, n, 7 + j + fid, nnz_exact=per[j], empty_rows={39})
            if ix:
                ix[0], ix[-1] = n - 1, n - 1
            mats.append((ip, ix, vs))
        out.append((name, mats, n))
    # nothing at all: one row, one column, no entry, n == 1
    out.append(("empty", [([0, 0], [], []) for _ in range(k)], 1))
    # a column with an entry in every row of every matrix
    mats = [ints_of(*sc.heavy_column_csr(fid, 300, 200, 50 + j + fid)) for j in range(k)]
    out.append(("heavy", mats, spark_size([len(m[1]) for m in mats], 1, 300)))
    # more distinct columns in one block's tile (2048 entries) than its table holds (1024 slots): every entry a column of its own
    per = 4096 // k
    mats = []
    for j in range(k):
        ip = [0] + [min(per, 5 * (r + 1)) for r in range((per + 4) // 5)]
        mats.append((ip, [(per * j + e) % 4096 for e in range(per)], [(e + j) % 9 for e in range(per)]))
    out.append(("distinct", mats, 4096))
    return out


def mixed_coefficient_mats(fid, k):
    """the values of fv_common.mixed_coefficient_case: 1, p - 1, small, general"""
    ip, ix, dt, cols, _z, _z2, _o, _o2 = fc.mixed_coefficient_case(fid)
    m = ints_of(ip, ix, dt)
    return [m] * k, spark_size([len(m[1])] * k, cols, len(m[0]) - 1)


def to_numpy(mat):
    ip, ix, vs = mat
    return np.array(ip, np.uint64), np.array(ix, np.uint64), (fc.vec(vs).copy() if vs else np.zeros((0, 32), np.uint8))
