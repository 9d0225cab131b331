"""Instances for the satisfiability check (nmx_r1cs_is_sat; R1CSShape::is_sat / is_sat_relaxed, src/r1cs/mod.rs:474-574), made the way
bench.py makes its Spartan instance: for any A, B, C (tests/fv_common.random_csr: +-1, small and zero coefficients, one 40-entry row),
any W, X, u define E := Az o Bz - u Cz -- satisfied by construction.  Strict form: random A, B and a C with one entry per row in the
constant column (col = num_vars, where z holds 1) whose value is (Az o Bz)[row].  The expected answers come from oracle.cref.spmv,
oracle.pyref.cross_term and oracle.cref.commit; tests/test_r1cs_sat_abi.py checks this builder itself on the CPU."""
import numpy as np

from oracle import cref
from oracle import pyref as R
from tests import fv_common as C
from tests import util


class Instance:
    """A, B, C as (indptr, indices, data) CSR triples over field `fid`; W (n_w, 32), X (n_io, 32), u (1, 32) / E (rows, 32) or None."""

    def __init__(self, fid, rows, cols, n_io, csr, W, X, u=None, E=None):
        self.fid, self.cid, self.p = fid, C.CURVE_WITH_SCALAR_FIELD[fid], C.FIELDS[fid]
        self.rows, self.cols, self.n_io, self.n_w = rows, cols, n_io, cols - 1 - n_io
        self.csr, self.W, self.X, self.u, self.E = csr, W, X, u, E

    @property
    def relaxed(self):
        return self.E is not None

    def copy(self):
        return Instance(self.fid, self.rows, self.cols, self.n_io, self.csr, self.W.copy(), self.X.copy(),
                        None if self.u is None else self.u.copy(), None if self.E is None else self.E.copy())

    def z(self):
        one = C.vec([1]) if self.u is None else self.u.reshape(1, 32)
        return np.concatenate([self.W.reshape(-1, 32), one, self.X.reshape(-1, 32)])

    def products(self):
        """(Az, Bz, Cz) as lists of ints (oracle.cref.spmv)"""
        z = self.z()
        return [C.ints(np.frombuffer(cref.spmv(self.fid, ip, ix, dt, self.rows, z), np.uint8)) for ip, ix, dt in self.csr]

    def residual(self):
        """Az o Bz - u Cz - E per row (oracle.pyref.cross_term); the strict form is u = 1, E = 0"""
        az, bz, cz = self.products()
        e = C.ints(self.E) if self.relaxed else [0] * self.rows
        u = C.ints(self.u)[0] if self.relaxed else 1
        return R.cross_term(self.p, az, bz, cz, e, u)

    def bad_rows(self):
        """(number of violated rows, the lowest one or 2^64 - 1) according to the oracle residual"""
        bad = [i for i, t in enumerate(self.residual()) if t]
        return len(bad), (bad[0] if bad else 2 ** 64 - 1)


def make_relaxed(fid, rows, cols, n_io=2, seed=1):
    csr = [C.random_csr(fid, rows, cols, seed + 10 * j) for j in range(3)]
    n_w = cols - 1 - n_io
    inst = Instance(fid, rows, cols, n_io, csr, C.rand_vec(fid, n_w, seed + 100).copy(), C.rand_vec(fid, n_io, seed + 101).copy(),
                    u=C.rand_vec(fid, 1, seed + 102).copy(), E=np.zeros((rows, 32), np.uint8))
    inst.E = C.vec(inst.residual())  # E := Az o Bz - u Cz
    return inst


def make_strict(fid, rows, cols, n_io=2, seed=1):
    n_w = cols - 1 - n_io
    A, B = (C.random_csr(fid, rows, cols, seed + 10 * j) for j in range(2))
    empty = (np.zeros(rows + 1, np.uint64), np.zeros(0, np.uint64), np.zeros((0, 32), np.uint8))
    inst = Instance(fid, rows, cols, n_io, [A, B, empty], C.rand_vec(fid, n_w, seed + 100).copy(), C.rand_vec(fid, n_io, seed + 101).copy())
    az, bz, _cz = inst.products()
    p = inst.p
    inst.csr[2] = (np.arange(rows + 1, dtype=np.uint64), np.full(rows, n_w, np.uint64), C.vec([a * b % p for a, b in zip(az, bz)]))
    return inst


# ---- corruptions: each changes a VALUE, never a shape ------------------------------------------------------------------------
def bump(v, j, delta, p):
    """v[j] += delta (mod p), in place"""
    v[j] = util.int_to_le32((C.ints(v[j])[0] + delta) % p)


def corrupt_E_plus_one(inst, j):
    out = inst.copy()
    bump(out.E, j, 1, inst.p)
    return out


def corrupt_E_minus_one(inst, j):
    out = inst.copy()
    bump(out.E, j, inst.p - 1, inst.p)
    return out


def corrupt_W(inst, k):
    out = inst.copy()
    bump(out.W, k, 1, inst.p)
    return out


def corrupt_u(inst):
    out = inst.copy()
    bump(out.u, 0, 1, inst.p)
    return out


def column_of_row(inst, j):
    """a witness column (< n_w) that row j of A reads, or None"""
    ip, ix, _dt = inst.csr[0]
    for k in range(int(ip[j]), int(ip[j + 1])):
        if int(ix[k]) < inst.n_w:
            return int(ix[k])
    return None


# ---- the commitment half -------------------------------------------------------------------------------------------------------
def key_points(inst, k0=7):
    """(ck bases (n, 64), h (64 bytes)) long enough for W and E: P_i = (k0 + i) G, h = P_n"""
    curve = [c for c in R.CURVES.values() if c.cid == inst.cid][0]
    n = max(inst.n_w, inst.rows)
    pts = cref.sequential_bases(curve, k0, n + 1)
    return pts[:n], pts[n].tobytes()


def expected_commitments(inst, bases, h, r_W, r_E=None):
    """((xy64, is_inf) of W, the same of E or None) from oracle.cref.commit"""
    cw = cref.commit(inst.cid, inst.W, bases[:inst.n_w], inst.n_w, h, r_W)
    ce = cref.commit(inst.cid, inst.E, bases[:inst.rows], inst.rows, h, r_E) if inst.relaxed else None
    return cw, ce


def to_mont(inst):
    """the same instance with W, X, u, E as Montgomery limbs (x * 2^256 mod p); the matrices are registered as they are"""
    m = lambda v: None if v is None else util.to_mont_scalars(inst.cid, v)
    return Instance(inst.fid, inst.rows, inst.cols, inst.n_io, inst.csr, m(inst.W), m(inst.X), m(inst.u), m(inst.E))
