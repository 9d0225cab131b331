"""Fixtures for the sparse-matrix kernels at their class, operand and column-split edges (nova_amd/csrc/spmv_row.hpp: spmv_row /
spmv_small_term; fieldvec.hip: SpmvFn, SpmvPairFn, SpmvSegFn + k_spmv_heavy, SpmvCrossFn, k_r1cs_sat; capi.hip: transposed_of), shared
by tests/test_spmv_edges.py (CPU) and tests/test_gpu_spmv_edges.py (GPU).  Everything is deterministic.  The yardstick is Python big
integers -- oracle.pyref.spmv, oracle.pyref.cross_term and the dense restatement of the transposed product below -- never the code
under test.

What an operand WORD means: a gathered vector is 32-byte words; a kernel reads a word w as the residue w mod p whatever w is
(spmv_row.hpp: "z is any 256-bit value"), so every expectation here is taken over `w % p`.  In the canonical layout a word is the
value itself.  In the Montgomery layout a canonical value v travels as v * 2^256 mod p and a matrix registered with mont=True
multiplies words by the canonical coefficient, so the expectation is linear in the words in both layouts:
    out_word[row] = sum_k c_k * (w_k mod p) mod p          (c_k the canonical coefficient)."""
import functools
import random

import numpy as np

from oracle import pyref as R
from tests import fv_common as C

NONCANON_FROM = 11   # ZVALS(p)[:NONCANON_FROM] are < p, the rest are words >= p
P_MINUS_1_COL = 3    # ZVALS(p)[3] == p - 1
ALL_ONES_COL = 14    # ZVALS(p)[14] == 2^256 - 1


def coefficient_class(p, v):
    """SpmvClassifyFn (nova_amd/csrc/fieldvec.hip): 0 general, 1 +1, 2 -1, 3..8 +2..+7, 9..14 -2..-7"""
    if v == 1:
        return 1
    if 2 <= v <= 7:
        return v + 1
    if p - v == 1:
        return 2
    if 2 <= p - v <= 7:
        return p - v + 7
    return 0


def COEFFS(p):
    """every class, its neighbours (0, 8, p - 8: general) and general values of every size"""
    return ([0] + list(range(1, 8)) + [8] + [p - k for k in range(1, 8)] + [p - 8, (p - 1) // 2, (p + 1) // 2, 1 << 253,
            random.Random(0xC0EF).randrange(p)])


def ZVALS(p):
    """operand words: eleven canonical values, then the four words >= p of test_horner_outputs_are_canonical_for_any_input_words"""
    canon = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, (1 << 29) - 1, 1 << 29, 1 << 232, random.Random(0x2A).randrange(p)]
    assert len(canon) == NONCANON_FROM and all(v < p for v in canon)
    return canon + [p, p + 1, 2 * p + 5, (1 << 256) - 1]


class Csr:
    """a CSR matrix with its coefficients as Python integers (.coeffs) and as (nnz, 32) bytes (.data)"""

    def __init__(self, fid, rows, cols, indptr, indices, coeffs, name):
        self.fid, self.p, self.rows, self.cols, self.name = fid, C.FIELDS[fid], rows, cols, name
        self.indptr, self.indices = np.asarray(indptr, np.uint64), np.asarray(indices, np.uint64)
        self.coeffs = [int(c) for c in coeffs]
        assert len(self.indptr) == rows + 1 and int(self.indptr[-1]) == len(self.coeffs) == len(self.indices)
        assert all(0 <= c < self.p for c in self.coeffs) and (not len(self.indices) or int(self.indices.max()) < cols)
        self.data = C.vec(self.coeffs) if self.coeffs else np.zeros((0, 32), np.uint8)

    @property
    def triple(self):
        return self.indptr, self.indices, self.data

    def classes(self):
        return {coefficient_class(self.p, c) for c in self.coeffs}

    def column_lengths(self):
        return np.bincount(self.indices.astype(np.int64), minlength=self.cols).tolist()

    def times(self, words):
        """M w over the residues of the words: oracle.pyref.spmv"""
        assert len(words) == self.cols
        return R.spmv(self.p, [int(x) for x in self.indptr], [int(x) for x in self.indices], self.coeffs, [w % self.p for w in words])

    def transposed_times(self, words):
        """M^T w, dense restatement (as tests/spartan_common.dense_transposed): out[col] += w[row] * c for every entry"""
        assert len(words) == self.rows
        p, out = self.p, [0] * self.cols
        ip, ix = [int(x) for x in self.indptr], [int(x) for x in self.indices]
        for r in range(self.rows):
            w = words[r] % p
            for k in range(ip[r], ip[r + 1]):
                out[ix[k]] += w * self.coeffs[k]
        return [x % p for x in out]

    def transpose(self, name):
        """the same entries as the CSR of M^T (entries of a row of M^T in the order of M's rows)"""
        ip, ix = [int(x) for x in self.indptr], [int(x) for x in self.indices]
        ent = sorted((ix[k], r, self.coeffs[k]) for r in range(self.rows) for k in range(ip[r], ip[r + 1]))
        cnt = np.bincount([e[0] for e in ent], minlength=self.cols) if ent else np.zeros(self.cols, np.int64)
        return Csr(self.fid, self.cols, self.rows, np.concatenate([[0], np.cumsum(cnt)]), [e[1] for e in ent], [e[2] for e in ent], name)


def mont_words(p, words):
    """canonical values as Montgomery words; a word >= p has no Montgomery preimage and travels as it is"""
    return [(w << 256) % p if w < p else w for w in words]


# ---- grid: one row per (coefficient, operand word) ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_csr(fid, canonical_only=False):
    """row i * |Z| + j holds the single entry (column j, COEFFS[i]); gathered with ZVALS as the vector, row i * |Z| + j is
    COEFFS[i] * ZVALS[j], so a failing row names the pair.  canonical_only: the columns of the values < p alone."""
    p = C.FIELDS[fid]
    nz = NONCANON_FROM if canonical_only else len(ZVALS(p))
    co = COEFFS(p)
    rows = len(co) * nz
    return Csr(fid, rows, nz, np.arange(rows + 1), [r % nz for r in range(rows)], [co[r // nz] for r in range(rows)],
               "grid" + ("_canonical" if canonical_only else ""))


def grid_z(fid, canonical_only=False):
    z = ZVALS(C.FIELDS[fid])
    return z[:NONCANON_FROM] if canonical_only else z


def grid_pair_name(fid, row, canonical_only=False):
    p = C.FIELDS[fid]
    nz = NONCANON_FROM if canonical_only else len(ZVALS(p))
    return "coefficient COEFFS[%d] = %#x (class %d), word ZVALS[%d] = %#x" % (row // nz, COEFFS(p)[row // nz], coefficient_class(p, COEFFS(p)[row // nz]),
                                                                            row % nz, ZVALS(p)[row % nz])


@functools.lru_cache(maxsize=None)
def grid_T(fid):
    """the transpose of grid_csr as CSR: |Z| rows, every column one entry long"""
    return grid_csr(fid).transpose("grid_T")


# ---- pileup: row lengths either side of every multiple of six, worst-case terms -----------------------------------------------------
PILEUP_LENGTHS = (1, 2, 5, 6, 7, 11, 12, 13, 18, 19, 40, 100)
PILEUP_FILLS = ("+7", "-7", "-1", "general p-8", "-7 / general")


def pileup_fill(p, kind, n):
    g = p - 8
    return {"+7": [7] * n, "-7": [p - 7] * n, "-1": [p - 1] * n, "general p-8": [g] * n,
            "-7 / general": [p - 7 if k % 2 == 0 else g for k in range(n)]}[kind]


@functools.lru_cache(maxsize=None)
def pileup_csr(fid, col=P_MINUS_1_COL, cols=None, rows=None):
    """row r has PILEUP_LENGTHS[(r // 5) % 12] entries of fill PILEUP_FILLS[r % 5], ALL at column `col` (duplicate (row, column)
    entries).  With ZVALS as the vector col = P_MINUS_1_COL gathers p - 1 and col = ALL_ONES_COL gathers 2^256 - 1: the same entries
    pointed at the other operand.  rows beyond 60 repeat the pattern, cols beyond col + 1 are never gathered."""
    p = C.FIELDS[fid]
    cols = len(ZVALS(p)) if cols is None else cols
    rows = len(PILEUP_LENGTHS) * len(PILEUP_FILLS) if rows is None else rows
    counts, coeffs = [], []
    for r in range(rows):
        n = PILEUP_LENGTHS[(r // len(PILEUP_FILLS)) % len(PILEUP_LENGTHS)]
        counts.append(n)
        coeffs += pileup_fill(p, PILEUP_FILLS[r % len(PILEUP_FILLS)], n)
    return Csr(fid, rows, cols, np.concatenate([[0], np.cumsum(counts)]), [col] * len(coeffs), coeffs, "pileup_col%d" % col)


def pileup_row_name(row):
    return "%d entries, fill %s" % (PILEUP_LENGTHS[(row // len(PILEUP_FILLS)) % len(PILEUP_LENGTHS)], PILEUP_FILLS[row % len(PILEUP_FILLS)])


# ---- column lengths around the transposed form's cut ---------------------------------------------------------------------------------
COLUMN_ROWS = 32768
# transposed_of (capi.hip) cuts a column longer than 32 entries into chunks of 16; k_spmv_heavy adds a column's partials with 256 lanes,
# reducing each lane's sum after six: 4096 / 4097 entries are 256 / 257 partials, 24576 / 24577 are 1536 / 1537 (six / seven per lane),
# 32768 are 2048.  A long column first, one last, and long ones side by side.
COLUMN_LENGTHS = (32768, 0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 4096, 24576, 24577, 4097)
COLUMN_VARIANTS = ("minus_one", "general", "classes", "max_partials")


@functools.lru_cache(maxsize=None)
def _column_pattern():
    rr = np.concatenate([np.arange(n, dtype=np.int64) for n in COLUMN_LENGTHS])
    cc = np.concatenate([np.full(n, j, np.int64) for j, n in enumerate(COLUMN_LENGTHS)])
    order = np.lexsort((cc, rr))
    rr, cc = rr[order], cc[order]
    return np.concatenate([[0], np.cumsum(np.bincount(rr, minlength=COLUMN_ROWS))]), cc


@functools.lru_cache(maxsize=None)
def column_lengths_csr(fid, variant):
    """COLUMN_ROWS x 16, column j with entries in rows 0 .. COLUMN_LENGTHS[j] - 1 (about 9 * 10^4 entries).  Variants:
    minus_one     every coefficient p - 1 (x all p - 1: the negative branch on the largest operand, every term);
    general       random general coefficients with 0, 1, p - 1, p - 2, 2 sprinkled in (fv_common.edge_vectors);
    classes       COEFFS in turn, so every class meets every chunk position;
    max_partials  every coefficient +1 (x = p - 1 on every 16th row, 0 elsewhere: every full chunk's partial is p - 1, the largest
                  value k_spmv_heavy can be handed, 1536 / 1537 / 2048 times over)."""
    p = C.FIELDS[fid]
    indptr, indices = _column_pattern()
    nnz = len(indices)
    if variant == "minus_one":
        coeffs = [p - 1] * nnz
    elif variant == "general":
        coeffs = C.ints(C.edge_vectors(fid, nnz, 11 + fid))
    elif variant == "classes":
        co = COEFFS(p)
        coeffs = [co[k % len(co)] for k in range(nnz)]
    else:
        assert variant == "max_partials"
        coeffs = [1] * nnz
    return Csr(fid, COLUMN_ROWS, len(COLUMN_LENGTHS), indptr, indices, coeffs, "columns_" + variant)


@functools.lru_cache(maxsize=None)
def column_x(fid, variant):
    """the vector over the ROWS that goes with a variant (canonical values), as a tuple of ints"""
    p = C.FIELDS[fid]
    if variant == "minus_one":
        return (p - 1,) * COLUMN_ROWS
    if variant == "max_partials":
        return tuple(p - 1 if r % 16 == 0 else 0 for r in range(COLUMN_ROWS))
    return tuple(C.ints(C.edge_vectors(fid, COLUMN_ROWS, 23 + fid)))   # general and classes share one x (multiply_vec_many)


@functools.lru_cache(maxsize=None)
def column_z(fid):
    """a vector over the 16 COLUMNS for the forward product: edge values, then random ones"""
    p = C.FIELDS[fid]
    return tuple([0, 1, p - 1, p - 2, 2] + C.ints(C.rand_vec(fid, len(COLUMN_LENGTHS) - 5, 31 + fid)))


@functools.lru_cache(maxsize=None)
def column_expect_transposed(fid, variant, x_variant=None):
    """M^T x, computed once per field and variant (about 10^5 big-integer products)"""
    return tuple(column_lengths_csr(fid, variant).transposed_times(column_x(fid, x_variant or variant)))


@functools.lru_cache(maxsize=None)
def column_expect_forward(fid, variant):
    return tuple(column_lengths_csr(fid, variant).times(column_z(fid)))


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape_csrs(fid):
    """rows 1, 255, 256, 257 (either side of the 256-lane block) with COEFFS in turn, a matrix without entries, and one whose rows
    are all empty but the last"""
    p = C.FIELDS[fid]
    co = COEFFS(p)
    out = []
    for rows in (1, 255, 256, 257):
        cols = 19
        rng = np.random.Generator(np.random.PCG64(100 * rows + fid))
        counts = rng.integers(0, 8, size=rows)
        counts[rows - 1] = 7
        nnz = int(counts.sum())
        indices = rng.integers(0, cols, size=nnz)
        indices[nnz - 1] = cols - 1
        out.append(Csr(fid, rows, cols, np.concatenate([[0], np.cumsum(counts)]), indices, [co[(k + rows) % len(co)] for k in range(nnz)], "rows%d" % rows))
    out.append(Csr(fid, 5, 3, np.zeros(6, np.uint64), [], [], "nnz0"))
    out.append(Csr(fid, 257, 19, [0] * 257 + [9], [0, 18, 3, 3, 7, 1, 2, 18, 0], [1, p - 1, 7, p - 7, p - 8, 0, 2, p - 2, co[-1]], "last_row_only"))
    return tuple(out)


def shape_words(fid, n, seed):
    """n operand words: ZVALS (the words >= p included) in turn among random values"""
    p = C.FIELDS[fid]
    z = ZVALS(p)
    rnd = C.ints(C.rand_vec(fid, n, seed))
    return [z[i // 2 % len(z)] if i % 2 == 0 else rnd[i] for i in range(n)]


def canonical_fixtures(fid):
    """(matrix, vector over its columns) for every fixture, canonical values only: what the C oracle is pinned on"""
    p = C.FIELDS[fid]
    zc = grid_z(fid, True)
    out = [(grid_csr(fid, True), zc), (grid_csr(fid, True).transpose("grid_T_canonical"), C.ints(C.edge_vectors(fid, grid_csr(fid, True).rows, 5 + fid))),
           (pileup_csr(fid, P_MINUS_1_COL, NONCANON_FROM), zc)]
    out += [(column_lengths_csr(fid, v), list(column_z(fid))) for v in COLUMN_VARIANTS]
    out += [(m, [w % p for w in shape_words(fid, m.cols, 41 + fid)]) for m in shape_csrs(fid)]
    return out
