"""Fixtures for the dense field-vector maps and the three sum passes at their value and lane edges (nova_amd/csrc/fieldvec_maps.hpp:
AxpyFn, Axpy2Fn, CrossTermFn, CrossTerm2Fn, VecAddFn, BindTopFn, FoldPairFn, LinCombFn; nova_amd/csrc/sumcheck_sums.hpp: the lane bodies
of k_eq_sums / k_eq_rows, k_bind_eq_sums, k_plain_sums), shared by tests/test_fieldvec_edges.py (CPU) and
tests/test_gpu_fieldvec_edges.py (GPU).  Everything is deterministic and every expectation is Python big integers.

What a WORD means: a vector is 32-byte words.  A kernel reads a word w as the residue w mod p whatever w is.  In the canonical layout
the word's value is that residue; in the Montgomery layout a stored word w stands for the value w * 2^-256 mod p.  Every expectation
here converts words to values, evaluates the reference's formula over values, and converts the result back to a word (value * 2^256
mod p in the Montgomery layout) -- so the linear operations act on the words as they are and a product of two words carries one 2^-256.
A challenge is given as a VALUE; challenge_word() is what the call is handed."""
import functools
import itertools
import random

from tests import fv_common as C

M256 = (1 << 256) - 1


def EDGE(p):
    return [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, (1 << 256) % p]


def NONCANON(p):
    return [p, p + 1, 2 * p + 5, M256]


def _keep_order(p):
    """EDGE in the order in which values are kept when a grid is trimmed: 0, 1, p - 1, p - 2, (p - 1) / 2 always stay"""
    return [0, 1, p - 1, p - 2, (p - 1) // 2, (1 << 256) % p, (p + 1) // 2, 2]


GRID_MAX_ROWS = 8192


def grid_values(p, k, noncanon=False):
    """the values one operand of a k-operand map takes: EDGE (trimmed for k = 5 so that the grid stays below GRID_MAX_ROWS rows), or
    {0, p - 1} and the words >= p"""
    if noncanon:
        vals = [0, p - 1] + NONCANON(p)
    else:
        vals = _keep_order(p)
    while len(vals) ** k >= GRID_MAX_ROWS:
        vals = vals[:-1]
    return vals


@functools.lru_cache(maxsize=None)
def grid(fid, k, noncanon=False):
    """k columns (tuples of words) that enumerate the Cartesian product of grid_values: row i holds the i-th tuple, first operand
    slowest"""
    vals = grid_values(C.FIELDS[fid], k, noncanon)
    rows = list(itertools.product(vals, repeat=k))
    return tuple(tuple(r[j] for r in rows) for j in range(k))


def grid_row_name(fid, k, noncanon, row):
    vals = grid_values(C.FIELDS[fid], k, noncanon)
    return "(" + ", ".join("%#x" % v for v in list(itertools.product(vals, repeat=k))[row]) + ")"


def challenges(fid):
    """challenge VALUES: 0, 1, p - 1, p - 2 and one random value"""
    p = C.FIELDS[fid]
    return [0, 1, p - 1, p - 2, random.Random(0xC4A1 + fid).randrange(p)]


def challenge_word(p, c, mont):
    return (c << 256) % p if mont else c


def _rinv(p, mont):
    return pow(1 << 256, -1, p) if mont else 1


def values(p, words, mont):
    k = _rinv(p, mont)
    return [w * k % p for w in words]


def words_of(p, vals, mont):
    R = (1 << 256) % p if mont else 1
    return [v * R % p for v in vals]


# ---- the maps: name -> (operands, takes a challenge, formula over values) --------------------------------------------------------------
MAPS = {
    "axpy": (2, True, lambda p, v, r: v[0] + r * v[1]),
    "axpy2": (3, True, lambda p, v, r: v[0] + r * v[1] + r * r * v[2]),
    "cross_term": (4, True, lambda p, v, u: v[0] * v[1] - u * v[2] - v[3]),
    "cross_term2": (5, True, lambda p, v, u: v[0] * v[1] - u * v[2] - v[3] - v[4]),
    "vec_add": (2, False, lambda p, v, r: v[0] + v[1]),
    "bind": (2, True, lambda p, v, r: v[0] + r * (v[1] - v[0])),   # (lo, hi)
}


def expect_map(name, fid, cols, c, mont):
    """the output words of map `name` over the operand columns `cols` (words) with challenge value c"""
    p = C.FIELDS[fid]
    k, _has, fn = MAPS[name]
    assert len(cols) == k
    ri, R = _rinv(p, mont), (1 << 256) % p if mont else 1
    memo = {}   # (the uniform tables repeat a handful of rows)
    out = []
    for row in zip(*cols):
        if row not in memo:
            memo[row] = fn(p, [w * ri % p for w in row], c) % p * R % p
        out.append(memo[row])
    return out


def bind_top_input(lo, hi):
    """bind_poly_var_top's vector for the columns (lo, hi): the low half, then the high half"""
    return list(lo) + list(hi)


def fold_pairs_input(lo, hi):
    """fold_pairs' vector: P[2j] = lo[j], P[2j + 1] = hi[j]"""
    out = []
    for a, b in zip(lo, hi):
        out += [a, b]
    return out


def expect_fold_chain(fid, words, cs, mont):
    """HyperKZG's fold loop: [fold(words, cs[0]), fold(that, cs[1]), ...] as lists of words"""
    outs, cur = [], list(words)
    for c in cs:
        cur = expect_map("bind", fid, (cur[0::2], cur[1::2]), c, mont)
        outs.append(cur)
    return outs


def shape_columns(fid, k, n, noncanon):
    """k columns of n words for the length tests: the grid's rows in turn (n may exceed or fall short of the grid)"""
    g = grid(fid, k, noncanon)
    rows = len(g[0])
    # a stride coprime to the grid size, so that short lengths still meet mixed tuples
    return tuple([col[(i * 37 + 11) % rows] for i in range(n)] for col in g)


# ---- the linear combination ------------------------------------------------------------------------------------------------------------
LINCOMB_KS = (1, 4, 5, 23, 24, 25, 28, 29, 48, 49)   # LinCombFn reduces after six groups of four vectors: 24 vectors
LINCOMB_N_OUT = 300
_LINCOMB_LENS = (300, 1, 255, 256, 257, 299, 64)


def lincomb_weights(p):
    """the values s whose powers are the weights"""
    return [p - 1, p - 2, (p - 1) // 2, 2]


def lincomb_vectors(fid, k, fill):
    """k ragged vectors of words: fill 'p-1' (every word p - 1) or 'max' (every word 2^256 - 1)"""
    p = C.FIELDS[fid]
    w = p - 1 if fill == "p-1" else M256
    return [[w] * _LINCOMB_LENS[j % len(_LINCOMB_LENS)] for j in range(k)]


def expect_lincomb(fid, vecs, s, n_out, mont):
    """sum_j s^j * v_j, shorter vectors zero-padded (linear: the weights are values, the words go in as they are)"""
    p = C.FIELDS[fid]
    out = [0] * n_out
    w = 1
    for v in vecs:
        for i, x in enumerate(v):
            out[i] += w * (x % p)
        w = w * s % p
    return [x % p for x in out]


# ---- table patterns of the sum passes ---------------------------------------------------------------------------------------------------
TABLE_PATTERNS = ("all_pm1", "lo0_hi_pm1", "lo_pm1_hi0", "all_max", "lo0_hi_max", "lo_max_hi0", "edge_vectors")
EQ_PATTERNS = ("pm1", "random", "max")
# (table pattern, eq pattern): every table pattern under the all-(p - 1) eq tables, then random eq tables and eq tables of words >= p
SUM_CASES = tuple((t, "pm1") for t in TABLE_PATTERNS) + (("edge_vectors", "random"), ("all_pm1", "random"), ("all_max", "max"))


def _two_values(p, pattern):
    big = M256 if "max" in pattern else p - 1
    if pattern.startswith("all_"):
        return big, big
    return (0, big) if pattern.startswith("lo0_") else (big, 0)


@functools.lru_cache(maxsize=None)
def table(fid, pattern, n, which=0, quarters=False):
    """a table of n words (n even).  The uniform patterns hold value u in the low half and v in the high half; with quarters=True
    (the bind pass: n a multiple of 4) the quarters hold (u, v, v, u), so that both binds of a lane see the two values in both orders.
    which = 0, 1, 2 (A, B, C): C holds the halves swapped; edge_vectors draws a different seed per table."""
    p = C.FIELDS[fid]
    if pattern == "edge_vectors":
        return tuple(C.ints(C.edge_vectors(fid, n, 61 + 7 * which + fid)))
    u, v = _two_values(p, pattern)
    if which == 2:
        u, v = v, u
    if quarters:
        q = n // 4
        return tuple([u] * q + [v] * q + [v] * q + [u] * q)
    return tuple([u] * (n // 2) + [v] * (n - n // 2))


@functools.lru_cache(maxsize=None)
def eq_table(fid, pattern, n, seed=0):
    p = C.FIELDS[fid]
    if pattern == "pm1":
        return (p - 1,) * n
    if pattern == "max":
        return (M256,) * n
    return tuple(C.ints(C.rand_vec(fid, n, 97 + seed + fid)))


def eq_factor(p, eqL, eqR, shift, i):
    return eqR[i] if eqL is None else eqL[i >> shift] * eqR[i & ((1 << shift) - 1)] % p


def eq_sums_values(p, mode, A, B, C_, eqL, eqR, shift):
    """(t_0, t_inf) over VALUES: EqSumCheckInstance's evaluation points (the header of nova_amd/csrc/sumcheck.hip)"""
    h = len(A) // 2
    t0 = t1 = 0
    memo = {}   # (the uniform tables repeat a handful of index tuples)
    for i in range(h):
        key = (A[i], A[i + h], B[i] if mode >= 2 else 0, B[i + h] if mode >= 2 else 0, C_[i] if mode == 3 else 0,
               eqR[i] if eqL is None else eqR[i & ((1 << shift) - 1)], 0 if eqL is None else eqL[i >> shift])
        if key not in memo:
            f = eq_factor(p, eqL, eqR, shift, i)
            if mode == 1:
                memo[key] = (A[i] * f % p, 0)
            else:
                memo[key] = ((A[i] * B[i] - (C_[i] if mode == 3 else 1)) * f % p, (A[i + h] - A[i]) * (B[i + h] - B[i]) % p * f % p)
        t0 += memo[key][0]
        t1 += memo[key][1]
    return t0 % p, t1 % p


def expect_eq_sums(fid, mode, A, B, C_, eqR, eqL, shift, mont):
    """the two output words of nmx_sumcheck_eq_sums (mode 1: the second is zero)"""
    p = C.FIELDS[fid]
    v = lambda x: None if x is None else values(p, x, mont)   # noqa: E731
    return tuple(words_of(p, eq_sums_values(p, mode, v(A), v(B), v(C_), v(eqL), v(eqR), shift), mont))


def expect_bind_top(fid, X, c, mont):
    n = len(X)
    return expect_map("bind", fid, (X[:n // 2], X[n // 2:]), c, mont)


def expect_bind_eq_sums(fid, mode, A, B, C_, c, eqR, eqL, shift, mont):
    """nmx_sumcheck_bind_eq_sums: the bound tables (words, len / 2 each; None for a table the mode does not use) and the next round's sums"""
    bound = [None if (X is None or m > mode) else expect_bind_top(fid, X, c, mont) for m, X in ((1, A), (2, B), (3, C_))]
    return bound, expect_eq_sums(fid, mode, bound[0], bound[1], bound[2], eqR, eqL, shift, mont)


def plain_sums_values(p, kind, A, B, C_):
    h = len(A) // 2
    s = [0, 0, 0]
    memo = {}   # (the uniform tables repeat a handful of index tuples)
    for i in range(h):
        a0, a1, b0, b1 = A[i], A[i + h], B[i], B[i + h]
        c0, c1 = (C_[i], C_[i + h]) if kind == 4 else (0, 0)
        key = (a0, a1, b0, b1, c0, c1)
        if key not in memo:
            if kind == 1:
                t = (a0 * b0, (a1 - a0) * (b1 - b0), 0)
            elif kind == 2:
                t = (a0 - b0, (2 * a0 - a1) - (2 * b0 - b1), 0)
            elif kind == 3:
                t = (a0 * b0, (2 * a0 - a1) * (2 * b0 - b1), 0)
            else:
                t = (a0 * b0 * c0, (a1 - a0) * (b1 - b0) * (c1 - c0), (2 * a0 - a1) * (2 * b0 - b1) * (2 * c0 - c1))
            memo[key] = tuple(x % p for x in t)
        for j in range(3):
            s[j] += memo[key][j]
    return [x % p for x in s][:3 if kind == 4 else 2]


def expect_plain_sums(fid, kind, A, B, C_, mont):
    p = C.FIELDS[fid]
    v = lambda x: None if x is None else values(p, x, mont)   # noqa: E731
    return tuple(words_of(p, plain_sums_values(p, kind, v(A), v(B), v(C_)), mont))


def is_canonical_case(tpat, epat):
    return "max" not in tpat and epat != "max"
