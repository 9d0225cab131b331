"""Fixtures for the eq tables, the MLE and polynomial evaluations and batch inversion at their edges (nmx_eq_evals_from_points,
nmx_mle_evaluate, nmx_mle_multi_evaluate, nmx_poly_eval_multi, nmx_field_batch_invert; the functors live in
nova_amd/csrc/fieldvec_eval.hpp), shared by tests/test_eval_edges.py (CPU) and tests/test_gpu_eval_edges.py (GPU).  Everything is
deterministic and every expectation is Python big integers.

Words and values are those of tests/fieldvec_edges_common.py: a kernel reads a 32-byte word w of a VECTOR as w mod p whatever w is; in
the Montgomery layout the word stands for the value w * 2^-256 mod p.  A point (challenge) is given here as VALUES; challenge_word()
makes the word the call is handed, which must be below p."""
import functools
import random

from tests import fv_common as C
from tests.fieldvec_edges_common import EDGE, M256, NONCANON, challenge_word, values, words_of  # noqa: F401  (re-exported)

# ---- points -----------------------------------------------------------------------------------------------------------------------------
CHALLENGE_PATTERNS = ("zeros", "ones", "alt01", "alt10", "pm1", "twos", "half", "random")


@functools.lru_cache(maxsize=None)
def point(fid, pattern, ell):
    """a point of ell coordinates, as values; coordinate 0 is the most significant variable"""
    p = C.FIELDS[fid]
    if pattern == "random":
        rng = random.Random(0xE9 + 131 * fid + ell)
        return tuple(rng.randrange(2, p - 1) for _ in range(ell))
    one = {"zeros": lambda i: 0, "ones": lambda i: 1, "alt01": lambda i: i & 1, "alt10": lambda i: 1 - (i & 1), "pm1": lambda i: p - 1,
           "twos": lambda i: 2, "half": lambda i: (p + 1) // 2}[pattern]
    return tuple(one(i) for i in range(ell))


def point_words(fid, r, mont):
    p = C.FIELDS[fid]
    return [challenge_word(p, c, mont) for c in r]


def indicator_index(r):
    """the index at which eq(r, .) is 1 for a point of zeros and ones (None for any other point)"""
    if any(c not in (0, 1) for c in r):
        return None
    idx = 0
    for c in r:
        idx = 2 * idx + c
    return idx


# ---- eq tables --------------------------------------------------------------------------------------------------------------------------
def eq_value(p, r, x):
    """eq(r, x) = prod_i (x_i ? r_i : 1 - r_i), x_0 (the bit of r[0]) the most significant bit of x"""
    ell = len(r)
    acc = 1
    for i in range(ell):
        acc = acc * (r[i] if (x >> (ell - 1 - i)) & 1 else 1 - r[i]) % p
        if acc == 0:
            break
    return acc


@functools.lru_cache(maxsize=128)
def eq_values(fid, r):
    p = C.FIELDS[fid]
    return tuple(eq_value(p, r, x) for x in range(1 << len(r)))


def expect_eq(fid, r, mont):
    """the words of nmx_eq_evals_from_points at the point r (values): by the definition, entry by entry"""
    return words_of(C.FIELDS[fid], eq_values(fid, tuple(r)), mont)


def expect_eq_at(fid, r, indices, mont):
    p = C.FIELDS[fid]
    return words_of(p, [eq_value(p, r, x) for x in indices], mont)


# the 2^24 table: coordinates 0..6 and 12..18 pinned to zeros and ones, the other ten random (neither 0 nor 1)
PINNED = tuple(range(0, 7)) + tuple(range(12, 19))


@functools.lru_cache(maxsize=None)
def pinned_point(fid, ell=24):
    p = C.FIELDS[fid]
    rng = random.Random(0x24 + fid)
    r = [rng.randrange(2, p - 1) for _ in range(ell)]
    for k, i in enumerate(PINNED):
        r[i] = (0x2B5D >> k) & 1   # 0b10101101011101: both bits, runs of one, two and three
    return tuple(r)


def pinned_support(r):
    """the indices at which eq(r, .) can be non-zero: the bits of the 0/1 coordinates agree with them"""
    ell = len(r)
    free = [i for i in range(ell) if r[i] not in (0, 1)]
    base = sum(r[i] << (ell - 1 - i) for i in range(ell) if r[i] in (0, 1))
    out = []
    for m in range(1 << len(free)):
        x = base
        for k, i in enumerate(free):
            if (m >> k) & 1:
                x |= 1 << (ell - 1 - i)
        out.append(x)
    return sorted(out)


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
OPERAND_PATTERNS = ("pm1", "max", "edge_cycle", "last_only", "random")
INVERT_PATTERNS = ("pm1", "max", "edge_cycle", "random")


@functools.lru_cache(maxsize=None)
def operand(fid, pattern, n, seed=0, nonzero=False):
    """n words.  nonzero=True (inversion): the words that are 0 mod p are left out of the cycle and of the random draw"""
    p = C.FIELDS[fid]
    if pattern == "pm1":
        return (p - 1,) * n
    if pattern == "max":
        return (M256,) * n
    if pattern == "edge_cycle":
        cyc = [w for w in EDGE(p) + NONCANON(p) if not (nonzero and w % p == 0)]
        return tuple(cyc[(i + seed) % len(cyc)] for i in range(n))
    if pattern == "last_only":
        assert not nonzero
        return (0,) * (n - 1) + (p - 1,) * min(n, 1)
    assert pattern == "random"
    rng = random.Random(0x0D + 977 * fid + 31 * seed + n)
    return tuple(rng.randrange(1 if nonzero else 0, p) for _ in range(n))


def zero_class(p):
    """words that are 0 mod p: 0, p, 2p, and 3p where it is below 2^256"""
    return [k * p for k in range(4) if k * p < (1 << 256)]


# ---- expectations -----------------------------------------------------------------------------------------------------------------------
def expect_mle(fid, z_words, r, mont):
    """the word nmx_mle_evaluate returns: sum_x z[x] eq(r, x) over VALUES, back in the layout"""
    p = C.FIELDS[fid]
    z = values(p, z_words, mont)
    e = eq_values(fid, tuple(r))
    assert len(z) == len(e)
    return words_of(p, [sum(a * b for a, b in zip(z, e) if b) % p], mont)[0]


def horner(p, coeffs, u):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * u + c) % p
    return acc


def expect_eval(fid, f_words, u, mont):
    """the word nmx_poly_eval_multi returns for coefficients f (low to high) at the point u (a VALUE): Horner over integers.  An
    evaluation is linear in the coefficients, so the factor 2^-256 that turns Montgomery words into values and the 2^256 that turns the
    result back cancel: the word is Horner over the words read mod p, in both layouts (test_eval_edges.py checks that against the long
    way round)."""
    p = C.FIELDS[fid]
    return horner(p, [w % p for w in f_words], u)


def expect_eval_long_way(fid, f_words, u, mont):
    p = C.FIELDS[fid]
    return words_of(p, [horner(p, values(p, f_words, mont), u)], mont)[0]


def expect_inverse(fid, words, mont):
    """the words of nmx_field_batch_invert, or None when a word is 0 mod p"""
    p = C.FIELDS[fid]
    vals = values(p, words, mont)
    if any(v == 0 for v in vals):
        return None
    memo = {}
    for v in set(vals):
        memo[v] = pow(v, -1, p)
    return words_of(p, [memo[v] for v in vals], mont)


def eval_points(fid):
    """the four points of the evaluation tests, as values: 0, 1, p - 1 and a random one"""
    p = C.FIELDS[fid]
    return [0, 1, p - 1, random.Random(0xE7A1 + fid).randrange(2, p - 1)]
