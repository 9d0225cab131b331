"""NeutronNova's folding step restated in Python integers, from the formulas of include/nova_mi355x.h and the reference (src/neutron/nifs.rs:29-186
prove_helper, src/neutron/relation.rs:83-97 is_sat and :131-156 FoldedWitness::fold, src/spartan/polys/power.rs:62-86 split_evals,
src/spartan/polys/univariate.rs from_evals) and deliberately NOT in the factored, incrementally walked form the kernels use
(nova_amd/csrc/neutron.hpp).  This module is the yardstick of tests/test_neutron_abi.py and tests/test_gpu_neutron.py; it shares no code with
the library.  Everything here works on VALUES mod p; words()/values() move between values and the stored 256-bit words of a layout.

Notation: E = e ++ f, e = E[:left], f = E[left:]; an N-vector (N = left * right) is indexed k = i * left + j; X(t) = X1 + t (X2 - X1)."""
import functools
import random

from tests import fv_common as fc

R256 = 1 << 256
POINTS = (0, 2, 3, 4, 5)
# (left, right) of the two sums: single element, single row / column, odd sizes, a partial tile next to full ones (65 and 1024 against the
# kernels' 64 lanes and 256-column tiles), more tiles than one block takes (256 x 256: 256 tiles, 512 x 256: 512) and a row of four tiles
SMALL_SHAPES = ((1, 1), (2, 1), (2, 2), (1, 64), (64, 1), (3, 5), (65, 7), (8, 4))
LARGE_SHAPES = ((256, 256), (512, 256), (1024, 3))


# ---- the four definitions -------------------------------------------------------------------------------------------------------------
def pow_split_evals(p, tau, left, right):
    tl = pow(tau, left, p)
    return [pow(tau, j, p) for j in range(left)] + [pow(tl, i, p) for i in range(right)]    # pow(0, 0, p) == 1


def relation_sum(p, left, right, E, Az, Bz, Cz):
    assert len(E) == left + right and len(Az) == len(Bz) == len(Cz) == left * right
    total = 0
    for i in range(right):
        for j in range(left):
            k = i * left + j
            total += E[left + i] * E[j] * (Az[k] * Bz[k] - Cz[k])
    return total % p


def at(p, v1, v2, t):
    return [(x1 + t * (x2 - x1)) % p for x1, x2 in zip(v1, v2)]


def fold_sums(p, left, right, inst1, inst2, rho):
    """inst = (E, Az, Bz, Cz) -> the five values out_t, t = 0, 2, 3, 4, 5"""
    out = []
    for t in POINTS:
        c_t = ((1 - rho) + t * (2 * rho - 1)) % p
        out.append(c_t * relation_sum(p, left, right, *[at(p, v1, v2, t) for v1, v2 in zip(inst1, inst2)]) % p)
    return out


def fold_witness(p, w1, w2, e1, e2, r_b):
    return at(p, w1, w2, r_b), at(p, e1, e2, r_b)


# ---- UniPoly::from_evals as Lagrange interpolation on 0 .. len - 1; coefficients low to high --------------------------------------------
def from_evals(p, evals):
    n = len(evals)
    coeffs = [0] * n
    for i, y in enumerate(evals):
        num, den = [1], 1                           # prod_{m != i} (X - m) / (i - m)
        for m in range(n):
            if m != i:
                num = [(a - m * b) % p for a, b in zip([0] + num, num + [0])]
                den = den * (i - m) % p
        s = y * pow(den, -1, p) % p
        for k in range(n):
            coeffs[k] = (coeffs[k] + s * num[k]) % p
    return coeffs


def poly_eval(p, coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


def eq(p, a, b):
    return ((1 - a) * (1 - b) + a * b) % p


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------
def words(p, vals, mont):
    """values -> the stored words of the layout (canonical representatives)"""
    return [v * R256 % p for v in vals] if mont else [v % p for v in vals]


def values(p, ws, mont):
    """stored words, ANY 256-bit values -> the values they stand for (w mod p; Montgomery: w 2^-256 mod p)"""
    inv = pow(R256, -1, p)
    return [w * inv % p for w in ws] if mont else [w % p for w in ws]


# ---- cases: eight lists of STORED WORDS (E1, Az1, Bz1, Cz1, E2, Az2, Bz2, Cz2) and the value of rho ------------------------------------
class Case:
    def __init__(self, name, fid, left, right, vecs, rho):
        self.name, self.fid, self.p, self.left, self.right, self.vecs, self.rho = name, fid, fc.FIELDS[fid], left, right, vecs, rho

    def want_fold(self, mont):
        v = [values(self.p, w, mont) for w in self.vecs]
        return fold_sums(self.p, self.left, self.right, v[:4], v[4:], self.rho)

    def want_relation(self, mont, which=1):
        v = [values(self.p, w, mont) for w in self.vecs]
        return relation_sum(self.p, self.left, self.right, *(v[4:] if which == 2 else v[:4]))


def sizes(left, right):
    n = left * right
    return [left + right, n, n, n] * 2


@functools.lru_cache(maxsize=None)
def random_case(fid, left, right, seed=1):
    p, rng = fc.FIELDS[fid], random.Random(1000 * seed + 97 * fid + 7 * left + right)
    return Case("random", fid, left, right, [[rng.randrange(p) for _ in range(m)] for m in sizes(left, right)], rng.randrange(p))


def edge_cases(fid, left, right, seed=2):
    """the edge contents of the issue, as stored words: all 0; all p - 1; the words p, p + 1 and 2^256 - 1 in every vector; rho in
    {0, 1, (p + 1) / 2, p - 1}; instance 1 all zero (the default running instance); instance 1 == instance 2"""
    p, rng = fc.FIELDS[fid], random.Random(31 * seed + fid)
    sz = sizes(left, right)
    rnd = lambda: [[rng.randrange(p) for _ in range(m)] for m in sz]  # noqa: E731
    yield Case("all zero", fid, left, right, [[0] * m for m in sz], rng.randrange(p))
    yield Case("all p - 1", fid, left, right, [[p - 1] * m for m in sz], p - 1)
    v = rnd()
    for vec in v:
        for x in (p, p + 1, R256 - 1):
            vec[rng.randrange(len(vec))] = x
    yield Case("words at and above p", fid, left, right, v, rng.randrange(p))
    yield Case("every word 2^256 - 1", fid, left, right, [[R256 - 1] * m for m in sz], p - 1)
    base = rnd()
    for rho in (0, 1, (p + 1) // 2, p - 1):
        yield Case("rho = %d" % rho, fid, left, right, base, rho)
    v = rnd()
    yield Case("instance 1 zero", fid, left, right, [[0] * m for m in sz[:4]] + v[4:], rng.randrange(p))
    yield Case("instance 1 == instance 2", fid, left, right, v[4:] + v[4:], rng.randrange(p))
