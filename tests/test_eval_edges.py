"""The eq tables, the MLE and polynomial evaluations and batch inversion at their edges, without a GPU.  (1) The fixtures of
tests/eval_edges_common.py are what they claim to be.  (2) The C oracle oracle.cref -- the yardstick of tests/test_gpu_fieldvec.py --
equals the big-integer expectation on every canonical fixture.  (3) The functors of nova_amd/csrc/fieldvec_eval.hpp (EqDirectFn,
EqDirect2Fn, EqSplit2Fn + EqProductFn, EqStepFn, BatchInvFwdFn / BatchInvBwdFn, eval_multi_lane) run on the CPU with limb bounds asserted
(tests/host_emul/eval_emul.cpp, built here with -DNMX_DEBUG_BOUNDS: a violated bound aborts the run), four fields, both layouts; every
output is the big integer byte for byte and < p.  The constants a call derives on the host (r 2^261, (1 - r) 2^261, ONE in the vectors'
form, the internal ONE, the chunk inverses, the points and power tables) are computed here, so the host half is not trusted.

EqStepFn chained to ell = 10 over every point pattern is the only check of the doubling form that nmx_eq_evals_from_points takes from
ell = 25 (a 1 GiB table, which no GPU test builds).  What the emulation does NOT run: the choice of form by ell, staging, block_sum and
the block powers of k_eval_multi, the host level of batch_invert, the kernels of the device-resident evaluations --
tests/test_gpu_eval_edges.py covers those."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import cref
from tests import eval_edges_common as X
from tests import fv_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_SRC = os.path.join(ROOT, "tests", "host_emul", "eval_emul.cpp")
EMUL_SO = os.path.join(ROOT, "tests", "host_emul", "libnmx_eval_emul.so")
CSRC = os.path.join(ROOT, "nova_amd", "csrc")
RI = 1 << 261  # the internal residue form: x * 2^261 mod p (nova_amd/csrc/fp.hpp)
FIDS = sorted(C.FIELDS)
LAYOUTS = pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])


# ---- (1) the fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIDS)
def test_fixtures_are_what_they_claim(fid):
    p = C.FIELDS[fid]
    R = (1 << 256) % p
    assert set(X.CHALLENGE_PATTERNS) == {"zeros", "ones", "alt01", "alt10", "pm1", "twos", "half", "random"}
    assert X.point(fid, "alt01", 4) == (0, 1, 0, 1) and X.point(fid, "alt10", 3) == (1, 0, 1) and X.point(fid, "pm1", 2) == (p - 1, p - 1)
    assert X.point(fid, "twos", 2) == (2, 2) and X.point(fid, "half", 1) == ((p + 1) // 2,) and 2 * X.point(fid, "half", 1)[0] % p == 1
    assert all(1 < c < p - 1 for c in X.point(fid, "random", 24)) and len(set(X.point(fid, "random", 24))) == 24
    assert X.point(fid, "zeros", 0) == ()
    # alt01 at ell = 4 is the indicator of index 5 (0b0101: coordinate 0 is the most significant bit)
    assert X.indicator_index(X.point(fid, "alt01", 4)) == 5 and X.indicator_index((2, 0)) is None
    for mont in (False, True):
        assert X.expect_eq(fid, X.point(fid, "alt01", 4), mont) == [(R if mont else 1) if i == 5 else 0 for i in range(16)]
        assert X.expect_eq(fid, X.point(fid, "alt10", 3), mont) == [(R if mont else 1) if i == 5 else 0 for i in range(8)]
        assert X.expect_eq(fid, X.point(fid, "zeros", 3), mont)[0] == (R if mont else 1)
        assert X.expect_eq(fid, X.point(fid, "ones", 3), mont)[7] == (R if mont else 1)
        assert X.expect_eq(fid, (), mont) == [R if mont else 1]
        # half: every entry is 2^-ell
        assert X.expect_eq(fid, X.point(fid, "half", 5), mont) == [pow(2, -5, p) * (R if mont else 1) % p] * 32
        # twos: 1 - r = p - 1, so entry x is (-1)^(zeros of x) 2^(ones of x)
        assert X.expect_eq(fid, X.point(fid, "twos", 2), False) == [1, p - 2, p - 2, 4]
    # r[0] is the most significant variable: eq((a, b), .) = [(1-a)(1-b), (1-a) b, a (1-b), a b]
    a, b = 3, 10
    assert X.expect_eq(fid, (a, b), False) == [(1 - a) * (1 - b) % p, (1 - a) * b % p, a * (1 - b) % p, a * b % p]
    # the sum of a table is 1, for every pattern
    for pat in X.CHALLENGE_PATTERNS:
        assert sum(X.eq_values(fid, X.point(fid, pat, 6))) % p == 1, pat
    # an indicator point picks z[idx] mod p, whatever the words are
    z = X.operand(fid, "edge_cycle", 16)
    assert X.expect_mle(fid, z, X.point(fid, "alt01", 4), False) == z[5] % p
    assert X.expect_mle(fid, z, X.point(fid, "alt01", 4), True) == z[5] % p     # (w 2^-256) 2^256
    zmax = X.operand(fid, "max", 8)
    assert X.expect_mle(fid, zmax, X.point(fid, "random", 3), False) == X.M256 % p   # a constant polynomial
    # Montgomery bookkeeping on two hand-computed rows: z = (3 R, 5 R) stands for (3, 5); at r = 4: 3 + 4 (5 - 3) = 11, as the word 11 R
    assert X.expect_mle(fid, [3 * R % p, 5 * R % p], (4,), True) == 11 * R % p
    assert X.expect_mle(fid, [3, 5], (4,), False) == 11
    # ... and f = 3 + 5 X at u = 4 is 23; the words 3 R, 5 R give the word 23 R
    assert X.expect_eval(fid, [3 * R % p, 5 * R % p], 4, True) == 23 * R % p and X.expect_eval(fid, [3, 5], 4, False) == 23
    assert X.challenge_word(p, 4, True) == 4 * R % p
    f = X.operand(fid, "edge_cycle", 40)
    for u in X.eval_points(fid):
        for mont in (False, True):
            assert X.expect_eval(fid, f, u, mont) == X.expect_eval_long_way(fid, f, u, mont)
    assert X.expect_eval(fid, [], 7, False) == 0
    # inverses: the word 2 R stands for 2, its inverse is the word R / 2; the canonical word p + 2 is read as 2
    assert X.expect_inverse(fid, [2 * R % p], True) == [pow(2, -1, p) * R % p] and X.expect_inverse(fid, [p + 2], False) == [pow(2, -1, p)]
    assert X.expect_inverse(fid, [1, p - 1], False) == [1, p - 1]
    for w in X.zero_class(p):
        assert w % p == 0 and w < (1 << 256) and X.expect_inverse(fid, [1, w, 2], False) is None and X.expect_inverse(fid, [w], True) is None
    assert X.zero_class(p)[:3] == [0, p, 2 * p]
    # operands
    assert X.operand(fid, "pm1", 3) == (p - 1,) * 3 and X.operand(fid, "max", 2) == (X.M256,) * 2
    assert list(X.operand(fid, "edge_cycle", 12)) == X.EDGE(p) + X.NONCANON(p)
    assert X.operand(fid, "last_only", 4) == (0, 0, 0, p - 1) and all(w < p for w in X.operand(fid, "random", 50))
    for pat in X.INVERT_PATTERNS:
        assert all(w % p for w in X.operand(fid, pat, 40, 0, True)), pat
    assert X.M256 in X.operand(fid, "edge_cycle", 40, 0, True) and p + 1 in X.operand(fid, "edge_cycle", 40, 0, True)
    # the pinned point of the 2^24 table: 14 coordinates are zeros and ones, 1024 indices can be non-zero and are
    r = X.pinned_point(fid)
    assert len(r) == 24 and [i for i in range(24) if r[i] in (0, 1)] == list(X.PINNED) and {r[i] for i in X.PINNED} == {0, 1}
    sup = X.pinned_support(r)
    assert len(sup) == len(set(sup)) == 1024 and all(X.eq_value(p, r, x) != 0 for x in sup)
    r8 = (1, 5, 0, 7)
    assert X.pinned_support(r8) == [x for x in range(16) if X.eq_value(p, r8, x)] == [8, 9, 12, 13]


# ---- (2) the C oracle on the canonical fixtures -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIDS)
def test_c_oracle_equals_python_integers_on_every_canonical_fixture(fid):
    import __graft_entry__
    __graft_entry__.build()
    p = C.FIELDS[fid]
    canon = [pat for pat in X.OPERAND_PATTERNS if pat != "max"]
    ops = lambda pat, n: [w % p for w in X.operand(fid, pat, n)]   # noqa: E731  (the oracle takes canonical words)
    for ell in (0, 1, 2, 5, 9):
        n = 1 << ell
        for cpat in X.CHALLENGE_PATTERNS:
            r = X.point(fid, cpat, ell)
            rv = C.vec(r) if ell else np.zeros((0, 32), np.uint8)
            assert C.ints(np.frombuffer(cref.eq_evals(fid, rv, ell), np.uint8)) == X.expect_eq(fid, r, False), (ell, cpat)
            zs = [ops(pat, n) for pat in canon]
            want = [X.expect_mle(fid, z, r, False) for z in zs]
            assert [int.from_bytes(cref.mle_evaluate(fid, C.vec(z), ell, rv), "little") for z in zs] == want, (ell, cpat)
            assert [int.from_bytes(b, "little") for b in cref.mle_multi_evaluate(fid, [C.vec(z) for z in zs], ell, rv)] == want, (ell, cpat)
    for n in (1, 16, 17, 300):
        for pat in canon:
            f = ops(pat, n)
            for u in X.eval_points(fid):
                got = C.ints(np.frombuffer(cref.suffix_horner(fid, C.vec(f), n, C.vec([u])), np.uint8))[0]
                assert got == X.expect_eval(fid, f, u, False), (n, pat)
    for n in (1, 2, 127, 128, 129, 300):
        for pat in X.INVERT_PATTERNS:
            v = [w % p for w in X.operand(fid, pat, n, 0, True)]
            assert C.ints(np.frombuffer(cref.batch_invert(fid, C.vec(v), n), np.uint8)) == X.expect_inverse(fid, v, False), (n, pat)
    v = list(X.operand(fid, "random", 20, 0, True))
    v[7] = 0
    assert cref.batch_invert(fid, C.vec(v), 20) is None and X.expect_inverse(fid, v, False) is None


# ---- (3) the emulation, limb bounds asserted -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def E():
    deps = [EMUL_SRC] + [os.path.join(CSRC, f) for f in ("fp.hpp", "spmv_row.hpp", "fieldvec_eval.hpp")]
    if not os.path.exists(EMUL_SO) or os.path.getmtime(EMUL_SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", EMUL_SO, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_SO)
    vp, u, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    lib.emul_eq_direct.argtypes = [i, u, vp, vp, vp, vp]
    lib.emul_eq_direct2.argtypes = [i, u, u, vp, vp, vp, vp, vp]
    lib.emul_eq_split.argtypes = [i, u, u, vp, vp, vp, vp, vp, vp, vp]
    lib.emul_eq_steps.argtypes = [i, u, vp, vp, vp]
    lib.emul_binv_fwd.argtypes = [i, vp, u, u, u, vp, vp]
    lib.emul_binv_bwd.argtypes = [i, vp, vp, vp, u, u, u]
    lib.emul_eval_lane.argtypes = [i, vp, u, u, u, vp, vp, u, vp]
    return lib


def u32(vals):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in vals) or bytes(32), np.uint32).copy()


def buf(n):
    return np.full(max(n, 1) * 8, 0xa5a5a5a5, np.uint32)


def ints(a, n=None):
    v = C.ints(a.view(np.uint8))
    return v if n is None else v[:n]


def eq_constants(p, r, mont):
    """what the host half hands an eq functor: r_i 2^261, (1 - r_i) 2^261, ONE in the vectors' form as a plain residue"""
    return u32([c * RI % p for c in r]), u32([(1 - c) * RI % p for c in r]), u32([(1 << 256) % p if mont else 1])


def check_table(fid, got, r, mont, what):
    p = C.FIELDS[fid]
    want = X.expect_eq(fid, r, mont)
    bad = [x for x in range(len(want)) if got[x] != want[x]]
    assert not bad, (what, len(bad), bad[:6])
    assert all(w < p for w in got), what


@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_emulated_direct_tables(E, fid, mont):
    """EqDirectFn at ell 0, 1, 2, 11, 12, every point pattern"""
    p = C.FIELDS[fid]
    for ell in (0, 1, 2, 11, 12):
        for pat in X.CHALLENGE_PATTERNS:
            r = X.point(fid, pat, ell)
            rr, nr, one = eq_constants(p, r, mont)
            out = buf(1 << ell)
            assert E.emul_eq_direct(fid, ell, rr.ctypes.data, nr.ctypes.data, one.ctypes.data, out.ctypes.data) == 0
            check_table(fid, ints(out, 1 << ell), r, mont, (ell, pat))


@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_emulated_pair_of_direct_tables(E, fid, mont):
    """EqDirect2Fn: both sqrt-size tables of an evaluation in one launch, at (ellL, ellR) = (1, 0), (1, 1), (5, 4), (12, 12)"""
    p = C.FIELDS[fid]
    for ellL, ellR in ((1, 0), (1, 1), (5, 4), (12, 12)):
        for pat in X.CHALLENGE_PATTERNS:
            r = X.point(fid, pat, ellL + ellR)
            rr, nr, one = eq_constants(p, r, mont)
            oL, oR = buf(1 << ellL), buf(1 << ellR)
            assert E.emul_eq_direct2(fid, ellL, ellR, rr.ctypes.data, nr.ctypes.data, one.ctypes.data, oL.ctypes.data, oR.ctypes.data) == 0
            check_table(fid, ints(oL, 1 << ellL), r[:ellL], mont, (ellL, ellR, pat, "left"))
            check_table(fid, ints(oR, 1 << ellR), r[ellL:], mont, (ellL, ellR, pat, "right"))


@LAYOUTS
@pytest.mark.parametrize("ell", [13, 14, 15])
@pytest.mark.parametrize("fid", FIDS)
def test_emulated_split_tables(E, fid, ell, mont):
    """EqSplit2Fn + EqProductFn with the library's split ellR = ell / 2, ellL = ell - ellR: the left table in the internal form (times
    2^261), the right one in the vectors' form, their product the table"""
    p = C.FIELDS[fid]
    ellR = ell // 2
    ellL = ell - ellR
    pats = X.CHALLENGE_PATTERNS if ell == 13 else ("alt01", "pm1", "random")
    for pat in pats:
        r = X.point(fid, pat, ell)
        rr, nr, one = eq_constants(p, r, mont)
        oneL = u32([RI % p])
        oL, oR, out = buf(1 << ellL), buf(1 << ellR), buf(1 << ell)
        assert E.emul_eq_split(fid, ellL, ellR, rr.ctypes.data, nr.ctypes.data, oneL.ctypes.data, one.ctypes.data, oL.ctypes.data, oR.ctypes.data,
                               out.ctypes.data) == 0
        check_table(fid, ints(out, 1 << ell), r, mont, (ell, pat))
        assert ints(oL, 1 << ellL) == [v * RI % p for v in X.eq_values(fid, r[:ellL])], (ell, pat, "left table, internal form")
        check_table(fid, ints(oR, 1 << ellR), r[ellL:], mont, (ell, pat, "right"))


@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_emulated_doubling_steps_to_ell_10(E, fid, mont):
    """EqStepFn chained as nmx_eq_evals_from_points chains it from ell = 25: the last challenge first, in place"""
    p = C.FIELDS[fid]
    for ell in (1, 2, 10):
        for pat in X.CHALLENGE_PATTERNS:
            r = X.point(fid, pat, ell)
            rr, _nr, one = eq_constants(p, r, mont)
            out = buf(1 << ell)
            assert E.emul_eq_steps(fid, ell, rr.ctypes.data, one.ctypes.data, out.ctypes.data) == 0
            check_table(fid, ints(out, 1 << ell), r, mont, (ell, pat))


@LAYOUTS
@pytest.mark.parametrize("K", [8, 16, 32])
@pytest.mark.parametrize("fid", FIDS)
def test_emulated_batch_invert_level(E, fid, K, mont):
    """One level of Montgomery's trick: T lanes, lane c owns the strided chunk {c, c + T, ...}.  The forward pass leaves the prefix
    products (element j of a chunk: the product of the j words before it over 2^(261 (j - 1)); the first: 2^261) and the chunk products;
    the backward pass, handed Fm^2 / (chunk product) from big integers, leaves Fm^2 / w (Fm = 1, or 2^256 in the Montgomery layout)."""
    p = C.FIELDS[fid]
    Minv = pow(RI, -1, p)
    s = pow(1 << 256, 2, p) if mont else 1
    for T in (1, 5):
        for n in sorted({K * T, K * T - 1, K * (T - 1) + 1}):
            assert (n + K - 1) // K == T
            for pat in X.INVERT_PATTERNS:
                v = X.operand(fid, pat, n, K + T, True)
                want_prefix, want_prod = [0] * n, [0] * T
                for c in range(T):
                    acc = RI % p
                    for i in range(c, n, T):
                        want_prefix[i] = acc
                        acc = acc * v[i] * Minv % p
                    want_prod[c] = acc
                # v and the prefix array are followed by slack up to K T elements (v's: words >= p), which no lane may read or write
                vv, prefix, prod = u32(list(v) + [X.M256 - 1] * (K * T - n)), buf(K * T), buf(T)
                assert E.emul_binv_fwd(fid, vv.ctypes.data, n, T, K, prefix.ctypes.data, prod.ctypes.data) == 0
                assert ints(prefix, n) == want_prefix, (T, n, pat, "prefix products")
                assert ints(prod, T) == want_prod, (T, n, pat, "chunk products")
                assert (prefix[8 * n:] == 0xa5a5a5a5).all(), (T, n, pat, "written past the end")
                cinv = u32([s * pow(x, -1, p) % p for x in want_prod])
                assert E.emul_binv_bwd(fid, vv.ctypes.data, cinv.ctypes.data, prefix.ctypes.data, n, T, K) == 0
                assert (prefix[8 * n:] == 0xa5a5a5a5).all(), (T, n, pat, "written past the end")
                got = ints(prefix, n)
                assert got == X.expect_inverse(fid, v, mont), (T, n, pat, "inverses")
                assert all(w < p for w in got)


@pytest.mark.parametrize("pat", ["pm1", "max"])
@pytest.mark.parametrize("fid", FIDS)
def test_emulated_evaluation_lane(E, fid, pat):
    """eval_multi_lane over chunks [lo, hi) of 16, 15 and 1 coefficients at m = 1 .. 4 points out of 0, 1, p - 1, 2 and a random one:
    (sum_i f[lo + i] u^i) u^(16 t) for lane t, in the coefficients' own form (the layout does not enter: the points arrive in the
    internal form whichever it is)."""
    p = C.FIELDS[fid]
    f = X.operand(fid, pat, 48)
    rnd = random.Random(0x1A + fid).randrange(2, p - 1)
    pts_all = [0, 1, p - 1, 2, rnd]
    for lo, hi in ((0, 16), (16, 31), (47, 48), (32, 48)):
        for m in (1, 2, 3, 4):
            for first in range(len(pts_all)):
                us = [pts_all[(first + j) % len(pts_all)] for j in range(m)]
                for t in (0, 1, 255):
                    pts = u32([u * RI % p for u in us])
                    pw = np.zeros(m * 256 * 8, np.uint32)
                    for j, u in enumerate(us):
                        pw[(j * 256 + t) * 8:(j * 256 + t) * 8 + 8] = u32([pow(u, 16 * t, p) * RI % p])
                    out = buf(4)
                    assert E.emul_eval_lane(fid, u32(f).ctypes.data, lo, hi, m, pts.ctypes.data, pw.ctypes.data, t, out.ctypes.data) == 0
                    got = ints(out, m)
                    want = [X.horner(p, [w % p for w in f[lo:hi]], u) * pow(u, 16 * t, p) % p for u in us]
                    assert got == want, (lo, hi, m, t, first)
                    assert all(w < p for w in got)
