"""The dense field-vector maps and the three sum passes at their value and lane edges, without a GPU.  (1) The fixtures of
tests/fieldvec_edges_common.py are what they claim to be.  (2) The C oracle oracle.cref -- the yardstick of tests/test_gpu_fieldvec.py --
equals the big-integer expectation on every canonical fixture.  (3) The map functors (nova_amd/csrc/fieldvec_maps.hpp) and the lane bodies
of k_eq_sums / k_eq_rows, k_bind_eq_sums and k_plain_sums (nova_amd/csrc/sumcheck_sums.hpp) run on the CPU with limb bounds asserted
(tests/host_emul/fieldvec_emul.cpp, built here with -DNMX_DEBUG_BOUNDS) over both operand grids, every challenge, four fields and both
layouts; every output is the big integer byte for byte and < p.  The constants a call derives from its challenge (r 2^261, p - u,
2^522 or 2^266, nk) are computed here, so the host half is not trusted.

What the emulation does NOT run: the block reductions (block_sum, block_sum_waves), k_sum_partials_n, the staging of host operands,
the host-side form constants (the correction 2^e; it IS restated here to tie the lane sums to the fixtures' expectations) and
k_fold_chain -- tests/test_gpu_fieldvec_edges.py covers those."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import cref
from tests import fieldvec_edges_common as X
from tests import fv_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_SRC = os.path.join(ROOT, "tests", "host_emul", "fieldvec_emul.cpp")
EMUL_SO = os.path.join(ROOT, "tests", "host_emul", "libnmx_fieldvec_emul.so")
CSRC = os.path.join(ROOT, "nova_amd", "csrc")
RI = 1 << 261  # the internal residue form: x * 2^261 mod p (nova_amd/csrc/fp.hpp)
FIDS = sorted(C.FIELDS)
LAYOUTS = pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
OPS = {"axpy": 0, "axpy2": 1, "cross_term": 2, "cross_term2": 3, "vec_add": 4, "bind": 5}


# ---- (1) the fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIDS)
def test_fixtures_are_what_they_claim(fid):
    p = C.FIELDS[fid]
    assert X.EDGE(p) == [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, (1 << 256) % p] and all(v < p for v in X.EDGE(p))
    assert X.NONCANON(p) == [p, p + 1, 2 * p + 5, (1 << 256) - 1] and all(p <= v < (1 << 256) for v in X.NONCANON(p))
    for k in (2, 3, 4, 5):
        for nc in (False, True):
            vals, g = X.grid_values(p, k, nc), X.grid(fid, k, nc)
            assert len(g) == k and len(g[0]) == len(vals) ** k < X.GRID_MAX_ROWS
            assert all(0 <= w < (1 << 256) for col in g for w in col)
            if nc:
                assert set(vals) == {0, p - 1} | set(X.NONCANON(p))
            else:
                assert {0, 1, p - 1, p - 2, (p - 1) // 2} <= set(vals) <= set(X.EDGE(p))
                assert k == 5 or set(vals) == set(X.EDGE(p))
            # every pair of values meets in every pair of operands (in particular every pair of extremes)
            for a in range(k):
                for b in range(a + 1, k):
                    assert set(zip(g[a], g[b])) == {(x, y) for x in vals for y in vals}
            assert tuple(col[0] for col in g) == (vals[0],) * k and tuple(col[-1] for col in g) == (vals[-1],) * k
    # all operands p - 1 at once, and all 2^256 - 1 at once
    assert (p - 1,) * 5 in set(zip(*X.grid(fid, 5))) and ((1 << 256) - 1,) * 5 in set(zip(*X.grid(fid, 5, True)))
    ch = X.challenges(fid)
    assert ch[:4] == [0, 1, p - 1, p - 2] and len(ch) == 5 and 2 < ch[4] < p - 2
    assert {24, 25} <= set(X.LINCOMB_KS) and max(X.LINCOMB_KS) == 49
    assert [len(v) for v in X.lincomb_vectors(fid, 8, "max")] == [300, 1, 255, 256, 257, 299, 64, 300]
    for pat in X.TABLE_PATTERNS:
        for which in range(3):
            t = X.table(fid, pat, 16, which)
            assert len(t) == 16 and all(0 <= w < (1 << 256) for w in t)
    assert X.table(fid, "lo0_hi_pm1", 8) == (0,) * 4 + (p - 1,) * 4 and X.table(fid, "lo_max_hi0", 8) == ((1 << 256) - 1,) * 4 + (0,) * 4
    assert X.table(fid, "lo0_hi_pm1", 8, 2) == X.table(fid, "lo_pm1_hi0", 8)
    assert X.table(fid, "lo0_hi_max", 8, 0, True) == (0, 0) + ((1 << 256) - 1,) * 4 + (0, 0)
    assert X.eq_table(fid, "pm1", 4) == (p - 1,) * 4 and all(w < p for w in X.eq_table(fid, "random", 9))
    assert {t for t, _e in X.SUM_CASES} == set(X.TABLE_PATTERNS) and {e for _t, e in X.SUM_CASES} == set(X.EQ_PATTERNS)
    # the layouts: a Montgomery word w stands for w 2^-256; linear maps act on words as they are, a product carries one 2^-256
    Rm = (1 << 256) % p
    assert X.expect_map("vec_add", fid, ([3], [p - 1]), 0, True) == [2]
    assert X.expect_map("axpy", fid, ([5], [7]), 3, True) == [26] and X.challenge_word(p, 3, True) == 3 * Rm % p
    assert X.expect_map("cross_term", fid, ([Rm * 3 % p], [Rm * 5 % p], [0], [Rm]), 0, True) == [14 * Rm % p]


# ---- (2) the C oracle on the canonical fixtures -----------------------------------------------------------------------------------------
def _b(words):
    return C.vec(words)


@pytest.mark.parametrize("fid", FIDS)
def test_c_oracle_equals_python_integers_on_every_canonical_fixture(fid):
    import __graft_entry__
    __graft_entry__.build()
    p = C.FIELDS[fid]
    got = lambda b: C.ints(np.frombuffer(C.to_bytes(b), np.uint8))   # noqa: E731
    for c in X.challenges(fid):
        r = _b([c])
        g = X.grid(fid, 2)
        n = len(g[0])
        assert got(cref.field_axpy(fid, _b(g[0]), _b(g[1]), r, n)) == X.expect_map("axpy", fid, g, c, False)
        assert got(cref.field_bind(fid, _b(X.bind_top_input(*g)), 0, n, 1, r, n)) == X.expect_map("bind", fid, g, c, False)
        assert got(cref.field_bind(fid, _b(X.fold_pairs_input(*g)), 0, 1, 2, r, n)) == X.expect_map("bind", fid, g, c, False)
        g = X.grid(fid, 3)
        assert got(cref.field_axpy2(fid, _b(g[0]), _b(g[1]), _b(g[2]), r, len(g[0]))) == X.expect_map("axpy2", fid, g, c, False)
        g = X.grid(fid, 4)
        assert got(cref.field_cross_term(fid, *[_b(x) for x in g], r, len(g[0]))) == X.expect_map("cross_term", fid, g, c, False)
        g = X.grid(fid, 5)
        assert got(cref.field_cross_term2(fid, *[_b(x) for x in g], r, len(g[0]))) == X.expect_map("cross_term2", fid, g, c, False)
    for k in (24, 25, 29):
        vecs = X.lincomb_vectors(fid, k, "p-1")
        for s in X.lincomb_weights(p):
            assert got(cref.lincomb_powers(fid, [_b(v).tobytes() for v in vecs], _b([s]), X.LINCOMB_N_OUT)) == \
                X.expect_lincomb(fid, vecs, s, X.LINCOMB_N_OUT, False)
    n = 2 * (256 + 5)
    for tpat, epat in X.SUM_CASES:
        if not X.is_canonical_case(tpat, epat):
            continue
        A, B, Cc = (X.table(fid, tpat, n, w) for w in range(3))
        eqR = X.eq_table(fid, epat, n // 2)
        for mode in (1, 2, 3):
            want = X.expect_eq_sums(fid, mode, A, B, Cc, eqR, None, 0, False)
            assert tuple(got(b)[0] for b in cref.sumcheck_eq_sums(fid, mode, _b(A), _b(B), _b(Cc), n, _b(eqR))) == want, (tpat, epat, mode)
        eqL, eqR3 = X.eq_table(fid, epat, -(-(n // 2) // 8), 1), X.eq_table(fid, epat, 8, 2)
        want = X.expect_eq_sums(fid, 3, A, B, Cc, eqR3, eqL, 3, False)
        assert tuple(got(b)[0] for b in cref.sumcheck_eq_sums(fid, 3, _b(A), _b(B), _b(Cc), n, _b(eqR3), _b(eqL), 3)) == want, (tpat, epat)
        for kind in (1, 2, 3, 4):
            want = X.expect_plain_sums(fid, kind, A, B, Cc, False)
            assert tuple(got(b)[0] for b in cref.sumcheck_plain_sums(fid, kind, _b(A), _b(B), _b(Cc), n))[:len(want)] == want, (tpat, kind)


# ---- (3) the emulation, limb bounds asserted -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def E():
    deps = [EMUL_SRC] + [os.path.join(CSRC, f) for f in ("fp.hpp", "spmv_row.hpp", "fieldvec_maps.hpp", "sumcheck_sums.hpp")]
    if not os.path.exists(EMUL_SO) or os.path.getmtime(EMUL_SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", EMUL_SO, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_SO)
    vp, u32, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    lib.emul_fv_map.argtypes = [i, i, vp, vp, vp, u32, u32, vp, vp]
    lib.emul_fv_lincomb.argtypes = [i, vp, vp, vp, u32, u32, vp]
    lib.emul_eq_sums.argtypes = [i, i, vp, vp, vp, vp, vp, u32, u32, vp, u32, i, vp]
    lib.emul_bind_eq_sums.argtypes = [i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, vp, u32, vp]
    lib.emul_plain_sums.argtypes = [i, i, vp, vp, vp, u32, u32, vp]
    return lib


def u32(vals):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in vals) or bytes(32), np.uint32).copy()


def ptr(a):
    return None if a is None else a.ctypes.data


def map_constants(p, name, c, mont):
    """what the host half hands the functor: r 2^261 (and r^2 2^261); (p - u) 2^261 and 2^522 / Fm"""
    if name in ("axpy", "bind", "fold_pair"):
        return [c * RI % p], None
    if name == "axpy2":
        return [c * RI % p], [c * c * RI % p]
    if name in ("cross_term", "cross_term2"):
        return [(p - c) % p * RI % p], [(1 << (266 if mont else 522)) % p]
    return None, None


def run_map(E, fid, name, cols, c, mont, stride=1, n=None):
    p = C.FIELDS[fid]
    arrs = [u32(col) for col in cols]
    n = len(cols[0]) if n is None else n
    ins = (ctypes.c_void_p * 5)(*[a.ctypes.data for a in arrs])
    c0, c1 = map_constants(p, name, c, mont)
    c0, c1 = (None if c0 is None else u32(c0)), (None if c1 is None else u32(c1))
    out = np.full(n * 8, 0xa5a5a5a5, np.uint32)
    assert E.emul_fv_map(fid, OPS[name], ins, ptr(c0), ptr(c1), n, stride, out.ctypes.data, None) == 0
    return C.ints(out.view(np.uint8))


@LAYOUTS
@pytest.mark.parametrize("noncanon", [False, True], ids=["edge", "words>=p"])
@pytest.mark.parametrize("name", sorted(OPS))
@pytest.mark.parametrize("fid", FIDS)
def test_emulated_maps_over_the_grids_and_every_challenge(E, fid, name, noncanon, mont):
    p = C.FIELDS[fid]
    k, has_c, _fn = X.MAPS[name]
    g = X.grid(fid, k, noncanon)
    for c in (X.challenges(fid) if has_c else [0]):
        got, want = run_map(E, fid, name, g, c, mont), X.expect_map(name, fid, g, c, mont)
        bad = [X.grid_row_name(fid, k, noncanon, r) for r in range(len(want)) if got[r] != want[r]]
        assert not bad, (c, len(bad), bad[:4])
        assert all(x < p for x in got)


@pytest.mark.parametrize("noncanon", [False, True], ids=["edge", "words>=p"])
@pytest.mark.parametrize("fid", FIDS)
def test_emulated_bind_with_stride_two_and_the_nifs_fold(E, fid, noncanon):
    """BindTopFn as fold_pairs launches it (lo = P, hi = P + 1, stride 2), and FoldPairFn (two axpys in one launch, split at n_w)"""
    p = C.FIELDS[fid]
    g = X.grid(fid, 2, noncanon)
    n = len(g[0])
    for c in X.challenges(fid):
        P = u32(X.fold_pairs_input(*g))
        out = np.zeros(n * 8, np.uint32)
        ins = (ctypes.c_void_p * 5)(P.ctypes.data, P.ctypes.data + 32, None, None, None)
        assert E.emul_fv_map(fid, 5, ins, ptr(u32([c * RI % p])), None, n, 2, out.ctypes.data, None) == 0
        assert C.ints(out.view(np.uint8)) == X.expect_map("bind", fid, g, c, False)
        n_w = n // 3
        a, b = u32(g[0]), u32(g[1])
        ow, oe = np.zeros(n_w * 8, np.uint32), np.zeros((n - n_w) * 8, np.uint32)
        ins = (ctypes.c_void_p * 5)(a.ctypes.data, b.ctypes.data, a.ctypes.data + 32 * n_w, b.ctypes.data + 32 * n_w, None)
        assert E.emul_fv_map(fid, 6, ins, ptr(u32([c * RI % p])), None, n, n_w, ow.ctypes.data, oe.ctypes.data) == 0
        assert C.ints(ow.view(np.uint8)) + C.ints(oe.view(np.uint8)) == X.expect_map("axpy", fid, g, c, False)


@pytest.mark.parametrize("fill", ["p-1", "max"])
@pytest.mark.parametrize("fid", FIDS)
def test_emulated_lincomb_either_side_of_twenty_four_vectors(E, fid, fill):
    p = C.FIELDS[fid]
    for k in X.LINCOMB_KS:
        vecs = X.lincomb_vectors(fid, k, fill)
        arrs = [u32(v) for v in vecs]
        addr = np.array([a.ctypes.data for a in arrs], np.uint64)
        lens = np.array([len(v) for v in vecs], np.uint64)
        for s in X.lincomb_weights(p):
            w = u32([pow(s, j, p) * RI % p for j in range(k)])
            out = np.full(X.LINCOMB_N_OUT * 8, 0xa5a5a5a5, np.uint32)
            assert E.emul_fv_lincomb(fid, addr.ctypes.data, lens.ctypes.data, w.ctypes.data, k, X.LINCOMB_N_OUT, out.ctypes.data) == 0
            got = C.ints(out.view(np.uint8))
            assert got == X.expect_lincomb(fid, vecs, s, X.LINCOMB_N_OUT, False), (k, hex(s))
            assert all(x < p for x in got)


# -- the sum passes: per-index terms in the kernels' own scale (residues; a product of two residues is x y 2^-261) -------------------------
def nk_of(p, mode, mont):
    """p - fconst: mode 3 the plain form factor Fm, mode 2 the constant 1 at product scale, Fm^2 2^-261 (sumcheck.hip eq_sums_t)"""
    if mode == 1:
        return 0
    Fm = (1 << 256) % p if mont else 1
    return (p - (Fm if mode == 3 else Fm * Fm * pow(RI, -1, p) % p)) % p


def eq_terms(p, mode, A, B, Cc, eqL, eqR, shift, h, nk):
    ri = pow(RI, -1, p)
    out, memo = [], {}   # (the uniform tables repeat a handful of index tuples)
    for i in range(h):
        key = (A[i], A[i + h], B[i], B[i + h], Cc[i], eqR[i] if eqL is None else eqR[i & ((1 << shift) - 1)], 0 if eqL is None else eqL[i >> shift])
        if key not in memo:
            f = eqR[i] % p if eqL is None else eqL[i >> shift] * eqR[i & ((1 << shift) - 1)] * ri % p
            if mode == 1:
                memo[key] = (A[i] * f * ri % p, 0)
            else:
                e0 = (A[i] * B[i] + Cc[i] * nk) * ri % p if mode == 3 else (A[i] * B[i] * ri + nk) % p
                q = (A[i + h] - A[i]) * (B[i + h] - B[i]) * ri % p
                memo[key] = (e0 * f * ri % p, q * f * ri % p)
        out.append(memo[key])
    return out


def correction(p, k, mont):
    """sums carry x Fm^k / R'^(k-1); back to the vectors' own form x Fm: times R'^(k-1) / Fm^(k-1)"""
    return pow(2, 261 * (k - 1) - (256 * (k - 1) if mont else 0), p)


def lane_sums(out, lanes, per):
    v = C.ints(out.view(np.uint8))
    return [tuple(v[per * l + j] for j in range(per)) for l in range(lanes)]


def check_lanes(p, got, terms, lane_of, lanes, per, what):
    want = [[0] * per for _ in range(lanes)]
    for i, t in enumerate(terms):
        for j in range(per):
            want[lane_of(i)][j] += t[j]
    want = [tuple(x % p for x in w) for w in want]
    bad = [l for l in range(lanes) if got[l] != want[l]]
    assert not bad, (what, len(bad), bad[:6])
    assert all(x < p for g in got for x in g), what


SUM_SHAPES = [(grid, per) for grid in (1, 2) for per in (1, 12, 13)]
# mode 1 hands the kernel nothing that depends on the layout (nk = 0): it runs once and both corrections are checked
MODE_LAYOUTS = pytest.mark.parametrize("mode,monts", [(1, (False, True)), (2, (False,)), (2, (True,)), (3, (False,)), (3, (True,))],
                                       ids=["mode1", "mode2-canonical", "mode2-montgomery", "mode3-canonical", "mode3-montgomery"])


def check_totals(p, got, k, monts, expect, what):
    """the lane sums, corrected as the host half does, are the fixture's expectation (what the GPU test asserts)"""
    for mont in monts:
        corr = correction(p, k, mont)
        assert tuple(sum(g[j] for g in got) * corr % p for j in range(2)) == expect(mont), (what, mont)


@MODE_LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_emulated_eq_sums_lanes(E, fid, mode, monts):
    p = C.FIELDS[fid]
    nk = nk_of(p, mode, monts[0])
    for grid, per in SUM_SHAPES:
        h = grid * 256 * per + 1   # `per` indices per lane and one odd index: the pair loop either side of its sixth turn, then the tail
        for tpat, epat in X.SUM_CASES:
            A, B, Cc = (X.table(fid, tpat, 2 * h, w) for w in range(3))
            eqR = X.eq_table(fid, epat, h)
            out = np.zeros(grid * 256 * 16, np.uint32)
            assert E.emul_eq_sums(fid, mode, ptr(u32(A)), ptr(u32(B)), ptr(u32(Cc)), None, ptr(u32(eqR)), 0, h, ptr(u32([nk])), grid, 0,
                                  out.ctypes.data) == 0
            got = lane_sums(out, grid * 256, 2)
            terms = eq_terms(p, mode, A, B, Cc, None, eqR, 0, h, nk)
            check_lanes(p, got, terms, lambda i: i % (grid * 256), grid * 256, 2, (grid, per, tpat, epat))
            check_totals(p, got, 2 if mode == 1 else 3, monts, lambda mont: X.expect_eq_sums(fid, mode, A, B, Cc, eqR, None, 0, mont),
                         (grid, per, tpat, epat))


@pytest.mark.parametrize("rows", [0, 1], ids=["k_eq_sums", "k_eq_rows"])
@MODE_LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_emulated_eq_sums_with_a_left_table(E, fid, mode, monts, rows):
    """shift 3: 32 rows per block, 13 rows per lane and a partial last row (pend_g); shift 13: K = 32 indices per lane and row (pend), one
    whole row and a partial one (k_eq_rows only: k_eq_sums walks indices, not rows, and has met the left table at shift 3)"""
    p = C.FIELDS[fid]
    nk = nk_of(p, mode, monts[0])
    for shift, h in ((3, 8 * 32 * 13 + 5), (13, (1 << 13) + 256 * 13 + 5))[:2 if rows else 1]:
        row = 1 << shift
        P = min(row, 256)
        rpb = 256 // P
        for grid in (1, 2):
            for tpat, epat in X.SUM_CASES:
                A, B, Cc = (X.table(fid, tpat, 2 * h, w) for w in range(3))
                eqL, eqR = X.eq_table(fid, epat, -(-h // row), 1), X.eq_table(fid, epat, row, 2)
                out = np.zeros(grid * 256 * 16, np.uint32)
                assert E.emul_eq_sums(fid, mode, ptr(u32(A)), ptr(u32(B)), ptr(u32(Cc)), ptr(u32(eqL)), ptr(u32(eqR)), shift, h, ptr(u32([nk])),
                                      grid, rows, out.ctypes.data) == 0
                got = lane_sums(out, grid * 256, 2)
                terms = eq_terms(p, mode, A, B, Cc, eqL, eqR, shift, h, nk)
                if rows:
                    lane_of = lambda i: ((i >> shift) // rpb % grid) * 256 + ((i >> shift) % rpb) * P + (i & (row - 1)) % P   # noqa: E731
                else:
                    lane_of = lambda i: i % (grid * 256)   # noqa: E731
                check_lanes(p, got, terms, lane_of, grid * 256, 2, (shift, grid, tpat, epat))
                check_totals(p, got, 3 if mode == 1 else 4, monts, lambda mont: X.expect_eq_sums(fid, mode, A, B, Cc, eqR, eqL, shift, mont),
                             (shift, grid, tpat, epat))


@MODE_LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_emulated_bind_eq_sums_lanes_and_bound_tables(E, fid, mode, monts):
    p = C.FIELDS[fid]
    nk = nk_of(p, mode, monts[0])
    cs = X.challenges(fid)
    for n_case, (grid, per) in enumerate(SUM_SHAPES):
        hq = grid * 256 * per + 1
        for tpat, epat in X.SUM_CASES:
            c = cs[(n_case + len(tpat)) % len(cs)]
            T = [X.table(fid, tpat, 4 * hq, w, True) for w in range(3)]
            eqR = X.eq_table(fid, epat, hq)
            bufs = [u32(t) for t in T]
            out = np.zeros(grid * 256 * 16, np.uint32)
            assert E.emul_bind_eq_sums(fid, mode, *[ptr(b) for b in bufs], *[ptr(b) for b in bufs], ptr(u32([c * RI % p])), None, ptr(u32(eqR)), 0,
                                       hq, ptr(u32([nk])), grid, out.ctypes.data) == 0   # in place, as the product call
            bound = [X.expect_bind_top(fid, t, c, False) if m < mode else list(t[:2 * hq]) for m, t in enumerate(T)]   # (linear: the same words in both layouts)
            for m in range(mode):
                assert C.ints(bufs[m].view(np.uint8))[:2 * hq] == bound[m], (grid, per, tpat, "table %d" % m)
            got = lane_sums(out, grid * 256, 2)
            terms = eq_terms(p, mode, bound[0], bound[1], bound[2], None, eqR, 0, hq, nk)
            check_lanes(p, got, terms, lambda i: i % (grid * 256), grid * 256, 2, (grid, per, tpat, epat))
            if per == 1:   # (the fixture's own composition of bind and sums, once per grid: it binds all over again)
                assert X.expect_bind_eq_sums(fid, mode, T[0], T[1], T[2], c, eqR, None, 0, monts[0])[0][:mode] == bound[:mode]
            check_totals(p, got, 2 if mode == 1 else 3, monts, lambda mont: X.expect_eq_sums(fid, mode, bound[0], bound[1], bound[2], eqR, None, 0, mont),
                         (grid, per, tpat, epat))


def plain_terms(p, kind, A, B, Cc, h):
    ri = pow(RI, -1, p)
    out = []
    for i in range(h):
        a0, a1, b0, b1 = A[i], A[i + h], B[i], B[i + h]
        if kind == 1:
            out.append((a0 * b0 * ri % p, (a1 - a0) * (b1 - b0) * ri % p, 0))
        elif kind == 2:
            out.append(((a0 - b0) % p, ((2 * a0 - a1) - (2 * b0 - b1)) % p, 0))
        elif kind == 3:
            out.append((a0 * b0 * ri % p, (2 * a0 - a1) * (2 * b0 - b1) * ri % p, 0))
        else:
            c0, c1 = Cc[i], Cc[i + h]
            out.append((a0 * b0 * c0 * ri * ri % p, (a1 - a0) * (b1 - b0) * (c1 - c0) * ri * ri % p,
                        (2 * a0 - a1) * (2 * b0 - b1) * (2 * c0 - c1) * ri * ri % p))
    return out


@pytest.mark.parametrize("kind", [1, 2, 3, 4])
@pytest.mark.parametrize("fid", FIDS)
def test_emulated_plain_sums_lanes(E, fid, kind):
    p = C.FIELDS[fid]
    for grid, per in SUM_SHAPES:
        h = grid * 256 * per + 1
        for tpat in X.TABLE_PATTERNS:
            A, B, Cc = (X.table(fid, tpat, 2 * h, w) for w in range(3))
            out = np.zeros(grid * 256 * 24, np.uint32)
            assert E.emul_plain_sums(fid, kind, ptr(u32(A)), ptr(u32(B)), ptr(u32(Cc)), h, grid, out.ctypes.data) == 0
            got = lane_sums(out, grid * 256, 3)
            check_lanes(p, got, plain_terms(p, kind, A, B, Cc, h), lambda i: i % (grid * 256), grid * 256, 3, (grid, per, tpat))
            k = {1: 2, 2: 1, 3: 2, 4: 3}[kind]
            for mont in (False, True):
                corr = correction(p, k, mont)
                tot = tuple(sum(g[j] for g in got) * corr % p for j in range(3 if kind == 4 else 2))
                assert tot == X.expect_plain_sums(fid, kind, A, B, Cc, mont), (grid, per, tpat, mont)
