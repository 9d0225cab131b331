"""CPU: the inputs of tests/msm_degenerate_common.py (rank-one keys, digit-edge scalars) checked against a model in Python integers, then run
through the emulation of the kernel bodies (tests/host_emul, the library of tests/test_emul.py) against the closed form.

The model tests are conditions on the INPUTS: they prove that cyc(k) really makes every level-0 pair of the bucket reduction equal, that
cyc_cancel(k) makes it opposite, that heavy fills one bucket per window, and that the digit-edge set reaches M, M + 1 and a carry-made zero
digit in every window where a scalar below r can.  Every window width that a CPU or GPU test of this family uses is in WIDTHS.

The emulator runs cover the code the device shares with the host (XYZZ::add / add_affine_signed / dbl, the accumulate tasks, the folds, the pair
tree, the three digit loops, the host tail).  The four-lane additions of curve_quad.hpp and the GPU-only launch forms are device code:
tests/test_gpu_msm_degenerate.py runs the same inputs there."""
import numpy as np
import pytest

from oracle import cref
from oracle import pyref as R
from tests import msm_degenerate_common as D
from tests.test_emul import emul, run, run_pre  # noqa: F401  (the fixture builds and loads the emulator exactly as test_emul.py does)

PLAIN_WIDTHS = [3, 7, 8, 13, 15, 16, 20]        # emul_msm force_c
TABLE_WIDTHS = [8, 11, 15, 16, 17]              # emul_msm_precomp pre_c
# every width in use: the two lists above, nmx_set_window_bits of the GPU tests (3 .. 20), and the default widths their keys get (9, 10, 14)
WIDTHS = sorted(set(PLAIN_WIDTHS + TABLE_WIDTHS + [3, 7, 8, 13, 15, 16, 17, 20] + [9, 10, 14]))
EMUL_CURVES = [R.BN254_G1, R.PALLAS]            # 254- and 255-bit scalars: the top window differs
SIZES = [300, 8200]                             # below every split; 8200 > 256 * lmax: all three fold passes
KEYS = {"plus": D.signs_plus, "alt": D.signs_alt, "mixed": D.signs_mixed}


def cyc_k(cw):
    return min(cw - 1, 7)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------------
# (width, n, k): the emulator's and the GPU variant tests' k = min(c - 1, 7) at a size that is no multiple of 2^k, and the shapes of the GPU
# reduction-form tests, where k = min(c - 1, log2 n) fills the whole bucket set (or its first n buckets)
CYC_SHAPES = [(cw, 300, cyc_k(cw)) for cw in WIDTHS] + [(15, 20000, 7), (8, 1 << 10, 7), (15, 1 << 14, 14), (17, 1 << 13, 13), (20, 1 << 14, 14)]


@pytest.mark.parametrize("cw,n,k", CYC_SHAPES)
def test_model_cyc_pairs_are_equal_and_cyc_cancel_pairs_opposite(cw, n, k):
    c = R.BN254_G1
    bits = c.r.bit_length()
    assert 1 <= k <= cw - 1
    s = D.cyc(n, k)
    filled = min(1 << k, n)                       # buckets that hold anything
    pairs = filled // 2
    assert pairs == (1 << (k - 1) if n >= 1 << k else n // 2) and pairs >= 1
    a = max(n >> k, 1)
    m = D.bucket_mults(c.r, s, D.signs_plus(n), cw, bits)
    assert all(not mw for mw in m[1:]) and sorted(m[0]) == list(range(1, filled + 1))      # window 0 only, digits 1 .. filled
    assert all(m[0][2 * j + 1] == m[0][2 * j + 2] == a for j in range(pairs))              # every level-0 pair: aP + aP
    m = D.bucket_mults(c.r, s, D.signs_alt(n), cw, bits)
    assert all(not mw for mw in m[1:]) and sorted(m[0]) == list(range(1, filled + 1))
    assert all(m[0][2 * j + 1] == a and m[0][2 * j + 2] == c.r - a for j in range(pairs))  # aP + (-aP)
    plus, alt = D.cyc_total(n, k)
    assert alt == -a * pairs and alt % c.r != 0 and plus % c.r != 0                        # the total is not the identity


@pytest.mark.parametrize("c", list(R.CURVES.values()), ids=lambda c: c.name)
@pytest.mark.parametrize("cw", WIDTHS)
def test_model_heavy_fills_one_bucket_per_window(cw, c):
    bits = c.r.bit_length()
    digits = D.signed_digits(D.heavy_scalar(c), cw, bits)
    assert sum(1 for d in digits if d) > len(digits) // 2        # a full-width scalar: most windows take part
    for n in (300, 301):
        m = D.bucket_mults(c.r, D.heavy(c, n), D.signs_plus(n), cw, bits)
        assert [len(mw) for mw in m] == [1 if d else 0 for d in digits]
        assert all(mw[abs(d)] == (n if d > 0 else c.r - n) for mw, d in zip(m, digits) if d)
        m = D.bucket_mults(c.r, D.heavy(c, n), D.signs_alt(n), cw, bits)
        assert [len(mw) for mw in m] == [1 if d else 0 for d in digits]
        want = {300: lambda d: 0, 301: lambda d: 1 if d > 0 else c.r - 1}[n]    # n even: every bucket cancels; n odd: one point survives
        assert all(mw[abs(d)] == want(d) for mw, d in zip(m, digits) if d)


@pytest.mark.parametrize("c", list(R.CURVES.values()), ids=lambda c: c.name)
@pytest.mark.parametrize("cw", WIDTHS)
def test_model_digit_edges_reach_every_boundary_in_every_window(cw, c):
    """In every window w < W - 1 where some scalar below r can have it, the set holds a digit exactly M, one exactly M + 1 (window plus carry;
    it recodes to -(M - 1) with carry 1) and, from window 1 on (window 0 receives no carry), a zero digit made by a carry into an all-ones
    window.  Below window W - 2 all three always fit; window W - 2 is bounded by r when the windows below the top one cover all of r's bits
    (c * (W - 1) == bits), so the condition there is computed, not assumed.  Below W - 2, M + 1 is also reached through a carry (all-M + 1)."""
    r, bits = c.r, c.r.bit_length()
    W, M, full = D.n_windows(cw, bits), 1 << (cw - 1), (1 << cw) - 1
    vals = D.digit_edges(cw, c)
    digs = [D.signed_digits(s, cw, bits) for s in vals]
    raws = [[(s >> (cw * w)) & full for w in range(W)] for s in vals]
    for w in range(W - 1):
        can_m, can_m1, can_zero = (M << (cw * w)) < r, ((M + 1) << (cw * w)) < r, w >= 1 and (1 << (cw * (w + 1))) - 1 < r
        if w < W - 2:
            assert can_m and can_m1 and (can_zero or w == 0)
        if can_m:
            assert any(d[w] == M for d in digs), w
        if can_m1:
            assert any(d[w] == -(M - 1) for d in digs), w
        if can_zero:
            assert any(d[w] == 0 and raw[w] == full for d, raw in zip(digs, raws)), w
        if 1 <= w < W - 2:
            assert any(d[w] == -(M - 1) and raw[w] == M for d, raw in zip(digs, raws)), w
    # the values next to r set r's top bit: the last window that holds scalar bits is exercised at its largest value
    assert any(s >> (bits - 1) for s in vals) and r - 1 in vals


def test_model_u64_edges_fit_their_declared_width():
    for cw in WIDTHS:
        for b in D.u64_widths(cw):
            vals = D.u64_edges(cw, b)
            assert (1 << b) - 1 in vals and all(0 <= v < 1 << b for v in vals)
            assert (1 << (cw - 1) in vals) == (cw - 1 < b)
            for v in vals:
                D.signed_digits(v, cw, b)            # the final carry is zero within ceil((b + 1) / c) windows


# ---------------------------------------------------------------------------------------------------------------------------------------
# the emulator
# ---------------------------------------------------------------------------------------------------------------------------------------
def families(c, n, cw, keys=("plus", "alt")):
    """[(name, scalars as integers, rank-one signs)]: cyc and heavy over the all-+P key, cyc_cancel and heavy+- over the alternating one"""
    out = []
    for key in keys:
        out.append((f"cyc({cyc_k(cw)})/{key}", D.cyc(n, cyc_k(cw)), KEYS[key](n)))
        out.append((f"heavy/{key}", D.heavy(c, n), KEYS[key](n)))
    return out


def edge_vectors(cw, c, n):
    """the digit-edge set as ONE vector: tiled to n, or, where the set is longer than n, the set itself (the emulation of a wide bucket
    array takes seconds per run whatever n is)"""
    vals = D.digit_edges(cw, c)
    return D.tile(vals, max(n, len(vals)))




def check_rank_one(runner, c, n, cw):
    for name, s, signs in families(c, n, cw):
        got = runner(D.rows32(s), D.rank_one_key(c, n, signs), n)
        assert got == (0,) + D.expect(c, s, signs), (name, cw, n)
    if n == SIZES[0]:            # heavy+- with n odd: one point survives
        m = n - 1
        got = runner(D.rows32(D.heavy(c, m)), D.rank_one_key(c, m, D.signs_alt(m)), m)
        assert got == (0,) + D.expect(c, D.heavy(c, m), D.signs_alt(m)) and got[2] == 0, ("heavy+-, n odd", cw, m)
    s = edge_vectors(cw, c, n)
    got = runner(D.rows32(s), D.multiples_key(c, len(s)), len(s))
    assert got == (0,) + D.expect(c, s, D.multiples_coeffs(len(s))), ("digit edges", cw, n)


@pytest.mark.parametrize("c", EMUL_CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cw", PLAIN_WIDTHS)
def test_emul_plain_msm_on_rank_one_keys_and_digit_edges(emul, cw, n, c):  # noqa: F811
    """msm_pipeline over plain keys (one bucket set per window) at a forced window width: AccumFn's runs add P + P and P + (-P)
    (add_affine_signed), the folds and the pair tree add equal and opposite XYZZ points (XYZZ::add), the host tail combines windows
    whose sums are multiples of one point."""
    check_rank_one(lambda s, key, m: run(emul, c.cid, s, key, m, force_c=cw), c, n, cw)


@pytest.mark.parametrize("c", EMUL_CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cw", TABLE_WIDTHS)
def test_emul_table_msm_on_rank_one_keys_and_digit_edges(emul, cw, n, c):  # noqa: F811
    """The same over window tables (PrecompFn: row w of a rank-one key is +-2^(cw) P, so all windows still feed multiples of one point into
    ONE bucket set; the compile-time digit loops for c = 8 / 15 / 16 and the run-time one for 11 / 17)."""
    check_rank_one(lambda s, key, m: run_pre(emul, c.cid, s, key, m, 0, m, cw), c, n, cw)


@pytest.mark.parametrize("n", SIZES)
def test_emul_identity_rows_between_opposite_points(emul, n):  # noqa: F811
    """The mixed key (+P, -P, identity, ...): the digit stage drops the identity rows, and what is left of a heavy bucket alternates
    P + (-P) with an odd or even count per piece."""
    c = R.BN254_G1
    for cw in (8, 13):
        for name, s, signs in families(c, n, cw, keys=("mixed",)):
            key = D.rank_one_key(c, n, signs)
            rc, got, inf = run(emul, c.cid, D.rows32(s), key, n, force_c=cw)
            assert rc == 0 and (got, inf) == D.expect(c, s, signs), ("plain", name, cw)
            if cw == 8:
                rc, got, inf = run_pre(emul, c.cid, D.rows32(s), key, n, 0, n, cw)
                assert rc == 0 and (got, inf) == D.expect(c, s, signs), ("tables", name, cw)


@pytest.mark.parametrize("c", EMUL_CURVES, ids=lambda c: c.name)
def test_emul_digit_edges_over_distinct_points(emul, c):  # noqa: F811
    """The digit-edge set of every width over distinct points against the oracle's MSM: a wrong digit cannot hide behind the key's rank."""
    for cw in sorted(set(PLAIN_WIDTHS + TABLE_WIDTHS)):
        vals = D.digit_edges(cw, c)
        n = len(vals)
        bases = cref.sequential_bases(c, 900 + cw, n)
        sc = D.rows32(vals)
        exp = cref.msm(c.cid, sc, bases, n)
        if cw in PLAIN_WIDTHS:
            rc, got, inf = run(emul, c.cid, sc, bases, n, force_c=cw)
            assert rc == 0 and (got, inf) == exp, ("plain", cw)
        if cw in TABLE_WIDTHS:
            rc, got, inf = run_pre(emul, c.cid, sc, bases, n, 0, n, cw)
            assert rc == 0 and (got, inf) == exp, ("tables", cw)


def test_emul_u64_edges(emul):  # noqa: F811
    """msm_small_with_max_num_bits semantics at the declared widths 1, c - 1, c, c + 1, 63, 64: 2^b - 1, M and M + 1 in a scalar whose
    window count follows b, over the multiples key (plain keys on BN254, tables on Pallas: u64 scalars do not depend on r).  This is where
    the comparison d > M itself is pinned: for a field scalar, d >= M would be another correct recoding (-M and a carry), because the top
    window of a scalar below r never reaches M; with b + 1 a multiple of c (b = 63 at c = 8 / 16) the top window of 2^b - 1 does, and the
    carry out of it would be lost.  At c = 20,
    where every emulated run clears 2^19 buckets per window, only b = 1 (a window wider than the scalar) and b = 64."""
    n = 64
    for c, widths, tables in ((R.BN254_G1, PLAIN_WIDTHS, False), (R.PALLAS, TABLE_WIDTHS, True)):
        key, coeffs = D.multiples_key(c, n), D.multiples_coeffs(n)
        for cw in widths:
            for b in D.u64_widths(cw) if cw < 20 else (1, 64):
                s = D.tile(D.u64_edges(cw, b), n)
                sc = np.array(s, np.uint64)
                if tables:
                    rc, got, inf = run_pre(emul, c.cid, sc, key, n, 0, n, cw, u64_bits=b)
                else:
                    rc, got, inf = run(emul, c.cid, sc, key, n, force_c=cw, u64_bits=b)
                assert rc == 0 and (got, inf) == D.expect(c, s, coeffs), (tables, cw, b)
