"""What every opening argument goes through, on the GPU at its edges: nmx_eq_evals_from_points (the direct form up to ell = 12, the
split form from 13 to 24), nmx_mle_evaluate / nmx_mle_multi_evaluate (host operands through k_eq_sums / k_eq_rows; HBM operands through
the one-block pass k_sc_small up to ell = 8 and k_eq_rows from 9, results through the mailbox), nmx_poly_eval_multi and
nmx_field_batch_invert (the host level alone up to 128 elements, one and two device levels above).  Fixtures and expectations:
tests/eval_edges_common.py (Python big integers; tests/test_eval_edges.py checks them, and the functors with limb bounds asserted, on the
CPU).  All four fields unless said otherwise, the canonical and the Montgomery layout, host and HBM operands; words >= p are handed
over as they are.  Every assertion is byte equality, or an error code.

NOT run here: ell >= 25 of nmx_eq_evals_from_points, the doubling form -- a table of 1 GiB and more; EqStepFn chained to ell = 10 in
tests/test_eval_edges.py stands for it.  The 16- and 32-element chunks of batch_invert start at 2^21 and 2^23 elements and stay with
tests/test_gpu_fieldvec_large.py."""
import ctypes
import functools

import numpy as np
import pytest

from tests import eval_edges_common as X
from tests import fv_common as C

pytestmark = pytest.mark.gpu

FIDS = sorted(C.FIELDS)
LAYOUTS = pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
EMPTY = np.zeros((0, 32), np.uint8)


def dev(v):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(v).copy()).cuda()
    torch.cuda.synchronize()
    return t


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def vec(words):
    return C.vec(words) if len(words) else EMPTY


def same(got, want_ints, what):
    g, w = host(got).tobytes(), vec(want_ints).tobytes()
    if g != w:
        gi = C.ints(np.frombuffer(g, np.uint8))
        bad = [i for i, (a, b) in enumerate(zip(gi, want_ints)) if a != b]
        raise AssertionError("%s: %d of %d elements differ, first at %s" % (what, len(bad), len(want_ints), bad[:6]))


def word(b):
    return int.from_bytes(bytes(b), "little")


def flags(mont, device=False):
    from nova_amd import _lib as L
    return (L.SCALARS_MONT if mont else 0) | (L.SCALARS_DEVICE if device else 0)


def code_of(fn):
    from nova_amd import NmxError
    with pytest.raises(NmxError) as e:
        fn()
    return e.value.code


# ---- eq tables ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIDS)
def test_eq_tables_of_every_pattern_either_side_of_the_direct_and_the_split_form(nmx, fid):
    """ell 0, 1, 2, 11, 12: EqDirectFn; 13, 14: EqSplit2Fn + EqProductFn (ellL 7, ellR 6 and 7, 7); 15 (8, 7) with two patterns.  Both
    layouts (the Montgomery ONE is 2^256 mod p); the table lands in host memory and in HBM."""
    from nova_amd import fieldvec as fv
    for ell in (0, 1, 2, 11, 12, 13, 14, 15):
        for pat in (X.CHALLENGE_PATTERNS if ell < 15 else ("random", "alt01")):
            r = X.point(fid, pat, ell)
            for mont in (False, True):
                rw = vec(X.point_words(fid, r, mont))
                want = X.expect_eq(fid, r, mont)
                same(fv.eq_evals_from_points(fid, rw, mont=mont), want, "host ell=%d %s mont=%s" % (ell, pat, mont))
                same(fv.eq_evals_from_points(fid, rw, mont=mont, device=True), want, "hbm ell=%d %s mont=%s" % (ell, pat, mont))


@LAYOUTS
@pytest.mark.parametrize("fid", [1, 3])
def test_eq_table_of_2_to_the_24_is_non_zero_at_exactly_the_1024_known_indices(nmx, fid, mont):
    """the last split form (ellL = ellR = 12), in HBM (512 MiB): fourteen coordinates are zeros and ones, so the table is non-zero at
    1024 indices -- seven bits of the left table's index and seven of the right one's are pinned"""
    import torch
    from nova_amd import fieldvec as fv
    r = X.pinned_point(fid)
    idx = X.pinned_support(r)
    t = fv.eq_evals_from_points(fid, vec(X.point_words(fid, r, mont)), mont=mont, device=True)
    assert tuple(t.shape) == (1 << 24, 32)
    nonzero = int((t.view(torch.int64) != 0).any(dim=1).sum().item())
    got = t[torch.tensor(idx, device=t.device)]
    del t
    same(got, X.expect_eq_at(fid, r, idx, mont), "the 1024 entries")
    assert nonzero == 1024


@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_eq_table_errors_leave_out_untouched(nmx, fid, mont):
    import torch
    from nova_amd import _lib as L
    lib, p = L.lib(), C.FIELDS[fid]
    r31 = vec([1] * 31)
    out = np.full(64, 0xAB, np.uint8)
    assert lib.nmx_eq_evals_from_points(fid, r31.ctypes.data, 31, flags(mont), out.ctypes.data) == L.E_ARG and (out == 0xAB).all()
    for ell in (5, 13):            # one of each form
        for bad in (p, X.M256):
            for at in (0, ell - 1):
                rw = X.point_words(fid, X.point(fid, "random", ell), mont)
                rw[at] = bad
                rv = vec(rw)
                out = np.full(32 << ell, 0xAB, np.uint8)
                assert lib.nmx_eq_evals_from_points(fid, rv.ctypes.data, ell, flags(mont), out.ctypes.data) == L.E_SCALAR_RANGE, (ell, at)
                assert (out == 0xAB).all(), (ell, at)
                d = torch.full((1 << ell, 32), 0xAB, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                assert lib.nmx_eq_evals_from_points(fid, rv.ctypes.data, ell, flags(mont, True), d.data_ptr()) == L.E_SCALAR_RANGE, (ell, at)
                assert bool((d == 0xAB).all().item()), (ell, at)
    # ... and the library works afterwards
    from nova_amd import fieldvec as fv
    r = X.point(fid, "random", 5)
    same(fv.eq_evals_from_points(fid, vec(X.point_words(fid, r, mont)), mont=mont), X.expect_eq(fid, r, mont), "after the errors")


# ---- MLE evaluation -----------------------------------------------------------------------------------------------------------------
MLE_ELLS = (0, 1, 2, 3, 6, 7, 8, 9, 10)
MLE_POINTS = ("alt01", "ones", "pm1", "random")


@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_mle_evaluate_host_and_hbm_operands_give_the_integer(nmx, fid, mont):
    """ell = 0: one entry; 1: a one-entry right table (mask 0); up to 8: HBM operands run one block of k_sc_small; from 9: k_eq_rows.
    Words >= p (max, edge_cycle) are read mod p on both paths.  The HBM operand is exactly len rows and is left as it was."""
    from nova_amd import fieldvec as fv
    p = C.FIELDS[fid]
    for ell in MLE_ELLS:
        n = 1 << ell
        for opat in X.OPERAND_PATTERNS:
            z = X.operand(fid, opat, n, ell)
            zh = vec(z)
            zd = dev(zh)
            for cpat in MLE_POINTS:
                r = X.point(fid, cpat, ell)
                rw = vec(X.point_words(fid, r, mont))
                want = X.expect_mle(fid, z, r, mont)
                if cpat in ("alt01", "ones"):
                    assert want == z[X.indicator_index(r)] % p
                assert word(fv.mle_evaluate(fid, zh, rw, mont=mont)) == want, ("host", ell, opat, cpat)
                assert word(fv.mle_evaluate(fid, zd, rw, mont=mont)) == want, ("hbm", ell, opat, cpat)
            assert tuple(zd.shape) == (n, 32) and host(zd).tobytes() == zh.tobytes(), ("operand changed", ell, opat)


def _distinct_operands(fid, k, n):
    """k pairwise different operands: the three constant patterns, then edge cycles and random words from different seeds"""
    fixed = [("pm1", 0), ("max", 0), ("last_only", 0)]
    picks = [fixed[j] if j < 3 else (("edge_cycle", j // 2) if j & 1 else ("random", j)) for j in range(k)]
    return [X.operand(fid, pat, n, seed) for pat, seed in picks]


@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_mle_multi_evaluate_fills_every_slot_and_a_second_pass(nmx, fid, mont):
    """k = 1, 16 (every mailbox slot), 17 (a second pass of one) HBM polynomials at ell = 3 (k_sc_small) and 9 (k_eq_rows): pairwise
    different operands, so a result in the wrong slot fails; each equals the single call and the integer.  Host operands too."""
    from nova_amd import fieldvec as fv
    for ell in (3, 9):
        n = 1 << ell
        zs = _distinct_operands(fid, 17, n)
        assert len(set(zs)) == 17
        zh = [vec(z) for z in zs]
        zd = [dev(z) for z in zh]
        for cpat in ("random", "pm1"):
            r = X.point(fid, cpat, ell)
            rw = vec(X.point_words(fid, r, mont))
            want = [X.expect_mle(fid, z, r, mont) for z in zs]
            assert len(set(want)) > 12
            single = [word(fv.mle_evaluate(fid, z, rw, mont=mont)) for z in zd]
            assert single == want, (ell, cpat, "single calls")
            for k in (1, 16, 17):
                assert [word(b) for b in fv.mle_multi_evaluate(fid, zd[:k], rw, mont=mont)] == want[:k], ("hbm", ell, cpat, k)
                assert [word(b) for b in fv.mle_multi_evaluate(fid, zh[:k], rw, mont=mont)] == want[:k], ("host", ell, cpat, k)
        for a, b in zip(zd, zh):
            assert host(a).tobytes() == b.tobytes(), "operand changed"


@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_mle_evaluate_errors(nmx, fid, mont):
    from nova_amd import _lib as L
    from nova_amd import fieldvec as fv
    lib, p = L.lib(), C.FIELDS[fid]
    z = X.operand(fid, "random", 8)
    zh = vec(z)
    zd = dev(zh)
    r = X.point(fid, "random", 3)
    rw = vec(X.point_words(fid, r, mont))
    for operand, ptr, device in ((zh, zh.ctypes.data, False), (zd, zd.data_ptr(), True)):
        out = np.full(64, 0xAB, np.uint8)
        for bad_len in (7, 9, 4, 16):
            assert lib.nmx_mle_evaluate(fid, ptr, bad_len, rw.ctypes.data, 3, flags(mont, device), out.ctypes.data) == L.E_ARG
            ptrs = (ctypes.c_void_p * 1)(ptr)
            assert lib.nmx_mle_multi_evaluate(fid, ptrs, 1, bad_len, rw.ctypes.data, 3, flags(mont, device), out.ctypes.data) == L.E_ARG
        for bad in (p, X.M256):
            for at in (0, 2):
                bw = X.point_words(fid, r, mont)
                bw[at] = bad
                assert code_of(lambda: fv.mle_evaluate(fid, operand, vec(bw), mont=mont)) == L.E_SCALAR_RANGE
                assert code_of(lambda: fv.mle_multi_evaluate(fid, [operand, operand], vec(bw), mont=mont)) == L.E_SCALAR_RANGE
                bv = vec(bw)
                assert lib.nmx_mle_evaluate(fid, ptr, 8, bv.ctypes.data, 3, flags(mont, device), out.ctypes.data) == L.E_SCALAR_RANGE
        assert (out == 0xAB).all()
        # the library works afterwards
        assert word(fv.mle_evaluate(fid, operand, rw, mont=mont)) == X.expect_mle(fid, z, r, mont)


# ---- poly_eval_multi ----------------------------------------------------------------------------------------------------------------
EVAL_LENS = (1, 16, 17, 4096, 4097, 0, 4096 * 33 + 7, 4096 * 64)   # blocks 0..33 and 0..63 of the last two: bits 0..5 of the block index


@pytest.fixture(scope="module")
def eval_expect():
    """Horner over the words mod p, shared by the layouts (tests/eval_edges_common.py: expect_eval)"""
    memo = {}

    def get(fid, pat, n, u):
        key = (fid, pat, n, u)
        if key not in memo:
            memo[key] = X.expect_eval(fid, X.operand(fid, pat, n, 3), u, False)
        return memo[key]
    return get


@functools.lru_cache(maxsize=None)
def _poly(fid, pat, n):
    a = vec(X.operand(fid, pat, n, 3))
    a.setflags(write=False)
    return a


@LAYOUTS
@pytest.mark.parametrize("pat", ["pm1", "max", "edge_cycle"])
@pytest.mark.parametrize("fid", FIDS)
def test_poly_eval_multi_lengths_around_the_chunk_and_the_block_and_block_powers_to_bit_5(nmx, eval_expect, fid, pat, mont):
    from nova_amd import fieldvec as fv
    p = C.FIELDS[fid]
    us = X.eval_points(fid)
    pts = vec([X.challenge_word(p, u, mont) for u in us])
    polys = [_poly(fid, pat, n) for n in EVAL_LENS]
    want = [[eval_expect(fid, pat, n, u) for u in us] for n in EVAL_LENS]
    assert want[5] == [0, 0, 0, 0]
    for where, ops in (("host", polys), ("hbm", [dev(f) if len(f) else f for f in polys])):
        got = fv.poly_eval_multi(fid, ops, pts, mont=mont)
        assert [[word(b) for b in row] for row in got] == want, where
    # m = 1, 2, 3 with a repeated point
    small = [polys[i] for i in (2, 4, 5)]
    for sel in ((3,), (3, 3), (2, 3, 2)):
        got = fv.poly_eval_multi(fid, small, vec([X.challenge_word(p, us[j], mont) for j in sel]), mont=mont)
        assert [[word(b) for b in row] for row in got] == [[want[i][j] for j in sel] for i in (2, 4, 5)], sel


@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_poly_eval_multi_4096_short_polynomials_and_the_limits(nmx, fid, mont):
    """4096 polynomials of i mod 19 coefficients (empty ones included) at two points: the block search of k_eval_multi over 4096
    descriptors; one polynomial more, or a fifth point, is NMX_E_TOO_LARGE; a point >= p is NMX_E_SCALAR_RANGE with out untouched"""
    from nova_amd import _lib as L
    from nova_amd import fieldvec as fv
    lib, p = L.lib(), C.FIELDS[fid]
    k = 4096
    lens = [i % 19 for i in range(k)]
    offs = np.concatenate([[0], np.cumsum(lens)]).tolist()
    words = X.operand(fid, "edge_cycle", offs[-1], 5)
    us = X.eval_points(fid)[2:]
    pts = vec([X.challenge_word(p, u, mont) for u in us])
    want = [[X.expect_eval(fid, words[offs[i]:offs[i + 1]], u, mont) for u in us] for i in range(k)]
    flat = vec(words)
    flat_d = dev(flat)
    for where, base in (("host", flat), ("hbm", flat_d)):
        got = fv.poly_eval_multi(fid, [base[offs[i]:offs[i + 1]] for i in range(k)], pts, mont=mont)
        assert [[word(b) for b in row] for row in got] == want, where
    one = [flat[:1]] * (k + 1)
    assert code_of(lambda: fv.poly_eval_multi(fid, one, pts, mont=mont)) == L.E_TOO_LARGE
    assert code_of(lambda: fv.poly_eval_multi(fid, one[:2], vec([1, 2, 3, 4, 5]), mont=mont)) == L.E_TOO_LARGE
    for bad in (p, X.M256):
        for at in (0, 1):
            bw = [X.challenge_word(p, u, mont) for u in us]
            bw[at] = bad
            bv = vec(bw)
            for base, device in ((flat, False), (flat_d, True)):
                ptr = base.data_ptr() if device else base.ctypes.data
                ptrs, ln = (ctypes.c_void_p * 2)(ptr, ptr + 32 * 40), (ctypes.c_size_t * 2)(40, 17)
                out = np.full(2 * 2 * 32 + 32, 0xAB, np.uint8)
                assert lib.nmx_poly_eval_multi(fid, ptrs, ln, 2, bv.ctypes.data, 2, flags(mont, device), out.ctypes.data) == L.E_SCALAR_RANGE
                assert (out == 0xAB).all()
    got = fv.poly_eval_multi(fid, [flat[:40]], pts, mont=mont)
    assert [word(b) for b in got[0]] == [X.expect_eval(fid, words[:40], u, mont) for u in us], "after the errors"


# ---- batch_invert -------------------------------------------------------------------------------------------------------------------
INVERT_NS = (1, 2, 127, 128, 129, 1023, 1024, 1025, 8193)   # the host level alone up to 128; one device level; two from 1025


@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_batch_invert_is_the_integer_inverse_at_every_size_and_for_every_word(nmx, fid, mont):
    """one contract either side of 128 elements: a word >= p is read mod p, every output is canonical"""
    from nova_amd import fieldvec as fv
    p = C.FIELDS[fid]
    for n in INVERT_NS:
        for pat in X.INVERT_PATTERNS:
            v = X.operand(fid, pat, n, n % 7, True)
            want = X.expect_inverse(fid, v, mont)
            assert want is not None and all(w < p for w in want)
            vh = vec(v)
            same(fv.batch_invert(fid, vh, mont=mont), want, "host n=%d %s" % (n, pat))
            vd = dev(vh)
            same(fv.batch_invert(fid, vd, mont=mont), want, "hbm n=%d %s" % (n, pat))
            assert host(vd).tobytes() == vh.tobytes(), "operand changed"


def _zero_positions(n):
    """first and last element of a full chunk, the last element of a ragged chunk, index 0 and index n - 1 (lane c of T = ceil(n / 8)
    lanes owns c, c + T, ...)"""
    T = (n + 7) // 8
    c = T - 1
    ragged_last = c + ((n - 1 - c) // T) * T
    assert 7 * T < n and (n - 1 - c) // T < 7 and T // 2 > 0
    return sorted({T // 2, 7 * T, ragged_last, 0, n - 1})


@LAYOUTS
@pytest.mark.parametrize("n", [100, 129, 1025])
@pytest.mark.parametrize("fid", FIDS)
def test_batch_invert_reports_every_word_that_is_zero_mod_p(nmx, fid, n, mont):
    """0, p, 2p (and 3p where it fits) are NMX_E_ZERO on the host level (n = 100) as behind one and two device levels; the next call
    succeeds"""
    from nova_amd import _lib as L
    from nova_amd import fieldvec as fv
    p = C.FIELDS[fid]
    base = list(X.operand(fid, "edge_cycle", n, 1, True))
    ok = vec(base[:3])
    ok_want = X.expect_inverse(fid, base[:3], mont)
    for at in _zero_positions(n):
        for z in X.zero_class(p):
            v = list(base)
            v[at] = z
            assert X.expect_inverse(fid, v, mont) is None
            vh = vec(v)
            for operand in (vh, dev(vh)):
                assert code_of(lambda: fv.batch_invert(fid, operand, mont=mont)) == L.E_ZERO, (at, hex(z))
                same(fv.batch_invert(fid, ok, mont=mont), ok_want, "the call after the error")
