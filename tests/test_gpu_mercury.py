"""nmx_mercury_h_poly / nmx_mercury_divide_by_binomial on the GPU, byte for byte against tests/mercury_common (the reference's
compute_h_poly and divide_by_binomial restated line by line in Python integers, itself checked on the CPU by tests/test_mercury_abi.py):
shapes from 1 x 1 to 512 x 1024, the segment boundaries of the division under the option mercury_seg_rows, edge values, both forms,
host and HBM operands, NMX_ASYNC, the other three fields, a bad field id, overlapping HBM buffers, and steps 1-11 of
mercury.rs::prove chained in HBM with every debug identity of the reference.  Of those steps make_s_polynomial stays the caller's (a
vector of b elements): a seeded stand-in of that length takes s's place in the evaluation call.  The pairing check of `verify` is
outside this library and is not tested."""
import ctypes
import random

import numpy as np
import pytest

from tests import fv_common as fc
from tests import mercury_common as mc

pytestmark = pytest.mark.gpu
FID = 1                                            # BN254 Fr: Mercury's field
R256 = 1 << 256
SMALL = [(1, 1), (1, 4), (2, 1), (2, 4), (3, 5), (5, 3), (4, 64), (64, 4), (17, 65), (33, 63)]
REFERENCE = [(16, 16), (8, 16), (32, 32), (16, 32), (64, 64), (32, 64)]      # (b, b) and (b / 2, b)


@pytest.fixture(scope="module")
def L(nmx):
    from nova_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def fv(nmx):
    from nova_amd import fieldvec
    return fieldvec


def gpu(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def instance(p, n_rows, n_cols, seed, fill=None):
    rng = random.Random(seed)
    val = (lambda: fill) if fill is not None else (lambda: rng.choice([0, 1, p - 1]) if rng.random() < 0.1 else rng.randrange(p))
    return [val() for _ in range(n_rows * n_cols)], [val() for _ in range(n_cols)], rng.randrange(p)


_want = {}


def want(p, f, n_rows, n_cols, eq, alpha, key=None):
    """(h, q, g) of the restatement, computed once per instance"""
    if key is None or key not in _want:
        h = mc.compute_h_poly(p, f, eq, n_rows, n_cols)
        qw, g = mc.divide_by_binomial(p, f, n_rows, n_cols, alpha)
        res = (h, mc.q_in_abi_layout(qw, n_rows, n_cols), g)
        if key is None:
            return res
        _want[key] = res
    return _want[key]


def run(fv, fid, f, n_rows, n_cols, eq, alpha, device, mont=False, async_=False):
    """-> (h, q, g) as integer lists through the Python wrappers"""
    fvec, evec, av = fc.vec(f), fc.vec(eq), fc.vec([alpha])
    if device:
        fvec, evec = gpu(fvec), gpu(evec)
    h = fv.mercury_h_poly(fid, fvec, n_rows, n_cols, evec, mont=mont, async_=async_)
    q, g = fv.mercury_divide_by_binomial(fid, fvec, n_rows, n_cols, av, mont=mont, async_=async_)
    if async_:
        fv.sync()
    return fc.ints(host(h)), (fc.ints(host(q)) if n_rows > 1 else []), fc.ints(host(g))


# ---- shapes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows,n_cols", SMALL + REFERENCE)
def test_shapes_against_the_restatement(fv, n_rows, n_cols):
    p = fc.FIELDS[FID]
    f, eq, alpha = instance(p, n_rows, n_cols, 100 * n_rows + n_cols)
    w = want(p, f, n_rows, n_cols, eq, alpha)
    assert run(fv, FID, f, n_rows, n_cols, eq, alpha, device=True) == w
    fvec = fc.vec(f).copy()
    before = fvec.copy()
    assert run(fv, FID, f, n_rows, n_cols, eq, alpha, device=False) == w          # host operands: staged, the same bytes
    hq = fv.mercury_divide_by_binomial(FID, fvec, n_rows, n_cols, fc.vec([alpha]))
    assert (fvec == before).all() and fc.ints(hq[1]) == w[2], "host operands must be left untouched"


@pytest.mark.parametrize("n_cols", [2048, 2049])
def test_h_at_the_lds_threshold(fv, n_cols):
    """2048 columns: the table staged in exactly 64 KiB of dynamic LDS; 2049: the launch form that reads it from memory"""
    p = fc.FIELDS[FID]
    f, eq, alpha = instance(p, 2, n_cols, n_cols)
    assert run(fv, FID, f, 2, n_cols, eq, alpha, device=True) == want(p, f, 2, n_cols, eq, alpha)
    f5, eq5, _a = instance(p, 5, n_cols, n_cols + 1)                          # more rows than one block's four waves
    h = fv.mercury_h_poly(FID, gpu(fc.vec(f5)), 5, n_cols, gpu(fc.vec(eq5)))
    assert fc.ints(host(h)) == mc.compute_h_poly(p, f5, eq5, 5, n_cols)


def test_host_operands_of_h_are_left_untouched_and_any_256_bit_words_are_taken(fv):
    p = fc.FIELDS[FID]
    n_rows, n_cols = 6, 70
    f, eq, alpha = instance(p, n_rows, n_cols, 44)
    top = (1 << 256) - 1
    f[3], f[77], eq[0], eq[5], eq[69] = top, p, top, p, p + 1                  # words that are no field elements, in f and in eq_col
    fvec, evec = fc.vec(f).copy(), fc.vec(eq).copy()
    f0, e0 = fvec.copy(), evec.copy()
    h = fv.mercury_h_poly(FID, fvec, n_rows, n_cols, evec)
    assert (fvec == f0).all() and (evec == e0).all(), "host operands must be left untouched"
    w = want(p, [x % p for x in f], n_rows, n_cols, [x % p for x in eq], alpha)
    assert fc.ints(h) == w[0]
    assert run(fv, FID, f, n_rows, n_cols, eq, alpha, device=True) == w
    assert run(fv, FID, f, n_rows, n_cols, eq, alpha, device=False) == w


def test_the_odd_log_n_shape_at_2_to_the_19(fv):
    p = fc.FIELDS[FID]
    n_rows, n_cols = 512, 1024
    f, eq, alpha = instance(p, n_rows, n_cols, 19)
    w = want(p, f, n_rows, n_cols, eq, alpha, key="2^19")
    assert run(fv, FID, f, n_rows, n_cols, eq, alpha, device=True) == w
    mc.check_division(p, f, w[1], w[2], n_cols, alpha, 12345)
    mc.check_g_against_h_alpha(p, eq, w[2], w[0], alpha)


# ---- segment boundaries ----------------------------------------------------------------------------------------------------------------
def test_segment_boundaries_give_identical_bytes(fv, L):
    p = fc.FIELDS[FID]
    R_, n_cols = 4, 65
    try:
        for n_rows in (R_ - 1, R_, R_ + 1, 2 * R_, 2 * R_ + 1):
            f, eq, alpha = instance(p, n_rows, n_cols, 7 + n_rows)
            w = want(p, f, n_rows, n_cols, eq, alpha)
            for opt in (R_, 0, n_rows, 1, 3):
                assert L.nmx_set_option(b"mercury_seg_rows", opt) == 0
                assert run(fv, FID, f, n_rows, n_cols, eq, alpha, device=True)[1:] == w[1:], (n_rows, opt)
        # a shape whose default plan has several segments and a short top one (33 rows: 4-row segments), and more than one column block
        f, eq, alpha = instance(p, 33, 300, 5)
        w = want(p, f, 33, 300, eq, alpha)
        for opt in (0, 5, 32, 33, 1000):
            assert L.nmx_set_option(b"mercury_seg_rows", opt) == 0
            assert run(fv, FID, f, 33, 300, eq, alpha, device=True) == w, opt
    finally:
        assert L.nmx_set_option(b"mercury_seg_rows", 0) == 0


# ---- values ----------------------------------------------------------------------------------------------------------------------------
def test_edge_values(fv):
    p = fc.FIELDS[FID]
    n_rows, n_cols = 9, 70
    for fill in (0, p - 1, None):
        f, eq, _a = instance(p, n_rows, n_cols, 31, fill=fill)
        if fill is not None:
            eq = instance(p, n_rows, n_cols, 32)[1]
        for alpha in (0, 1, p - 1, 0x1234567890abcdef1234567890abcdef):
            assert run(fv, FID, f, n_rows, n_cols, eq, alpha, device=True) == want(p, f, n_rows, n_cols, eq, alpha), (fill, alpha)


def test_eq_col_built_as_the_reference_builds_it(fv):
    p = fc.FIELDS[FID]
    rng = random.Random(3)
    u_col = [rng.randrange(p) for _ in range(5)]
    n_rows, n_cols = 16, 32
    f = [rng.randrange(p) for _ in range(n_rows * n_cols)]
    eq_dev = fv.eq_evals_from_points(FID, fc.vec(u_col), device=True)         # EqPolynomial::new(u_col).evals()
    eq = fc.ints(host(eq_dev))
    assert eq == mc.eq_evals(p, u_col)
    h = fv.mercury_h_poly(FID, gpu(fc.vec(f)), n_rows, n_cols, eq_dev)
    assert fc.ints(host(h)) == mc.compute_h_poly(p, f, eq, n_rows, n_cols)


# ---- forms -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [True, False])
def test_montgomery_words(fv, device):
    p = fc.FIELDS[FID]
    n_rows, n_cols = 17, 65
    f, eq, alpha = instance(p, n_rows, n_cols, 55)
    m = lambda v: [x * R256 % p for x in v]  # noqa: E731
    w = want(p, f, n_rows, n_cols, eq, alpha)
    got = run(fv, FID, m(f), n_rows, n_cols, m(eq), alpha * R256 % p, device=device, mont=True)
    assert got == tuple(m(x) for x in w)


def test_async_then_a_synchronous_call(fv):
    p = fc.FIELDS[FID]
    n_rows, n_cols = 32, 64
    f, eq, alpha = instance(p, n_rows, n_cols, 66)
    w = want(p, f, n_rows, n_cols, eq, alpha)
    fd, ed = gpu(fc.vec(f)), gpu(fc.vec(eq))
    h = fv.mercury_h_poly(FID, fd, n_rows, n_cols, ed, async_=True)
    q, g = fv.mercury_divide_by_binomial(FID, fd, n_rows, n_cols, fc.vec([alpha]), async_=True)
    # the next synchronous call of this thread is ordered behind both: g(alpha) through the suffix Horner
    out = fv.suffix_horner(FID, g, fc.vec([alpha]))
    assert fc.ints(host(out))[0] == mc.UniPoly(w[2], p).evaluate(alpha)
    assert (fc.ints(host(h)), fc.ints(host(q)), fc.ints(host(g))) == w
    assert run(fv, FID, f, n_rows, n_cols, eq, alpha, device=True, async_=True) == w


@pytest.mark.parametrize("fid", [0, 2, 3])
def test_a_reference_shape_on_the_other_fields(fv, fid):
    p = fc.FIELDS[fid]
    f, eq, alpha = instance(p, 16, 32, 70 + fid)
    assert run(fv, fid, f, 16, 32, eq, alpha, device=True) == want(p, f, 16, 32, eq, alpha)


# ---- errors --------------------------------------------------------------------------------------------------------------------------------
def test_bad_field_then_a_valid_call(fv, L):
    from nova_amd import _lib
    p = fc.FIELDS[FID]
    f, eq, alpha = instance(p, 5, 9, 80)
    fd, ed, av = gpu(fc.vec(f)), gpu(fc.vec(eq)), fc.vec([alpha]).copy()
    import torch
    hd, qd, gd = (torch.zeros((n, 32), dtype=torch.uint8, device="cuda") for n in (5, 36, 9))
    fl = _lib.SCALARS_DEVICE
    for bad in (4, -1):
        assert L.nmx_mercury_h_poly(bad, fd.data_ptr(), 5, 9, ed.data_ptr(), fl, hd.data_ptr()) == _lib.E_ARG
        assert b"bad field id" in L.nmx_last_error()
        assert L.nmx_mercury_divide_by_binomial(bad, fd.data_ptr(), 5, 9, av.ctypes.data, fl, qd.data_ptr(), gd.data_ptr()) == _lib.E_ARG
        assert b"bad field id" in L.nmx_last_error()
        assert not hd.any() and not qd.any() and not gd.any()
        assert run(fv, FID, f, 5, 9, eq, alpha, device=True) == want(p, f, 5, 9, eq, alpha)


def test_overlapping_hbm_buffers_are_refused_and_nothing_is_written(fv, L):
    from nova_amd import _lib
    p = fc.FIELDS[FID]
    n_rows, n_cols = 6, 10
    f, eq, alpha = instance(p, n_rows, n_cols, 90)
    buf = gpu(np.concatenate([fc.vec(f), fc.vec(eq), np.full((80, 32), 0x5a, np.uint8)]))      # f [0, 60), eq [60, 70), free [70, 150)
    before = buf.cpu().numpy().copy()
    at = lambda i: buf.data_ptr() + 32 * i  # noqa: E731
    av = fc.vec([alpha]).copy()
    fl = _lib.SCALARS_DEVICE
    d = lambda q, g: L.nmx_mercury_divide_by_binomial(FID, at(0), n_rows, n_cols, av.ctypes.data, fl, q, g)  # noqa: E731
    h = lambda out: L.nmx_mercury_h_poly(FID, at(0), n_rows, n_cols, at(60), fl, out)  # noqa: E731
    for q, g in ((at(0), at(140)), (at(59), at(140)), (at(70), at(50)), (at(70), at(119)), (at(80), at(71))):
        assert d(q, g) == _lib.E_ARG and b"overlap" in L.nmx_last_error()
    for out in (at(0), at(59), at(55), at(60), at(69), at(66)):
        assert h(out) == _lib.E_ARG and b"overlap" in L.nmx_last_error()
    assert L.nmx_sync() == 0
    assert (buf.cpu().numpy() == before).all()
    assert d(at(70), at(120)) == 0 and h(at(130)) == 0                                # adjacent, not overlapping: fine
    got = fc.ints(buf.cpu().numpy())
    w = want(p, f, n_rows, n_cols, eq, alpha)
    assert (got[130:136], got[70:120], got[120:130]) == w and got[:70] == f + eq


# ---- steps 1-11 of mercury.rs::prove, chained in HBM -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [10, 11])
def test_prove_steps_chained_in_hbm(nmx, fv, log_n):
    from nova_amd import CommitmentEngine, CommitmentKey
    from oracle import cref
    p = fc.FIELDS[FID]
    rng = random.Random(1000 + log_n)
    squeeze = lambda: rng.randrange(1, p)  # noqa: E731  (the seeded stand-in for the transcript)
    N = 1 << log_n
    ck = CommitmentKey.generate(0, N)
    bases = ck.read(0, N)
    ce = CommitmentEngine(0)

    def commit_matches(dev_vec, py_vals):
        got = ce.commit(ck, dev_vec)
        v = fc.vec(py_vals)
        assert (got.xy, int(got.is_inf)) == cref.msm(0, v, bases[:len(py_vals)], len(py_vals))
    try:
        f = [rng.randrange(p) for _ in range(N)]
        point = [rng.randrange(p) for _ in range(log_n)]
        f_dev = gpu(fc.vec(f))
        ev = int.from_bytes(fv.mle_evaluate(FID, f_dev, fc.vec(point)), "little")
        assert ev == mc.dot(p, f, mc.eq_evals(p, point))
        pt = ([0] + point) if log_n % 2 else point                        # :919-923
        log_b = len(pt) // 2
        b, b_row = 1 << log_b, N >> log_b
        eq_row = mc.eq_evals(p, pt[:log_b])
        eq_col_dev = fv.eq_evals_from_points(FID, fc.vec(pt[log_b:]), device=True)
        eq_col = fc.ints(host(eq_col_dev))
        # 1-2: h and its commitment
        h_dev = fv.mercury_h_poly(FID, f_dev, b_row, b, eq_col_dev)
        h = fc.ints(host(h_dev))
        assert h == mc.compute_h_poly(p, f, eq_col, b_row, b)
        mc.check_h_against_eval(p, eq_row, h, ev)
        commit_matches(h_dev, h)
        # 3-5: alpha, q and g, their commitments
        alpha = squeeze()
        q_dev, g_dev = fv.mercury_divide_by_binomial(FID, f_dev, b_row, b, fc.vec([alpha]))
        q, g = fc.ints(host(q_dev)), fc.ints(host(g_dev))
        qw, gw = mc.divide_by_binomial(p, f, b_row, b, alpha)
        assert (q, g) == (mc.q_in_abi_layout(qw, b_row, b), gw)
        assert mc.trimmed(p, q) == mc.trimmed(p, qw)                       # what the reference commits to after trim()
        mc.check_division(p, f, q, g, b, alpha, squeeze())
        mc.check_g_against_h_alpha(p, eq_col, g, h, alpha)
        commit_matches(q_dev, q)
        commit_matches(g_dev, g)
        # 6-8: gamma, s (the caller's: a stand-in of b elements here) and d = g reversed, both of size b
        _gamma = squeeze()
        s = [rng.randrange(p) for _ in range(b)]
        d = list(reversed(g))
        s_dev, d_dev = gpu(fc.vec(s)), gpu(fc.vec(d))
        # 9-10: zeta and the eight evaluations (:1136-1159), one call per distinct domain size
        zeta = squeeze()
        zeta_inv = pow(zeta, -1, p)
        pts3 = fc.vec([zeta, zeta_inv, alpha])
        ev3 = fv.poly_eval_multi(FID, [g_dev, h_dev, s_dev, d_dev], pts3)
        ints3 = [[int.from_bytes(x, "little") for x in row] for row in ev3]
        for poly, row in zip((g, h, s, d), ints3):
            assert row == [mc.UniPoly(poly, p).evaluate(x) for x in (zeta, zeta_inv, alpha)]
        g_zeta = ints3[0][0]
        assert ints3[1][2] == mc.dot(p, eq_col, g)                         # h(alpha) = <eq_col, g>
        # 11: quot_f from calls that exist; out[0] == g(zeta) restates the reference's assert_eq!(rem, ZERO)
        zba = (pow(zeta, b, p) - alpha) % p
        quot_dev, rem = fv.mercury_quot_f(FID, f_dev, q_dev, fc.vec([zba]), fc.vec([zeta]))
        assert int.from_bytes(rem, "little") == g_zeta
        quot = fc.ints(host(quot_dev))
        want_quot, want_rem = mc.quot_f(p, f, mc.trimmed(p, q), zeta, b, alpha, g_zeta)
        assert quot == want_quot
        mc.check_quot_f(p, f, q, quot, want_rem, zeta, b, alpha, g_zeta, squeeze())
        commit_matches(quot_dev, quot)
    finally:
        ck.close()
