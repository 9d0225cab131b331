"""The sparse-matrix kernels on the GPU at their class, operand and column-split edges, through the product entry points: SpmvFn
(multiply_vec, multiply_vec_many), SpmvPairFn (multiply_vec_pair), SpmvSegFn + k_spmv_heavy behind transposed_of
(multiply_vec_transposed, multiply_vec_many transposed), SpmvCrossFn (r1cs_cross_term) and k_r1cs_sat (nmx_r1cs_is_sat), with
SpmvClassifyFn and the coefficient conversion of registration in front of each.  Fixtures and expectations: tests/spmv_edges_common.py
(Python big integers; tests/test_spmv_edges.py checks them on the CPU).  All four fields; the canonical layout and the Montgomery
layout (matrix registered with mont=True, vectors converted with util.to_mont_scalars' formula, words >= p handed over as they
are).  Every assertion is byte equality."""
import random

import numpy as np
import pytest

from oracle import pyref as R
from tests import fv_common as C
from tests import r1cs_sat_common as S
from tests import spmv_edges_common as X
from tests import test_gpu_r1cs_sat as RS
from tests import util

pytestmark = pytest.mark.gpu

FIDS = sorted(C.FIELDS)
LAYOUTS = pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])


def dev(v):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(v).copy()).cuda()
    torch.cuda.synchronize()
    return t


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def register(m, mont):
    from nova_amd import fieldvec as fv
    data = util.to_mont_scalars(C.CURVE_WITH_SCALAR_FIELD[m.fid], m.data) if (mont and len(m.coeffs)) else m.data
    return fv.SparseMatrix(m.fid, m.indptr, m.indices, data, m.cols, mont=mont)


def words_in(p, words, mont):
    """operand words of a layout: values < p converted, words >= p as they are"""
    return X.mont_words(p, words) if mont else list(words)


def values_out(p, vals, mont):
    """canonical expected values -> the words the layout returns"""
    return [(v << 256) % p for v in vals] if mont else list(vals)


def same(got, want_ints, what, names=None):
    g = C.ints(host(got))
    if g != list(want_ints):
        bad = [i for i, (a, b) in enumerate(zip(g, want_ints)) if a != b]
        raise AssertionError("%s: %d elements differ, first at %s" % (what, len(bad), [names(i) if names else i for i in bad[:6]]))
    assert host(got).tobytes() == C.vec(want_ints).tobytes(), what


def small_fixtures(fid):
    """(matrix, operand words over its columns, row namer) -- the words >= p included"""
    z = X.ZVALS(C.FIELDS[fid])
    return [(X.grid_csr(fid), z, lambda r: X.grid_pair_name(fid, r)), (X.pileup_csr(fid, X.P_MINUS_1_COL), z, X.pileup_row_name),
            (X.pileup_csr(fid, X.ALL_ONES_COL), z, X.pileup_row_name)]


# ---- multiply_vec -----------------------------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_multiply_vec_every_class_word_and_row_length(nmx, fid, mont):
    p = C.FIELDS[fid]
    for m, z, names in small_fixtures(fid):
        w = words_in(p, z, mont)
        want = m.times(w)   # linear in the words in both layouts
        assert all(x < p for x in want)
        mat = register(m, mont)
        try:
            same(mat.multiply_vec(C.vec(w), mont=mont), want, "%s host" % m.name, names)
            same(mat.multiply_vec(dev(C.vec(w)), mont=mont), want, "%s hbm" % m.name, names)
        finally:
            mat.close()


@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_multiply_vec_on_the_column_length_matrices(nmx, fid, mont):
    p = C.FIELDS[fid]
    z = C.vec(words_in(p, X.column_z(fid), mont))
    for v in X.COLUMN_VARIANTS:
        m = X.column_lengths_csr(fid, v)
        want = values_out(p, X.column_expect_forward(fid, v), mont)
        mat = register(m, mont)
        try:
            same(mat.multiply_vec(z, mont=mont), want, "%s host" % m.name)
            same(mat.multiply_vec(dev(z), mont=mont), want, "%s hbm" % m.name)
        finally:
            mat.close()


# ---- multiply_vec_pair: SpmvPairFn has its own row loop ------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_multiply_vec_pair_accumulators_do_not_mix(nmx, fid, mont):
    p = C.FIELDS[fid]
    for m, z, names in small_fixtures(fid):
        edge = words_in(p, z, mont)
        rnd = words_in(p, C.ints(C.rand_vec(fid, m.cols, 77 + fid)), mont)
        want_e, want_r = m.times(edge), m.times(rnd)
        mat = register(m, mont)
        try:
            for up in (C.vec, lambda x: dev(C.vec(x))):
                o1, o2 = mat.multiply_vec_pair(up(edge), up(rnd), mont=mont)
                same(o1, want_e, "%s (edge, random)[0]" % m.name, names), same(o2, want_r, "%s (edge, random)[1]" % m.name, names)
                o1, o2 = mat.multiply_vec_pair(up(rnd), up(edge), mont=mont)
                same(o1, want_r, "%s (random, edge)[0]" % m.name, names), same(o2, want_e, "%s (random, edge)[1]" % m.name, names)
                o1, o2 = mat.multiply_vec_pair(up(edge), up(edge), mont=mont)
                same(o1, want_e, "%s (edge, edge)[0]" % m.name, names), same(o2, want_e, "%s (edge, edge)[1]" % m.name, names)
        finally:
            mat.close()


# ---- multiply_vec_transposed: the column cut and k_spmv_heavy ----------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_transposed_grid_every_class_times_every_word(nmx, fid, mont):
    p = C.FIELDS[fid]
    t, w = X.grid_T(fid), words_in(p, X.ZVALS(p), mont)
    want = t.transposed_times(w)
    assert want == X.grid_csr(fid).times(w)
    mat = register(t, mont)
    try:
        for up in (C.vec, lambda x: dev(C.vec(x))):
            for _ in range(2):   # the transposed form is built by the first call and cached
                same(mat.multiply_vec_transposed(up(w), mont=mont), want, "grid_T", lambda r: X.grid_pair_name(fid, r))
    finally:
        mat.close()


@LAYOUTS
@pytest.mark.parametrize("variant", X.COLUMN_VARIANTS)
@pytest.mark.parametrize("fid", FIDS)
def test_transposed_column_lengths_around_the_cut_and_the_block_sum(nmx, fid, variant, mont):
    p = C.FIELDS[fid]
    m = X.column_lengths_csr(fid, variant)
    canon = X.column_expect_transposed(fid, variant)
    assert canon[X.COLUMN_LENGTHS.index(0)] == 0, "the empty column gives zero"
    want = values_out(p, canon, mont)
    x = C.vec(words_in(p, X.column_x(fid, variant), mont))
    names = lambda j: "column %d of %d entries" % (j, X.COLUMN_LENGTHS[j])  # noqa: E731
    mat = register(m, mont)
    try:
        same(mat.multiply_vec_transposed(x, mont=mont), want, m.name + " host", names)
        dx = dev(x)
        for _ in range(2):
            same(mat.multiply_vec_transposed(dx, mont=mont), want, m.name + " hbm", names)
    finally:
        mat.close()


# ---- multiply_vec_many ---------------------------------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_multiply_vec_many_equals_the_single_calls(nmx, fid, mont):
    from nova_amd import fieldvec as fv
    p = C.FIELDS[fid]
    g = X.grid_csr(fid)
    small = [g, X.pileup_csr(fid, X.ALL_ONES_COL, g.cols, g.rows)]
    z = words_in(p, X.ZVALS(p), mont)
    xs = words_in(p, X.shape_words(fid, g.rows, 51 + fid), mont)
    big = [X.column_lengths_csr(fid, "general"), X.column_lengths_csr(fid, "classes")]
    xb = words_in(p, X.column_x(fid, "general"), mont)
    assert X.column_x(fid, "general") == X.column_x(fid, "classes")
    want_bt = [values_out(p, X.column_expect_transposed(fid, v), mont) for v in ("general", "classes")]
    mats_s, mats_b = [register(m, mont) for m in small], [register(m, mont) for m in big]
    try:
        for up in (lambda x: dev(C.vec(x)), C.vec):
            outs = fv.multiply_vec_many(mats_s, up(z), mont=mont)
            for m, mat, o in zip(small, mats_s, outs):
                same(o, m.times(z), "many forward " + m.name)
                assert host(o).tobytes() == host(mat.multiply_vec(up(z), mont=mont)).tobytes()
            outs = fv.multiply_vec_many(mats_s, up(xs), transposed=True, mont=mont)
            for m, mat, o in zip(small, mats_s, outs):
                same(o, m.transposed_times(xs), "many transposed " + m.name)
                assert host(o).tobytes() == host(mat.multiply_vec_transposed(up(xs), mont=mont)).tobytes()
            outs = fv.multiply_vec_many(mats_b, up(xb), transposed=True, mont=mont)
            for m, mat, o, want in zip(big, mats_b, outs, want_bt):
                same(o, want, "many transposed " + m.name)
                assert host(o).tobytes() == host(mat.multiply_vec_transposed(up(xb), mont=mont)).tobytes()
    finally:
        for mat in mats_s + mats_b:
            mat.close()


# ---- r1cs_cross_term: SpmvCrossFn ---------------------------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_cross_term_over_grid_and_pileup_matrices(nmx, fid, mont):
    from nova_amd import fieldvec as fv
    p = C.FIELDS[fid]
    rng = random.Random(900 + fid)
    g = X.grid_csr(fid)
    trio = [g, X.pileup_csr(fid, X.P_MINUS_1_COL, g.cols, g.rows), X.pileup_csr(fid, X.ALL_ONES_COL, g.cols, g.rows)]
    r_inv = pow(1 << 256, -1, p)
    e = [rng.randrange(p) for _ in range(g.rows)]                      # E and u stay canonical VALUES (< p), as the header requires
    r = [rng.randrange(p) for _ in range(g.cols)]
    z_any = words_in(p, X.ZVALS(p), mont)                              # words >= p included
    z_red = [w % p for w in z_any]
    z1 = [(a - b) % p for a, b in zip(z_red, r)]                       # z1 + z2 = z (mod p), both < p
    mats = [register(m, mont) for m in trio]
    try:
        for order in ((0, 1, 2), (2, 0, 1)):
            A, B, Cm = (trio[i] for i in order)
            hA, hB, hC = (mats[i] for i in order)
            prods = [[x * r_inv % p for x in m.times(z_any)] if mont else m.times(z_any) for m in (A, B, Cm)]   # the VALUES A z, B z, C z
            for u in (0, 1, p - 1, rng.randrange(p)):
                want = values_out(p, R.cross_term(p, prods[0], prods[1], prods[2], e, u), mont)
                dE, uu = dev(C.vec(values_out(p, e, mont))), C.vec(values_out(p, [u], mont))
                same(fv.r1cs_cross_term(hA, hB, hC, dev(C.vec(z_any)), None, dE, uu, mont=mont), want, "cross term, z2 = None, u = %#x" % u)
                same(fv.r1cs_cross_term(hA, hB, hC, dev(C.vec(z1)), dev(C.vec(r)), dE, uu, mont=mont), want, "cross term, z = z1 + z2, u = %#x" % u)
    finally:
        for mat in mats:
            mat.close()


# ---- r1cs_is_sat_relaxed / r1cs_is_sat: k_r1cs_sat -----------------------------------------------------------------------------------------------
def sat_instance(fid, strict):
    """grid x pile-up matrices of one shape (315 x 15; z = [W (12), u or 1, X (2)]), W and X holding 0, 1, p - 1, p - 2; relaxed: E := the
    residual; strict: C has one entry per row in the constant column, (A z)(B z)[row]"""
    p = C.FIELDS[fid]
    g = X.grid_csr(fid)
    n_io, n_w = 2, g.cols - 3
    W = C.vec((X.ZVALS(p)[:X.NONCANON_FROM] + [p - 2])[:n_w]).copy()
    Xv = C.vec([0, p - 2]).copy()
    assert {0, 1, p - 1, p - 2} <= set(C.ints(W)) and C.ints(W)[X.P_MINUS_1_COL] == p - 1
    A, B = g.triple, X.pileup_csr(fid, X.P_MINUS_1_COL, g.cols, g.rows).triple
    if strict:
        empty = (np.zeros(g.rows + 1, np.uint64), np.zeros(0, np.uint64), np.zeros((0, 32), np.uint8))
        inst = S.Instance(fid, g.rows, g.cols, n_io, [A, B, empty], W, Xv)
        az, bz, _cz = inst.products()
        inst.csr[2] = (np.arange(g.rows + 1, dtype=np.uint64), np.full(g.rows, n_w, np.uint64), C.vec([a * b % p for a, b in zip(az, bz)]))
        return inst
    inst = S.Instance(fid, g.rows, g.cols, n_io, [A, B, X.pileup_csr(fid, X.ALL_ONES_COL, g.cols, g.rows).triple], W, Xv,
                      u=C.rand_vec(fid, 1, 60 + fid).copy(), E=np.zeros((g.rows, 32), np.uint8))
    inst.E = C.vec(inst.residual()).copy()
    return inst


@pytest.mark.parametrize("dev_,mont", [(False, False), (True, True), (True, False), (False, True)], ids=["host-canonical", "hbm-montgomery", "hbm-canonical", "host-montgomery"])
@pytest.mark.parametrize("fid", FIDS)
def test_is_sat_relaxed_on_grid_and_pileup_matrices(nmx, RS_L, fid, dev_, mont):
    inst = sat_instance(fid, strict=False)
    rows = inst.rows
    assert inst.bad_rows() == (0, RS.NONE) and rows <= 400
    su = RS.Setup(nmx, inst)
    try:
        assert RS.call(RS_L, su, dev=dev_, mont=mont) == (0, 0, 0, RS.NONE), RS_L.nmx_last_error()
        for bumped in ((0,), (63,), (64,), (rows - 1,), (64, rows - 1), (0, 63)):
            bad = inst.copy()
            for j in bumped:
                S.bump(bad.E, j, 1 + j, inst.p)
            assert bad.bad_rows() == (len(bumped), bumped[0])
            _cw, ce = S.expected_commitments(bad, su.bases, su.h, su.r_W, su.r_E)   # the prover committed to the E it sent
            assert RS.call(RS_L, su, bad, dev=dev_, mont=mont, ce=ce) == (0, RS.EQ, len(bumped), bumped[0]), bumped
    finally:
        su.close()


@pytest.mark.parametrize("fid", FIDS)
def test_is_sat_strict_on_grid_and_pileup_matrices(nmx, RS_L, fid):
    inst = sat_instance(fid, strict=True)
    assert inst.bad_rows() == (0, RS.NONE)
    su = RS.Setup(nmx, inst, with_key=False)
    try:
        bad = S.corrupt_W(inst, X.P_MINUS_1_COL)      # the column every row of B gathers
        want = bad.bad_rows()
        assert want[0] >= 1
        for dev_, mont in ((False, False), (True, True)):
            assert RS.call(RS_L, su, dev=dev_, mont=mont) == (0, 0, 0, RS.NONE), RS_L.nmx_last_error()
            assert RS.call(RS_L, su, bad, dev=dev_, mont=mont) == (0, RS.EQ) + want
    finally:
        su.close()


@pytest.fixture(scope="module")
def RS_L(nmx):
    from nova_amd import _lib
    return _lib.lib()


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_shapes_either_side_of_a_block_and_empty_matrices(nmx, fid, mont):
    p = C.FIELDS[fid]
    for m in X.shape_csrs(fid):
        z = words_in(p, X.shape_words(fid, m.cols, 41 + fid), mont)
        z2 = words_in(p, C.ints(C.rand_vec(fid, m.cols, 43 + fid)), mont)
        x = words_in(p, X.shape_words(fid, m.rows, 45 + fid), mont)
        want, want2, want_t = m.times(z), m.times(z2), m.transposed_times(x)
        if m.name == "nnz0":
            assert want == [0] * m.rows and want_t == [0] * m.cols
        mat = register(m, mont)
        try:
            for up in (C.vec, lambda v: dev(C.vec(v))):
                same(mat.multiply_vec(up(z), mont=mont), want, m.name + " multiply_vec")
                o1, o2 = mat.multiply_vec_pair(up(z), up(z2), mont=mont)
                same(o1, want, m.name + " pair[0]"), same(o2, want2, m.name + " pair[1]")
                for _ in range(2):
                    same(mat.multiply_vec_transposed(up(x), mont=mont), want_t, m.name + " transposed")
        finally:
            mat.close()
