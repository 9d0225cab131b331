"""The dense field-vector calls and the three sum-check sum passes on the GPU at their value and lane edges, through nova_amd.fieldvec:
axpy, axpy2, cross_term, cross_term2, vec_add, bind_poly_var_top (also in place), fold_pairs, fold_chain, lincomb_powers, svec_map with
the output aliasing an operand, sumcheck_eq_sums (k_eq_sums and k_eq_rows, with the grid capped at one block by the option
eq_max_blocks so that a lane walks past its sixth pair, and at the default cap), sumcheck_bind_eq_sums and sumcheck_plain_sums.
Fixtures and expectations: tests/fieldvec_edges_common.py (Python big integers; tests/test_fieldvec_edges.py checks them, and the lane
bodies with limb bounds asserted, on the CPU).  All four fields, the canonical and the Montgomery layout, host and HBM operands; words
>= p are handed over as they are.  Every assertion is byte equality.

What stays with the CPU emulation: the `pending == 6` branch of k_bind_eq_sums (one index per lane below 2^20 indices, a hard cap of
4096 blocks above: it needs len > 2^24.6) and the pair loop's sixth turn in kinds 1 and 3 of k_plain_sums (>= 13 indices per lane under
a cap of 2048 blocks: len >= 2^24, which tests/test_gpu_fieldvec_large.py runs on random data)."""
import ctypes

import numpy as np
import pytest

from tests import fieldvec_edges_common as X
from tests import fv_common as C

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


def same(got, want_ints, what):
    g = C.ints(host(got))
    if g != list(want_ints):
        bad = [i for i, (a, b) in enumerate(zip(g, want_ints)) if a != b]
        raise AssertionError("%s: %d of %d elements differ, first at %s" % (what, len(bad), len(g), bad[:6]))
    assert host(got).tobytes() == C.vec(want_ints).tobytes(), what


def word(x):
    return int.from_bytes(bytes(x), "little")


def both(vecs):
    """the operand vectors as host arrays and as HBM tensors"""
    hs = [C.vec(v) for v in vecs]
    return ("host", hs), ("hbm", [dev(h) for h in hs])


def call_map(fv, name, fid, ops, r, mont):
    if name == "vec_add":
        return fv.vec_add(fid, *ops, mont=mont)
    return getattr(fv, name)(fid, *ops, r, mont=mont)


# ---- dense maps ---------------------------------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("name", ["axpy", "axpy2", "cross_term", "cross_term2", "vec_add"])
@pytest.mark.parametrize("fid", FIDS)
def test_maps_over_the_grids_and_every_challenge(nmx, fid, name, mont):
    from nova_amd import fieldvec as fv
    p = C.FIELDS[fid]
    k, has_c, _fn = X.MAPS[name]
    for nc in (False, True):
        g = X.grid(fid, k, nc)
        for where, ops in both(g):
            for c in (X.challenges(fid) if has_c else [0]):
                got = call_map(fv, name, fid, ops, C.vec([X.challenge_word(p, c, mont)]), mont)
                same(got, X.expect_map(name, fid, g, c, mont), "%s %s words>=p=%s c=%#x" % (name, where, nc, c))


@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_bind_and_fold_pairs_over_the_grids_and_every_challenge(nmx, fid, mont):
    from nova_amd import fieldvec as fv
    p = C.FIELDS[fid]
    for nc in (False, True):
        g = X.grid(fid, 2, nc)
        z, P = C.vec(X.bind_top_input(*g)), C.vec(X.fold_pairs_input(*g))
        for c in X.challenges(fid):
            r, want = C.vec([X.challenge_word(p, c, mont)]), X.expect_map("bind", fid, g, c, mont)
            same(fv.bind_poly_var_top(fid, z, r, mont=mont), want, "bind host %s %#x" % (nc, c))
            same(fv.bind_poly_var_top(fid, dev(z), r, mont=mont), want, "bind hbm %s %#x" % (nc, c))
            same(fv.bind_poly_var_top(fid, dev(z), r, mont=mont, in_place=True), want, "bind in place %s %#x" % (nc, c))
            same(fv.fold_pairs(fid, P, r, mont=mont), want, "fold_pairs host %s %#x" % (nc, c))
            same(fv.fold_pairs(fid, dev(P), r, mont=mont), want, "fold_pairs hbm %s %#x" % (nc, c))


@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_maps_at_lengths_around_the_block(nmx, fid, mont):
    """1, 255, 256, 257 output elements either side of the 256-lane block of k_launch (bind and fold: 2, 510, 512, 514 inputs)"""
    from nova_amd import fieldvec as fv
    p = C.FIELDS[fid]
    cs = X.challenges(fid)
    for n in (1, 255, 256, 257):
        for nc in (False, True):
            c = cs[(n + nc) % len(cs)] or cs[4]
            r = C.vec([X.challenge_word(p, c, mont)])
            for name in ("axpy", "axpy2", "cross_term", "cross_term2", "vec_add"):
                cols = X.shape_columns(fid, X.MAPS[name][0], n, nc)
                for where, ops in both(cols):
                    same(call_map(fv, name, fid, ops, r, mont), X.expect_map(name, fid, cols, c, mont), "%s %s n=%d %s" % (name, where, n, nc))
            cols = X.shape_columns(fid, 2, n, nc)
            want = X.expect_map("bind", fid, cols, c, mont)
            z, P = C.vec(X.bind_top_input(*cols)), C.vec(X.fold_pairs_input(*cols))
            same(fv.bind_poly_var_top(fid, z, r, mont=mont), want, "bind host n=%d" % n)
            same(fv.bind_poly_var_top(fid, dev(z), r, mont=mont, in_place=True), want, "bind in place n=%d" % n)
            same(fv.fold_pairs(fid, P, r, mont=mont), want, "fold_pairs host n=%d" % n)
            same(fv.fold_pairs(fid, dev(P), r, mont=mont), want, "fold_pairs hbm n=%d" % n)


@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_fold_chain_one_block_and_per_fold_launches(nmx, fid, mont):
    """4 and 2048 inputs: the one-block chain alone; 4096: one BindTopFn launch, then the chain"""
    from nova_amd import fieldvec as fv
    p = C.FIELDS[fid]
    cs = X.challenges(fid)
    for n in (4, 2048, 4096):
        for nc in (False, True):
            words = X.fold_pairs_input(*X.shape_columns(fid, 2, n // 2, nc))
            k = n.bit_length() - 1
            xs = [cs[(i + nc) % len(cs)] for i in range(k)]
            want = X.expect_fold_chain(fid, words, xs, mont)
            xw = C.vec([X.challenge_word(p, c, mont) for c in xs])
            for where, v in (("host", C.vec(words)), ("hbm", dev(C.vec(words)))):
                got = fv.fold_chain(fid, v, xw, mont=mont)
                assert len(got) == k
                for i in range(k):
                    same(got[i], want[i], "fold_chain %s n=%d fold %d words>=p=%s" % (where, n, i, nc))


@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_lincomb_powers_either_side_of_twenty_four_vectors(nmx, fid, mont):
    from nova_amd import fieldvec as fv
    p = C.FIELDS[fid]
    for k in (24, 25, 29):
        for fill in ("p-1", "max"):
            vecs = X.lincomb_vectors(fid, k, fill)
            for where, vs in both(vecs):
                for s in X.lincomb_weights(p):
                    got = fv.lincomb_powers(fid, vs, C.vec([X.challenge_word(p, s, mont)]), n_out=X.LINCOMB_N_OUT, mont=mont)
                    same(got, X.expect_lincomb(fid, vecs, s, X.LINCOMB_N_OUT, mont), "lincomb %s k=%d %s s=%#x" % (where, k, fill, s))


@pytest.mark.parametrize("fid", FIDS)
def test_svec_map_with_the_output_aliasing_each_operand(nmx, fid):
    """nmx_svec_map on one device: `out` may be any of the operands (a lane reads its element of every operand before it writes)"""
    from nova_amd import _lib
    p = C.FIELDS[fid]
    c = X.challenges(fid)[2]
    for name, op in (("axpy", _lib.OP_AXPY), ("axpy2", _lib.OP_AXPY2), ("cross_term", _lib.OP_CROSS_TERM), ("cross_term2", _lib.OP_CROSS_TERM2),
                     ("vec_add", _lib.OP_VEC_ADD)):
        k, has_c, _fn = X.MAPS[name]
        g = X.grid(fid, k)
        n = len(g[0])
        want = X.expect_map(name, fid, g, c if has_c else 0, False)
        for alias in range(k):
            sv = [nmx.ShardedVector.from_host(n, C.vec(col)) for col in g]
            try:
                nmx.svec_map(fid, op, sv, C.vec([c]) if has_c else None, out=sv[alias])
                same(sv[alias].to_host(), want, "%s out = operand %d" % (name, alias))
                for j in range(k):
                    if j != alias:
                        same(sv[j].to_host(), g[j], "%s operand %d untouched" % (name, j))
            finally:
                for v in sv:
                    v.close()


# ---- eq-factored sums ------------------------------------------------------------------------------------------------------------------
def eq_case(fid, tpat, epat, n, shift):
    """(A, B, C, eqR, eqL) as tuples of words; shift None: no left table"""
    h = n // 2
    A, B, Cc = (X.table(fid, tpat, n, w) for w in range(3))
    if shift is None:
        return A, B, Cc, X.eq_table(fid, epat, h), None
    return A, B, Cc, X.eq_table(fid, epat, 1 << shift, 2), X.eq_table(fid, epat, -(-h // (1 << shift)), 1)


def check_eq_sums(fv, fid, mont, n, shift, modes=(1, 2, 3)):
    for tpat, epat in X.SUM_CASES:
        A, B, Cc, eqR, eqL = eq_case(fid, tpat, epat, n, shift)
        hs = [C.vec(x) for x in (A, B, Cc, eqR)] + [None if eqL is None else C.vec(eqL)]
        ds = [None if x is None else dev(x) for x in hs]
        for mode in modes:
            want = X.expect_eq_sums(fid, mode, A, B, Cc, eqR, eqL, shift or 0, mont)
            for where, (a, b, c, r, l) in (("host", hs), ("hbm", ds)):
                got = fv.sumcheck_eq_sums(fid, mode, a, b, c, r, eq_left=l, shift=shift or 0, mont=mont)
                assert (word(got[0]), word(got[1])) == want, (where, n, shift, mode, tpat, epat)


@LAYOUTS
@pytest.mark.parametrize("shape", ["no_left_table", "shift3", "shift13"])
@pytest.mark.parametrize("fid", FIDS)
def test_eq_sums_one_block_walks_past_the_sixth_reduction(nmx, fid, shape, mont):
    """eq_max_blocks = 1: 13 indices per lane and one odd index (k_eq_sums: pending == 6, then the tail); shift 3: 13 rows per lane and a
    partial last row (k_eq_rows: pend_g); shift 13: K = 32 indices per lane and row (k_eq_rows: pend, mode 1 through Fp::dot)"""
    from nova_amd import _lib, fieldvec as fv
    L = _lib.lib()
    n, shift = {"no_left_table": (2 * (256 * 13 + 1), None), "shift3": (2 * (8 * 32 * 13 + 5), 3), "shift13": (1 << 15, 13)}[shape]
    assert L.nmx_set_option(b"eq_max_blocks", 1) == 0
    try:
        check_eq_sums(fv, fid, mont, n, shift)
    finally:
        assert L.nmx_set_option(b"eq_max_blocks", 0) == 0


@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_eq_sums_at_lengths_around_the_block(nmx, fid, mont):
    from nova_amd import fieldvec as fv
    for n in (2, 510, 512, 514):
        check_eq_sums(fv, fid, mont, n, None)
        check_eq_sums(fv, fid, mont, n, 3)


# ---- bind + eq sums -----------------------------------------------------------------------------------------------------------------------
def bind_eq_sums_out_of_place(fid, mode, tabs, r, eqR, mont):
    """nmx_sumcheck_bind_eq_sums with outputs apart from the inputs (the Python wrapper binds in place): (bound tables, (t_0, t_inf))"""
    import torch
    from nova_amd import _lib
    from nova_amd.provider import _check
    n = tabs[0].numel() // 32
    outs = [torch.zeros((n // 2, 32), dtype=torch.uint8, device="cuda") if m < mode else None for m in range(3)]
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    res = np.zeros(64, np.uint8)
    rr = np.ascontiguousarray(r)
    _check(_lib.lib().nmx_sumcheck_bind_eq_sums(fid, mode, *[ptr(t) if m < mode else None for m, t in enumerate(tabs)], n, rr.ctypes.data, None, 0,
                                                eqR.data_ptr(), eqR.numel() // 32, 0, _lib.SCALARS_DEVICE | (_lib.SCALARS_MONT if mont else 0),
                                                *[ptr(o) for o in outs], res.ctypes.data))
    return outs, (res[:32].tobytes(), res[32:].tobytes())


@LAYOUTS
@pytest.mark.parametrize("fid", FIDS)
def test_bind_eq_sums_bound_tables_and_sums(nmx, fid, mont):
    from nova_amd import fieldvec as fv
    p = C.FIELDS[fid]
    cs = X.challenges(fid)
    for n in (4, 8, 1020, 1024, 1028):
        for q, (tpat, epat) in enumerate(X.SUM_CASES):
            c = cs[(q + n) % len(cs)]
            r = C.vec([X.challenge_word(p, c, mont)])
            T = [X.table(fid, tpat, n, w, True) for w in range(3)]
            eqR = X.eq_table(fid, epat, n // 4)
            d_eq = dev(C.vec(eqR))
            for mode in (1, 2, 3):
                bound, sums = X.expect_bind_eq_sums(fid, mode, T[0], T[1], T[2], c, eqR, None, 0, mont)
                src = [dev(C.vec(t)) for t in T]
                outs, got = bind_eq_sums_out_of_place(fid, mode, src, r, d_eq, mont)
                assert (word(got[0]), word(got[1])) == sums, ("out of place", n, mode, tpat, epat)
                for m in range(mode):
                    same(outs[m], bound[m], "out of place n=%d mode %d %s table %d" % (n, mode, tpat, m))
                    same(src[m], T[m], "out of place: input %d untouched" % m)
                tabs = [dev(C.vec(t)) if m < mode else None for m, t in enumerate(T)]
                a, b, cc, got = fv.sumcheck_bind_eq_sums(fid, mode, tabs[0], tabs[1], tabs[2], r, d_eq, mont=mont)
                assert (word(got[0]), word(got[1])) == sums, ("in place", n, mode, tpat, epat)
                for m, t in enumerate((a, b, cc)[:mode]):
                    same(t, bound[m], "in place n=%d mode %d %s table %d" % (n, mode, tpat, m))


# ---- plain sums ---------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("kind", [1, 2, 3, 4])
@pytest.mark.parametrize("fid", FIDS)
def test_plain_sums_every_kind_and_pattern(nmx, fid, kind, mont):
    """2 .. 514: one block either side of 256 lanes; 4096 .. 8194: one and two blocks of eight indices per lane and one more -- kind 4
    (one index per turn) reaches its sixth term"""
    from nova_amd import fieldvec as fv
    for n in (2, 510, 512, 514, 4096, 4098, 8194):
        for tpat in X.TABLE_PATTERNS:
            A, B, Cc = (X.table(fid, tpat, n, w) for w in range(3))
            want = X.expect_plain_sums(fid, kind, A, B, Cc, mont)
            for where, (a, b, c) in both((A, B, Cc)):
                got = fv.sumcheck_plain_sums(fid, kind, a, b, c if kind == 4 else None, mont=mont)
                assert tuple(word(g) for g in got) == want, (where, n, tpat)
