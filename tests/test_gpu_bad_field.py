"""-m gpu: every C-ABI entry point that takes `int field` (enumerated from include/nova_mi355x.h), called with the field ids 4 and -1
and otherwise valid arguments of the smallest legal shape, returns NMX_E_ARG with a message; the same entry point called with a
valid field directly afterwards still returns the right answer -- a refused field id leaves nothing enqueued and no context
leased.  Shapes: vectors of 2 elements, 1 round, a 2 x 2 matrix with one entry (nmx_sumcheck_bind_eq_sums needs 4 elements: it
binds one variable and sums over the next)."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import cref
from tests import fv_common as C
from tests import spartan_common as sp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FID = 1  # BN254's scalar field
P = C.FIELDS[FID]


def entry_points_with_a_field():
    text = open(os.path.join(ROOT, "include", "nova_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", text), flags=re.S)
    return sorted(m.group(1) for m in re.finditer(r"\b(nmx_\w+)\s*\(([^;{]*?)\)\s*;", text, re.S)
                  if re.search(r"\bint\s+field\b", m.group(2)))


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def host(t):
    return t.cpu().numpy().tobytes()


a, b, c, e, e2 = (C.rand_vec(FID, 2, s) for s in (1, 2, 3, 4, 5))
a4, b4, c4 = (C.rand_vec(FID, 4, s) for s in (6, 7, 8))
r, eq1, eq2 = C.rand_vec(FID, 1, 9), C.rand_vec(FID, 1, 10), C.rand_vec(FID, 1, 11)


def _svec_map(f):
    from nova_amd import ShardedVector, _lib, svec_map
    vs = [ShardedVector.from_host(2, v) for v in (a, b)] + [ShardedVector(2, 2)]
    try:
        return svec_map(f, _lib.OP_AXPY, vs[:2], r, out=vs[2]).to_host().tobytes()
    finally:
        for v in vs:
            v.close()


def _bind_eq_sums(f):
    from nova_amd import fieldvec as fv
    oa, ob, oc, sums = fv.sumcheck_bind_eq_sums(f, 3, dev(a4), dev(b4), dev(c4), r, dev(eq1))
    return host(oa), host(ob), host(oc), sums


def _bind_eq_sums_expected():
    bound = [cref.field_bind(FID, X, 0, 2, 1, r, 2) for X in (a4, b4, c4)]
    return bound[0], bound[1], bound[2], cref.sumcheck_eq_sums(FID, 3, bound[0], bound[1], bound[2], 2, eq1)


def _nifs_fold(f):
    from nova_amd import fieldvec as fv
    w, ee = fv.nifs_fold(f, dev(a), dev(b), dev(c), dev(e), r)
    return host(w), host(ee)


def _register(f):
    """the 2 x 2 matrix [[0, 3], [0, 0]] times a"""
    from nova_amd import fieldvec as fv
    m = fv.SparseMatrix(f, [0, 1, 1], [1], C.vec([3]), 2)
    try:
        return m.multiply_vec(a).tobytes()
    finally:
        m.close()


def _fv(name, *args, out=lambda x: x.tobytes(), **kw):
    def call(f):
        from nova_amd import fieldvec as fv
        return out(getattr(fv, name)(f, *args, **kw))
    return call


def _prover(check, name, *args):
    """the prover's own check (tests/spartan_common.py: the reference's verifier on what it returns) is the right answer"""
    def call(f):
        from nova_amd import fieldvec as fv
        return check(lambda _fid, *x: getattr(fv, name)(f, *[v.copy() if isinstance(v, np.ndarray) else v for v in x]), FID, *args)
    return call


@functools.lru_cache(maxsize=None)
def cases():
    """entry point -> (call(field) -> result, the right answer for FID; None: the call checks itself)"""
    fold = cref.field_bind(FID, a, 0, 1, 2, r, 1)  # a[0] + r (a[1] - a[0])
    return {
        "nmx_svec_map": (_svec_map, cref.field_axpy(FID, a, b, r, 2)),
        "nmx_field_axpy": (_fv("axpy", a, b, r), cref.field_axpy(FID, a, b, r, 2)),
        "nmx_field_axpy2": (_fv("axpy2", a, b, c, r), cref.field_axpy2(FID, a, b, c, r, 2)),
        "nmx_field_cross_term": (_fv("cross_term", a, b, c, e, r), cref.field_cross_term(FID, a, b, c, e, r, 2)),
        "nmx_field_cross_term2": (_fv("cross_term2", a, b, c, e, e2, r), cref.field_cross_term2(FID, a, b, c, e, e2, r, 2)),
        "nmx_field_vec_add": (_fv("vec_add", a, b), C.vec([(x + y) % P for x, y in zip(C.ints(a), C.ints(b))]).tobytes()),
        "nmx_field_batch_invert": (_fv("batch_invert", a), C.vec([pow(x, -1, P) for x in C.ints(a)]).tobytes()),
        "nmx_field_concat": (_fv("concat", [a, r], out=host), a.tobytes() + r.tobytes()),
        "nmx_mle_bind_top": (_fv("bind_poly_var_top", a, r), cref.field_bind(FID, a, 0, 1, 1, r, 1)),
        "nmx_poly_fold_pairs": (_fv("fold_pairs", a, r), fold),
        "nmx_poly_fold_chain": (_fv("fold_chain", a, r, out=lambda outs: [o.tobytes() for o in outs]), [fold]),
        "nmx_sumcheck_eq_sums": (_fv("sumcheck_eq_sums", 3, a, b, c, eq1, eq2, 0, out=tuple),
                                 cref.sumcheck_eq_sums(FID, 3, a, b, c, 2, eq1, eq2, 0)),
        "nmx_sumcheck_bind_eq_sums": (_bind_eq_sums, _bind_eq_sums_expected()),
        "nmx_sumcheck_plain_sums": (_fv("sumcheck_plain_sums", 4, a, b, c, out=tuple), cref.sumcheck_plain_sums(FID, 4, a, b, c, 2)),
        "nmx_sumcheck_prove_cubic_with_three_inputs": (_prover(sp.check_cubic3, "sumcheck_prove_cubic_with_three_inputs", 1, 21), None),
        "nmx_sumcheck_prove_quad_prod": (_prover(sp.check_quad_prod, "sumcheck_prove_quad_prod", 1, 22), None),
        "nmx_sumcheck_prove_batch_eval": (_prover(sp.check_batch_eval, "sumcheck_prove_batch_eval", [1], 23), None),
        "nmx_field_lincomb_powers": (_fv("lincomb_powers", [a, b], r), cref.lincomb_powers(FID, [a.tobytes(), b.tobytes()], r, 2)),
        "nmx_poly_suffix_horner": (_fv("suffix_horner", a, r), cref.suffix_horner(FID, a, 2, r)),
        "nmx_poly_eval_multi": (_fv("poly_eval_multi", [a], r, out=lambda v: v), [[cref.suffix_horner(FID, a, 2, r)[:32]]]),
        "nmx_eq_evals_from_points": (_fv("eq_evals_from_points", r), cref.eq_evals(FID, r, 1)),
        "nmx_mle_evaluate": (_fv("mle_evaluate", a, r, out=bytes), cref.mle_evaluate(FID, a, 1, r)),
        "nmx_mle_multi_evaluate": (_fv("mle_multi_evaluate", [a, b], r, out=list), cref.mle_multi_evaluate(FID, [a.tobytes(), b.tobytes()], 1, r)),
        "nmx_spmv_register": (_register, C.vec([3 * C.ints(a)[1] % P, 0]).tobytes()),
        "nmx_nifs_fold": (_nifs_fold, (cref.field_axpy(FID, a, b, r, 2), cref.field_axpy(FID, c, e, r, 2))),
    }


@pytest.mark.parametrize("name", entry_points_with_a_field())
def test_bad_field_id_is_refused_and_the_next_call_is_right(nmx, name):
    from nova_amd import NmxError, _lib
    assert sorted(cases()) == entry_points_with_a_field()
    call, want = cases()[name]
    for bad in (4, -1):
        with pytest.raises(NmxError) as ei:
            call(bad)
        assert ei.value.code == _lib.E_ARG, (bad, ei.value)
        assert _lib.lib().nmx_last_error(), bad
    got = call(FID)
    if want is not None:
        assert got == want
