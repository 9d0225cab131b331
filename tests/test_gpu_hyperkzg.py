"""nmx_poly_lincomb_quotients and nmx_hyperkzg_prove on the GPU.
The quotient pass byte for byte against nmx_field_lincomb_powers + nmx_poly_suffix_horner per point and against the big-integer definition
(tests/hyperkzg_common.py); the one call against the composed sequence of the calls that existed before it (fold_chain, batch commitment,
poly_eval_multi, lincomb_powers, 3 x suffix Horner, batch commitment) under the same SHA3 transcript, against the yardstick's restatement
of EvaluationEngineTrait::prove (src/provider/hyperkzg.rs:926-1116) and against the reference's verifier up to the pairing (:1119-1230; with a
key made from a known tau, e(L, H) == e(R, tau_H) is L == tau R).  The pairing itself is outside this library and is not tested."""
import random
import threading

import numpy as np
import pytest

from oracle import pyref as R
from tests import fv_common as fc
from tests import hyperkzg_common as hk

pytestmark = pytest.mark.gpu
R256 = 1 << 256
W256 = (1 << 256) - 1
FIELD_OF_CURVE = {0: 1, 1: 0, 2: 3, 3: 2}


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


def rand_polys(p, lens, seed):
    rng = random.Random(seed)
    return [[rng.choice([0, 1, p - 1]) if rng.random() < 0.1 else rng.randrange(p) for _ in range(n)] for n in lens]


def as_vecs(polys, device):
    vs = [fc.vec(f).copy() if len(f) else np.zeros((0, 32), np.uint8) for f in polys]
    return [gpu(v) for v in vs] if device else vs


def composed_quotients(fv, fid, vecs, q, us, mont=False):
    """the parent's calls: B = lincomb_powers, then one suffix Horner per point"""
    B = fv.lincomb_powers(fid, vecs, fc.vec([q]), mont=mont)
    return [fc.ints(host(fv.suffix_horner(fid, B, fc.vec([u]), mont=mont))) for u in us]


def fused_quotients(fv, fid, vecs, q, us, mont=False, async_=False):
    outs = fv.lincomb_quotients(fid, vecs, fc.vec([q]), fc.vec(us), mont=mont, async_=async_)
    if async_:
        fv.sync()
    return [fc.ints(host(o)) for o in outs]


# ---- nmx_poly_lincomb_quotients --------------------------------------------------------------------------------------------------------
# lengths at the pass's chunk (4; 8 by option) and level sizes (16 chunks, 256 chunks) and one either side, one just above each size at which
# the launch plan gains a level (4, 64, 1024, 16384, 262144), ragged shapes, a first vector that is not the longest
SHAPES = [(1,), (3, 3), (4,), (5, 2, 5), (7, 3), (8, 8), (9, 2, 9), (63, 64), (65, 1), (127, 64), (128,), (129, 128, 1), (1023, 5), (1024, 512), (1025, 7),
          (2047, 5), (2048, 1024), (2049, 2049), (1000, 37, 999, 1, 0), (37, 1000), (16385, 100), (262145, 5)]


@pytest.mark.parametrize("lens", SHAPES)
def test_quotients_equal_the_composed_calls_and_the_definition(fv, lens):
    fid = 1
    p = fc.FIELDS[fid]
    rng = random.Random(sum(lens))
    polys = rand_polys(p, lens, len(lens) + lens[0])
    q, us = rng.randrange(p), [rng.randrange(p) for _ in range(3)]
    vecs = as_vecs(polys, True)
    got = fused_quotients(fv, fid, vecs, q, us)
    assert got == composed_quotients(fv, fid, vecs, q, us)
    if max(lens) <= 2049:
        assert got == hk.lincomb_quotients(p, polys, q, us)
    hv = as_vecs(polys, False)
    before = [v.copy() for v in hv]
    assert fused_quotients(fv, fid, hv, q, us[:2]) == got[:2]                  # host operands: staged, the same bytes, left untouched
    assert all((a == b).all() for a, b in zip(hv, before))
    assert fused_quotients(fv, fid, vecs, q, us[1:2], async_=True) == got[1:2]  # NMX_ASYNC, one point


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_quotients_on_proves_shape_in_every_field_and_both_forms(fv, fid):
    p = fc.FIELDS[fid]
    rng = random.Random(fid)
    ell = 11
    polys = rand_polys(p, [1 << (ell - i) for i in range(ell)], 30 + fid)
    r, q = rng.randrange(p), rng.randrange(p)
    us = [r, (-r) % p, r * r % p]
    vecs = as_vecs(polys, True)
    got = fused_quotients(fv, fid, vecs, q, us)
    assert got == hk.lincomb_quotients(p, polys, q, us) and got == composed_quotients(fv, fid, vecs, q, us)
    # out_j[0] = sum q^i f_i(u_j), from nmx_poly_eval_multi
    ev = fv.poly_eval_multi(fid, vecs, fc.vec(us))
    for j in range(3):
        assert got[j][0] == sum(pow(q, i, p) * int.from_bytes(ev[i][j], "little") for i in range(ell)) % p
    # Montgomery words: operands, q, the points and the outputs all x 2^256
    m = lambda x: x * R256 % p  # noqa: E731
    mv = as_vecs([[m(x) for x in f] for f in polys], True)
    gm = fused_quotients(fv, fid, mv, m(q), [m(u) for u in us], mont=True)
    assert gm == [[m(x) for x in o] for o in got] and gm == composed_quotients(fv, fid, mv, m(q), [m(u) for u in us], mont=True)


def test_quotients_at_value_edges(fv):
    fid = 1
    p = fc.FIELDS[fid]
    lens = (150, 75, 150, 9, 20, 33, 150)
    r = random.Random(2).randrange(p)
    mixed = rand_polys(p, lens, 77)
    mixed[2][5], mixed[0][149], mixed[6][0] = W256, p, p + 1
    for polys, q, us in (([[p - 1] * n for n in lens], p - 1, [p - 1] * 3), ([[0] * n for n in lens], r, [r, 0, 1]),
                         ([[W256] * n for n in lens], p - 1, [p - 1, r, 0]), (mixed, r, [0, 0, 0]), (mixed, 0, [r, (-r) % p, r * r % p]), (mixed, r, [r, r, r])):
        vecs = as_vecs(polys, True)
        got = fused_quotients(fv, fid, vecs, q, us)
        assert got == hk.lincomb_quotients(p, polys, q, us)
        assert got == composed_quotients(fv, fid, vecs, q, us)
    many = rand_polys(p, [40 + (i % 7) for i in range(40)], 5)               # k = 40: the descriptors travel through device memory
    vecs = as_vecs(many, True)
    assert fused_quotients(fv, fid, vecs, r, [r, 1]) == hk.lincomb_quotients(p, many, r, [r, 1])


def test_every_option_value_gives_the_same_bytes(L, fv):
    fid = 1
    p = fc.FIELDS[fid]
    polys = rand_polys(p, [4096 >> i for i in range(12)] + [4097], 12)
    q, us = 12345, [7, p - 7, 49]
    vecs = as_vecs(polys, True)
    want = hk.lincomb_quotients(p, polys, q, us)
    try:
        for chunk in (0, 4, 8):
            for scratch in (0, 1):
                assert L.nmx_set_option(b"kzg_quot_chunk", chunk) == 0 and L.nmx_set_option(b"kzg_quot_scratch", scratch) == 0
                assert fused_quotients(fv, fid, vecs, q, us) == want, (chunk, scratch)
        assert L.nmx_set_option(b"kzg_quot_chunk", 5) != 0
    finally:
        assert L.nmx_set_option(b"kzg_quot_chunk", 0) == 0 and L.nmx_set_option(b"kzg_quot_scratch", 1) == 0


def test_overlapping_hbm_buffers_and_bad_scalars_are_refused(L, fv):
    import ctypes
    from nova_amd import _lib
    p = fc.FIELDS[1]
    buf = gpu(fc.rand_vec(1, 64, 1))
    before = host(buf).copy()
    at = lambda i: buf.data_ptr() + 32 * i  # noqa: E731
    qv, pts, big = fc.vec([5]).copy(), fc.vec([7, 9]).copy(), fc.vec([p]).copy()

    def call(polys, lens, outs, q=qv, points=pts):
        pp, ll, oo = (ctypes.c_void_p * len(polys))(*polys), (ctypes.c_size_t * len(lens))(*lens), (ctypes.c_void_p * len(outs))(*outs)
        return L.nmx_poly_lincomb_quotients(1, pp, ll, len(polys), q.ctypes.data, points.ctypes.data, len(outs), _lib.SCALARS_DEVICE, oo)
    assert call((at(0), at(8)), (8, 4), (at(7), at(24))) == _lib.E_ARG and call((at(0), at(8)), (8, 4), (at(16), at(23))) == _lib.E_ARG
    assert call((at(0), at(8)), (8, 4), (at(16), at(24)), q=big) == _lib.E_SCALAR_RANGE
    assert call((at(0), at(8)), (8, 4), (at(16), at(24)), points=fc.vec([7, p]).copy()) == _lib.E_SCALAR_RANGE
    assert (host(buf) == before).all(), "a refused call wrote something"
    assert call((at(0), at(8)), (8, 4), (at(16), at(24))) == 0
    assert fc.ints(host(buf)[16:32]) == sum(hk.lincomb_quotients(p, [fc.ints(before[0:8]), fc.ints(before[8:12])], 5, [7, 9]), [])


# ---- nmx_hyperkzg_prove ------------------------------------------------------------------------------------------------------------
_keys = {}


def key_for(nova, cid, n, tables=True, tau=None):
    """a registered key of n points, made once per module: synthetic ((k0 + i) G), or tau^i G from a known tau"""
    k = (cid, n, tables, tau)
    if k not in _keys:
        if tau is None:
            _keys[k] = nova.CommitmentKey.generate(cid, n, k0=3, precompute=tables)
        else:
            _keys[k] = nova.CommitmentKey.setup_from_tau(cid, n, fc.vec([tau]), precompute=tables)
    return _keys[k]


def instance(cid, ell, seed):
    p = fc.FIELDS[FIELD_OF_CURVE[cid]]
    rng = random.Random(seed)
    return [rng.randrange(p) for _ in range(1 << ell)], [rng.randrange(p) for _ in range(ell)]


def one_call(nova, ck, hat_P_vec, point_vec, tr, mont=False):
    """-> (com, v, w) in the byte form of the composed sequence below"""
    com, v, w = nova.hyperkzg_prove(ck, hat_P_vec, point_vec, lambda s, d, c, i: tr.stage(s, d, c, i), mont=mont)
    return [(bytes(x), bool(i)) for x, i in com], [[bytes(e) for e in row] for row in v], [(bytes(x), bool(i)) for x, i in w]


def composed(nova, fv, cid, ck, hat_P_vec, point_vec, tr, mont=False):
    """the sequence every caller restated before the one call existed, with the two challenges squeezed in between"""
    fid = FIELD_OF_CURVE[cid]
    p = fc.FIELDS[fid]
    ce = nova.CommitmentEngine(cid)
    pt = np.asarray(point_vec).reshape(-1, 32)
    ell = len(pt)
    polys = [hat_P_vec]
    if ell > 1:
        polys += fv.fold_chain(fid, hat_P_vec, np.ascontiguousarray(pt[::-1][:ell - 1]), mont=mont)
    coms = ce.batch_commit(ck, polys[1:], mont=mont) if ell > 1 else []
    r = tr.decode(tr.stage(0, b"".join(c.xy for c in coms), len(coms), bytes(int(c.is_inf) for c in coms)))
    us = fc.vec([int.from_bytes(tr.encode(u), "little") for u in (r, (-r) % p, r * r % p)]).copy()
    v = fv.poly_eval_multi(fid, polys, us, mont=mont)
    q = tr.stage(1, b"".join(e for row in v for e in row), 3 * ell, None)
    B = fv.lincomb_powers(fid, polys, q, mont=mont)
    hs = [fv.suffix_horner(fid, B, us[j], mont=mont)[1:] for j in range(3)]
    w = ce.batch_commit(ck, hs, mont=mont)
    tr.stage(2, b"".join(c.xy for c in w), 3, bytes(int(c.is_inf) for c in w))
    return [(c.xy, c.is_inf) for c in coms], [[bytes(e) for e in row] for row in v], [(c.xy, c.is_inf) for c in w]


CASES = [(0, e) for e in (1, 2, 3, 4, 9, 10, 11, 14)] + [(c, e) for c in (1, 2, 3) for e in (3, 10)]


@pytest.mark.parametrize("cid,ell", CASES)
def test_prove_equals_the_composed_sequence(nmx, fv, cid, ell):
    p = fc.FIELDS[FIELD_OF_CURVE[cid]]
    hat_P, x = instance(cid, ell, 40 * cid + ell)
    ck = key_for(nmx, cid, 1 << (14 if cid == 0 else 10))
    Pv, xv = fc.vec(hat_P).copy(), fc.vec(x).copy()
    t0, t1, t2 = (hk.Sha3Transcript(p) for _ in range(3))
    want = composed(nmx, fv, cid, ck, gpu(Pv), xv, t0)
    dP = gpu(Pv)
    assert one_call(nmx, ck, dP, xv, t1) == want and (host(dP) == Pv).all(), "HBM operand: the same proof, hat_P never modified"
    assert t1.calls == t0.calls and [c[0] for c in t1.calls] == [0, 1, 2] and t1.calls[0][2] == ell - 1 and t1.calls[1][2] == 3 * ell
    before = Pv.copy()
    assert one_call(nmx, ck, Pv, xv, t2) == want and (Pv == before).all(), "host operand: the same proof, hat_P never modified"
    if ell in (3, 10):                                                          # Montgomery words, in HBM and on the host
        m = lambda vals: fc.vec([v * R256 % p for v in vals]).copy()  # noqa: E731
        tm0, tm1, tm2 = (hk.Sha3Transcript(p, mont=True) for _ in range(3))
        wm = composed(nmx, fv, cid, ck, gpu(m(hat_P)), m(x), tm0, mont=True)
        assert one_call(nmx, ck, gpu(m(hat_P)), m(x), tm1, mont=True) == wm and one_call(nmx, ck, m(hat_P), m(x), tm2, mont=True) == wm
        assert wm[0] == want[0], "the commitments of the folds come before any challenge: the same points in either form"


@pytest.mark.parametrize("ell", [4, 11])
def test_prove_on_a_key_without_window_tables(nmx, fv, ell):
    p = fc.FIELDS[1]
    hat_P, x = instance(0, ell, 7 + ell)
    Pv, xv = gpu(fc.vec(hat_P)), fc.vec(x).copy()
    with_t, without = key_for(nmx, 0, 1 << 14), key_for(nmx, 0, 1 << 11, tables=False)
    a = one_call(nmx, without, Pv, xv, hk.Sha3Transcript(p))
    assert a == composed(nmx, fv, 0, without, Pv, xv, hk.Sha3Transcript(p))
    assert a == one_call(nmx, with_t, Pv, xv, hk.Sha3Transcript(p)), "the two synthetic keys hold the same first points"


def to_points(pairs):
    return [None if inf else R.xy64_to_point(xy) for xy, inf in pairs]


@pytest.mark.parametrize("cid,ell", [(0, 1), (0, 2), (0, 5), (0, 8), (2, 3), (2, 8)])
def test_prove_equals_the_big_integer_restatement(nmx, cid, ell):
    c = R.CURVES_BY_ID[cid]
    p = c.r
    tau = random.Random(ell).randrange(2, p)
    hat_P, x = instance(cid, ell, 900 + ell)
    ck = key_for(nmx, cid, 256, tau=tau)
    com, v, w = one_call(nmx, ck, gpu(fc.vec(hat_P)), fc.vec(x).copy(), hk.Sha3Transcript(p))
    wc, wv, ww = hk.prove(c, tau, hat_P, x, hk.Sha3Transcript(p))
    assert (to_points(com), [[int.from_bytes(e, "little") for e in row] for row in v], to_points(w)) == (wc, wv, ww)


@pytest.mark.parametrize("cid", [0, 2])
@pytest.mark.parametrize("ell", [1, 6, 10])
def test_the_references_verifier_accepts(nmx, fv, cid, ell):
    c = R.CURVES_BY_ID[cid]
    p, fid = c.r, FIELD_OF_CURVE[cid]
    tau = random.Random(31 * ell + cid).randrange(2, p)
    ck = key_for(nmx, cid, 1024, tau=tau)
    grp, ce = nmx.DlogGroup(cid), nmx.CommitmentEngine(cid)
    hat_P, x = instance(cid, ell, 70 + ell)
    dP = gpu(fc.vec(hat_P))
    com, v, w = one_call(nmx, ck, dP, fc.vec(x).copy(), hk.Sha3Transcript(p))
    vi = [[int.from_bytes(e, "little") for e in row] for row in v]

    def msm(scalars, points):                                                   # the L of :1207-1225 through nmx_msm
        out = grp.vartime_multiscalar_mul(fc.vec(scalars).copy(), np.frombuffer(b"".join(R.point_to_xy64(P) for P in points), np.uint8).reshape(-1, 64).copy())
        return None if out.is_inf else R.xy64_to_point(out.xy)

    def accepted(poly_vec):
        cm = ce.commit(ck, poly_vec)
        y = int.from_bytes(fv.mle_evaluate(fid, poly_vec, fc.vec(x).copy()), "little")
        return hk.verify(c, tau, None if cm.is_inf else R.xy64_to_point(cm.xy), x, y, to_points(com), vi, to_points(w), hk.Sha3Transcript(p), msm=msm)
    assert accepted(dP) == (True, True)
    changed = fc.vec([(hat_P[0] + 1) % p] + hat_P[1:]).copy()                  # hat_P[0] changed after proving: another C and another y
    assert accepted(gpu(changed)) != (True, True)


class Forced:
    """a transcript that hands out fixed challenges (encoded values) at stages 0 / 1 and records what it is given"""

    def __init__(self, p, r=None, q=None, fail_at=None):
        self.inner, self.r, self.q, self.fail_at = hk.Sha3Transcript(p), r, q, fail_at
        self.encode, self.decode = self.inner.encode, self.inner.decode

    @property
    def calls(self):
        return self.inner.calls

    def stage(self, stage, data, count, is_inf):
        out = self.inner.stage(stage, data, count, is_inf)
        if self.fail_at == stage:
            raise RuntimeError("the transcript fails on purpose")
        forced = {0: self.r, 1: self.q}.get(stage)
        return out if forced is None else int(forced).to_bytes(32, "little")


def test_edges_zero_polynomial_zero_challenges_and_failing_callbacks(nmx, fv, L, capsys):
    from nova_amd import NmxError, _lib
    cid, ell = 0, 5
    p = fc.FIELDS[1]
    ck = key_for(nmx, cid, 1 << 14)
    hat_P, x = instance(cid, ell, 3)
    Pv, xv = gpu(fc.vec(hat_P)), fc.vec(x).copy()
    # hat_P all zero: every commitment is the identity, the flags are set, and the callback sees them
    tz = hk.Sha3Transcript(p)
    com, v, w = one_call(nmx, ck, gpu(np.zeros((1 << ell, 32), np.uint8)), xv, tz)
    assert com == [(bytes(64), True)] * (ell - 1) and w == [(bytes(64), True)] * 3 and v == [[bytes(32)] * 3] * ell
    assert tz.calls[0][3] == bytes([1] * (ell - 1)) and tz.calls[2][3] == bytes([1, 1, 1]) and tz.calls[1][3] is None
    # r = 0 (u = [0, 0, 0]) and q = 0: legal, nothing is inverted -- and equal to the composed sequence under the same transcript
    for r, q in ((0, None), (None, 0), (0, 0)):
        assert one_call(nmx, ck, Pv, xv, Forced(p, r, q)) == composed(nmx, fv, cid, ck, Pv, xv, Forced(p, r, q)), (r, q)
    # a challenge >= p: NMX_E_SCALAR_RANGE, and a later call on the same thread works
    want = one_call(nmx, ck, Pv, xv, hk.Sha3Transcript(p))
    for r, q in ((p, None), (None, W256)):
        with pytest.raises(NmxError) as e:
            one_call(nmx, ck, Pv, xv, Forced(p, r, q))
        assert e.value.code == _lib.E_SCALAR_RANGE
        assert one_call(nmx, ck, Pv, xv, hk.Sha3Transcript(p)) == want
    # a callback that returns non-zero (the Python wrapper turns an exception into 1), at every stage
    for stage in (0, 1, 2):
        with pytest.raises(NmxError) as e:
            one_call(nmx, ck, Pv, xv, Forced(p, fail_at=stage))
        assert e.value.code == _lib.E_ARG
    capsys.readouterr()                                                        # (the wrapper prints the traceback)
    assert one_call(nmx, ck, Pv, xv, hk.Sha3Transcript(p)) == want
    # n above the key's length, a coordinate of the point >= p
    short = key_for(nmx, cid, 1 << 11, tables=False)
    big, bx = instance(cid, 12, 4)
    with pytest.raises(NmxError) as e:
        one_call(nmx, short, gpu(fc.vec(big)), fc.vec(bx).copy(), hk.Sha3Transcript(p))
    assert e.value.code == _lib.E_HANDLE
    with pytest.raises(NmxError) as e:
        one_call(nmx, ck, Pv, fc.vec(x[:-1] + [p]).copy(), hk.Sha3Transcript(p))
    assert e.value.code == _lib.E_SCALAR_RANGE
    # every value of kzg_fused_quotients (0 the composed division, 1 the fused pass, 2 by size) gives the same proof, below and above the
    # size at which the default changes path
    for e2 in (1, 5, 11, 20):                                                  # 2^20: the size from which the default takes the fused pass
        big_ck = ck if e2 <= 14 else key_for(nmx, cid, 1 << e2, tables=False)
        dP, xv2 = gpu(fc.rand_vec(1, 1 << e2, 50 + e2)), fc.rand_vec(1, e2, 51 + e2).copy()
        proofs = []
        try:
            for val in (2, 0, 1):
                assert L.nmx_set_option(b"kzg_fused_quotients", val) == 0
                proofs.append(one_call(nmx, big_ck, dP, xv2, hk.Sha3Transcript(p)))
        finally:
            assert L.nmx_set_option(b"kzg_fused_quotients", 2) == 0
        assert proofs[0] == proofs[1] == proofs[2], e2
    assert L.nmx_set_option(b"kzg_fused_quotients", 3) != 0


def test_two_threads_prove_on_the_same_key_at_once(nmx):
    cid, ell = 0, 10
    p = fc.FIELDS[1]
    ck = key_for(nmx, cid, 1 << 14)
    insts = [instance(cid, ell, 60 + i) for i in range(2)]
    devs = [(gpu(fc.vec(P)), fc.vec(x).copy()) for P, x in insts]
    single = [one_call(nmx, ck, P, x, hk.Sha3Transcript(p)) for P, x in devs]
    got, errs = [None, None], []

    def work(i):
        try:
            for _ in range(3):
                got[i] = one_call(nmx, ck, devs[i][0], devs[i][1], hk.Sha3Transcript(p))
                assert got[i] == single[i]
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs and got == single
