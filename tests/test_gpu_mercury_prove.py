"""nmx_mercury_s_poly and nmx_mercury_prove on the GPU.
The correlation kernel byte for byte against its big-integer definition (tests/mercury_prove_common.s_definition, which
tests/test_mercury_prove_abi.py ties to the reference's FFT form); the one call against the yardstick's restatement of
EvaluationEngineTrait::prove (src/provider/mercury.rs:891-1268) under a key made from a known tau, against the composed sequence of public
calls under the same SHA3 transcript, and against the reference's verifier up to the pairing (:1270-1486; with tau known,
e(L, g2) == e(R, tau_H) is L == tau R).  The pairing itself, G2 and tau_H are outside this library and are not tested."""
import random
import threading

import numpy as np
import pytest

from oracle import pyref as R
from tests import fv_common as fc
from tests import mercury_prove_common as MP

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


def vec(vals):
    return fc.vec(vals).copy() if len(vals) else np.zeros((0, 32), np.uint8)


# ---- nmx_mercury_s_poly ---------------------------------------------------------------------------------------------------------------
def biased(p, n, rng, wide=True):
    """the 0 / 1 / p - 1 / p - 2 bias of tests/test_mercury_abi.py, and words at or above p"""
    edge = [0, 1, p - 1, p - 2] + ([p, p + 1, W256] if wide else [])
    return [rng.choice(edge) if rng.random() < 0.2 else rng.randrange(p) for _ in range(n)]


def s_call(fv, fid, ops, gamma, device, mont=False, async_=False):
    vs = [gpu(vec(v)) if device else vec(v) for v in ops]
    out = fv.mercury_s_poly(fid, vs[0], vs[1], vs[2], vs[3], fc.vec([gamma]), mont=mont, async_=async_)
    if async_:
        fv.sync()
    return fc.ints(host(out)) if len(ops[0]) > 1 else []


# the tile sizes (16, 32, 64) and one either side, the smallest shapes, several tiles and several chunks of index tiles
S_SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 512]


@pytest.mark.parametrize("b", S_SIZES)
def test_s_poly_equals_the_definition_in_every_field(fv, b):
    for fid, p in sorted(fc.FIELDS.items()):
        rng = random.Random(100 * b + fid)
        ops = [biased(p, b, rng) for _ in range(4)]
        for gamma in (0, 1, p - 1, rng.randrange(p)) if b <= 65 else (rng.randrange(p),):
            want = MP.s_definition(p, ops[0], ops[1], ops[2], ops[3], gamma)
            assert s_call(fv, fid, ops, gamma, True) == want, (fid, b, gamma)
        assert s_call(fv, fid, ops, gamma, False) == want, "host operands: staged, the same bytes"
        assert s_call(fv, fid, ops, gamma, True, async_=True) == want, "NMX_ASYNC"
        if b in (5, 65, 257):
            # Montgomery words (canonical values x 2^256): operands, gamma and the output all in that form
            vals = [biased(p, b, rng, wide=False) for _ in range(4)]
            m = lambda x: x * R256 % p  # noqa: E731
            got = s_call(fv, fid, [[m(x) for x in v] for v in vals], m(gamma), True, mont=True)
            assert got == [m(x) for x in MP.s_definition(p, vals[0], vals[1], vals[2], vals[3], gamma)]


def test_s_poly_at_the_shape_of_a_2p20_proof(fv):
    """b = 2^10 over BN254 Fr: the sum is spread widest here (32 x 32 tiles of 32, one chunk per tile)"""
    fid, b = 1, 1024
    p = fc.FIELDS[fid]
    rng = random.Random(1024)
    ops = [biased(p, b, rng) for _ in range(4)]
    gamma = rng.randrange(p)
    assert s_call(fv, fid, ops, gamma, True) == MP.s_definition(p, ops[0], ops[1], ops[2], ops[3], gamma)


def test_s_poly_every_option_value_gives_the_same_bytes_and_zero_upper_halves(L, fv):
    fid = 1
    p = fc.FIELDS[fid]
    rng = random.Random(77)
    try:
        for b in (5, 130, 512):
            ops = [biased(p, b, rng) for _ in range(4)]
            ops[2][b // 2:] = [0] * (b - b // 2)                                # the odd-ell shape: eq_row and h have a zero upper half
            ops[3][b // 2:] = [0] * (b - b // 2)
            gamma = rng.randrange(p)
            want = MP.s_definition(p, ops[0], ops[1], ops[2], ops[3], gamma)
            for tile in (0, 16, 32, 64):
                assert L.nmx_set_option(b"mercury_s_tile", tile) == 0
                assert s_call(fv, fid, ops, gamma, True) == want, (b, tile)
        assert L.nmx_set_option(b"mercury_s_tile", 48) != 0 and L.nmx_set_option(b"mercury_s_tile", 128) != 0
    finally:
        assert L.nmx_set_option(b"mercury_s_tile", 0) == 0
    zero = [[0] * 64 for _ in range(4)]
    assert s_call(fv, fid, zero, 5, True) == [0] * 63, "the zero polynomial: where the reference's drain(..b) panics, zeros here"


def test_s_poly_refuses_overlapping_hbm_buffers_and_bad_scalars(L):
    from nova_amd import _lib
    p = fc.FIELDS[1]
    buf = gpu(fc.rand_vec(1, 64, 1))
    before = host(buf).copy()
    at = lambda i: buf.data_ptr() + 32 * i  # noqa: E731
    g5, big = fc.vec([5]).copy(), fc.vec([p]).copy()

    def call(out, gamma=g5, b=8):
        return L.nmx_mercury_s_poly(1, at(0), at(8), at(16), at(24), b, gamma.ctypes.data, _lib.SCALARS_DEVICE, out)
    for out in (at(0), at(7), at(15), at(26), at(31)):
        assert call(out) == _lib.E_ARG, "out_s overlaps an input"
    assert call(at(32), gamma=big) == _lib.E_SCALAR_RANGE
    assert (host(buf) == before).all(), "a refused call wrote something"
    assert call(at(32)) == 0
    ops = [fc.ints(before[8 * i: 8 * i + 8]) for i in range(4)]
    after = host(buf)
    assert fc.ints(after[32:39]) == MP.s_definition(p, ops[0], ops[1], ops[2], ops[3], 5)
    assert (after[:32] == before[:32]).all() and (after[39:] == before[39:]).all(), "exactly b - 1 elements are written"


# ---- nmx_mercury_prove ------------------------------------------------------------------------------------------------------------
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


class Forced:
    """a transcript that hands out fixed challenges (plain integers, given encoded) at chosen stages, fails at one, and records everything"""

    def __init__(self, p, force=None, fail_at=None, raw=None, mont=False):
        self.inner, self.force, self.fail_at, self.raw = MP.Sha3Transcript(p, mont=mont), dict(force or {}), fail_at, dict(raw or {})
        self.encode, self.decode = self.inner.encode, self.inner.decode

    @property
    def calls(self):
        return self.inner.calls

    def stage(self, stage, data, count, is_inf):
        out = self.inner.stage(stage, data, count, is_inf)
        if self.fail_at == stage:
            raise RuntimeError("the transcript fails on purpose")
        if stage in self.raw:
            return int(self.raw[stage]).to_bytes(32, "little")
        return self.encode(self.force[stage]) if stage in self.force else out


def one_call(nova, ck, poly_vec, point_vec, tr, mont=False):
    comms, evals = nova.mercury_prove(ck, poly_vec, point_vec, lambda s, d, c, i: tr.stage(s, d, c, i), mont=mont)
    return [(bytes(x), bool(i)) for x, i in comms], [bytes(e) for e in evals]


def to_points(pairs):
    return [None if inf else R.xy64_to_point(xy) for xy, inf in pairs]


def restated(c, tau, poly, x, force=None, mont=False):
    comms, evals, trace = MP.prove(c, tau, poly, x, MP.Sha3Transcript(c.r, mont=mont), force=force)
    return comms, evals, trace


@pytest.mark.parametrize("cid,ell", [(0, 2), (0, 3), (0, 4), (0, 5), (0, 10), (0, 11), (1, 4), (2, 6), (2, 7), (3, 5)])
def test_prove_equals_the_big_integer_restatement(nmx, cid, ell):
    c = R.CURVES_BY_ID[cid]
    p = c.r
    tau = random.Random(ell).randrange(2, p)
    poly, x = instance(cid, ell, 900 + ell)
    ck = key_for(nmx, cid, 2048 if cid == 0 else 128, tau=tau)
    wc, we, _ = restated(c, tau, poly, x)
    tr = MP.Sha3Transcript(p)
    dP = gpu(fc.vec(poly))
    comms, evals = one_call(nmx, ck, dP, fc.vec(x).copy(), tr)
    assert (to_points(comms), [int.from_bytes(e, "little") for e in evals]) == (wc, we)
    assert [(s, n) for s, _d, n, _i in tr.calls] == [(0, 1), (1, 2), (2, 2), (3, 6), (4, 1), (5, 1), (6, 1)]
    assert tr.calls[3][3] is None and all(call[3] is not None for i, call in enumerate(tr.calls) if i != 3)
    assert (host(dP) == fc.vec(poly)).all(), "poly is never modified"
    if ell in (3, 4):
        # a host polynomial (left untouched), and Montgomery words in HBM and on the host: the restatement under a transcript that
        # absorbs and squeezes Montgomery words (the six evaluations reach it x 2^256, so its later challenges differ from the plain run's)
        hv = fc.vec(poly).copy()
        assert one_call(nmx, ck, hv, fc.vec(x).copy(), MP.Sha3Transcript(p)) == (comms, evals) and (hv == fc.vec(poly)).all()
        m = lambda vals: fc.vec([v * R256 % p for v in vals]).copy()  # noqa: E731
        mc, me, _ = restated(c, tau, poly, x, mont=True)
        assert mc[:5] == wc[:5], "the first five commitments come before the evaluations are absorbed: the same points in either form"
        for pv in (gpu(m(poly)), m(poly)):
            cm, em = one_call(nmx, ck, pv, m(x), MP.Sha3Transcript(p, mont=True), mont=True)
            assert to_points(cm) == mc and [int.from_bytes(e, "little") for e in em] == [v * R256 % p for v in me]


def composed(nova, fv, cid, ck, poly_vec, x, tr):
    """the sequence of public calls a caller had to restate: h, the division, s, the evaluations, quot_f, six commitment batches; the O(b)
    algebra of the batch opening from the yardstick in Python integers"""
    import torch
    fid = FIELD_OF_CURVE[cid]
    p = fc.FIELDS[fid]
    ce = nova.CommitmentEngine(cid)
    ell = len(x)
    pt = ([0] if ell % 2 else []) + list(x)
    log_b = len(pt) // 2
    b = 1 << log_b
    n_rows = (1 << ell) // b
    eq_row = fv.eq_evals_from_points(fid, fc.vec(pt[:log_b]).copy(), device=True)
    eq_col = fv.eq_evals_from_points(fid, fc.vec(pt[log_b:]).copy(), device=True)
    pair = lambda cs: (b"".join(c.xy for c in cs), len(cs), bytes(int(c.is_inf) for c in cs))  # noqa: E731
    h = torch.zeros((b, 32), dtype=torch.uint8, device="cuda")
    h[:n_rows] = fv.mercury_h_poly(fid, poly_vec, n_rows, b, eq_col)
    comm_h = ce.commit(ck, h[:n_rows].contiguous())
    alpha = tr.stage(0, *pair([comm_h]))
    q, g = fv.mercury_divide_by_binomial(fid, poly_vec, n_rows, b, alpha)
    comm_q, comm_g = ce.batch_commit(ck, [q, g])
    gamma = tr.stage(1, *pair([comm_q, comm_g]))
    s = fv.mercury_s_poly(fid, eq_col, g, eq_row, h, gamma)
    d = torch.flip(g, dims=[0]).contiguous()
    comm_s, comm_d = ce.batch_commit(ck, [s, d])
    zeta = tr.stage(2, *pair([comm_s, comm_d]))
    zi, al, ze = pow(tr.decode(zeta), -1, p), tr.decode(alpha), tr.decode(zeta)
    ev = fv.poly_eval_multi(fid, [g, h, s, d], fc.vec([ze, zi, al]).copy())
    E = lambda i, j: int.from_bytes(ev[i][j], "little")  # noqa: E731
    evd = {"g_zeta": E(0, 0), "g_zeta_inv": E(0, 1), "h_zeta": E(1, 0), "h_zeta_inv": E(1, 1), "h_alpha": E(1, 2), "s_zeta": E(2, 0), "s_zeta_inv": E(2, 1),
           "d_zeta": E(3, 0), "zeta": ze, "zeta_inv": zi, "alpha": al}
    evals = [ev[0][0], ev[0][1], ev[1][0], ev[1][1], ev[2][0], ev[2][1]]
    tr.stage(3, b"".join(evals), 6, None)
    quot, rem = fv.mercury_quot_f(fid, poly_vec, q, fc.vec([(pow(ze, b, p) - al) % p]).copy(), zeta)
    assert rem == ev[0][0], "quot_f's remainder is g(zeta)"
    comm_quot_f = ce.commit(ck, quot)
    beta = tr.decode(tr.stage(4, *pair([comm_quot_f])))
    ints = lambda t: fc.ints(host(t))  # noqa: E731
    done = {}

    def commit(coeffs):
        return ce.commit(ck, gpu(fc.vec(coeffs)))

    def squeeze_z(cw):
        done["w"] = cw
        return tr.decode(tr.stage(5, *pair([cw])))
    _cw, comm_wp, _W, _Wp = MP.generate_batch_evaluate_arg(p, commit, evd, (ints(g), ints(h), ints(s), ints(d)), beta, squeeze_z)
    tr.stage(6, *pair([comm_wp]))
    return [(c.xy, c.is_inf) for c in (comm_h, comm_g, comm_q, comm_s, comm_d, comm_quot_f, done["w"], comm_wp)], [bytes(e) for e in evals]


@pytest.mark.parametrize("ell", [14, 15])
def test_prove_equals_the_composed_sequence_of_public_calls(nmx, fv, ell):
    p = fc.FIELDS[1]
    ck = key_for(nmx, 0, 1 << 15)
    dP, xv = gpu(fc.rand_vec(1, 1 << ell, 40 + ell)), fc.rand_vec(1, ell, 41 + ell).copy()
    t0, t1 = MP.Sha3Transcript(p), MP.Sha3Transcript(p)
    want = composed(nmx, fv, 0, ck, dP, fc.ints(xv), t0)
    assert one_call(nmx, ck, dP, xv, t1) == want
    assert t1.calls == t0.calls


def accepted(nova, fv, c, tau, ck, poly_vec, x, comms, evals, force=None):
    fid = FIELD_OF_CURVE[c.cid]
    cm = nova.CommitmentEngine(c.cid).commit(ck, poly_vec)
    y = int.from_bytes(fv.mle_evaluate(fid, poly_vec, fc.vec(x).copy()), "little")
    return MP.verify(c, tau, None if cm.is_inf else R.xy64_to_point(cm.xy), x, y, to_points(comms), [int.from_bytes(e, "little") for e in evals],
                     MP.Sha3Transcript(c.r), force=force)


@pytest.mark.parametrize("cid", [0, 2])
@pytest.mark.parametrize("ell", [2, 3, 10, 11])
def test_the_references_verifier_accepts(nmx, fv, cid, ell):
    c = R.CURVES_BY_ID[cid]
    p = c.r
    tau = random.Random(31 * ell + cid).randrange(2, p)
    ck = key_for(nmx, cid, 2048, tau=tau)
    poly, x = instance(cid, ell, 70 + ell)
    dP = gpu(fc.vec(poly))
    comms, evals = one_call(nmx, ck, dP, fc.vec(x).copy(), MP.Sha3Transcript(p))
    assert accepted(nmx, fv, c, tau, ck, dP, x, comms, evals) == (True, True, True)
    changed = gpu(fc.vec([(poly[0] + 1) % p] + poly[1:]))                       # poly[0] changed after proving: another comm_f and another eval
    assert accepted(nmx, fv, c, tau, ck, changed, x, comms, evals) != (True, True, True)


@pytest.mark.parametrize("ell", [4, 11])
def test_prove_on_a_key_without_window_tables(nmx, ell):
    p = fc.FIELDS[1]
    poly, x = instance(0, ell, 7 + ell)
    Pv, xv = gpu(fc.vec(poly)), fc.vec(x).copy()
    with_t, without = key_for(nmx, 0, 1 << 15), key_for(nmx, 0, 1 << 11, tables=False)
    assert one_call(nmx, without, Pv, xv, MP.Sha3Transcript(p)) == one_call(nmx, with_t, Pv, xv, MP.Sha3Transcript(p)), \
        "the two synthetic keys hold the same first points"


def test_zero_polynomial_and_legal_edge_challenges(nmx, fv):
    c = R.BN254_G1
    p = c.r
    tau = random.Random(5).randrange(2, p)
    ck = key_for(nmx, 0, 2048, tau=tau)
    # the zero polynomial: eight identity points with their is_inf bytes, six zero evaluations
    tz = MP.Sha3Transcript(p)
    comms, evals = one_call(nmx, ck, gpu(np.zeros((32, 32), np.uint8)), fc.vec([3, 4, 5, 6, 7]).copy(), tz)
    assert comms == [(bytes(64), True)] * 8 and evals == [bytes(32)] * 6
    assert [call[3] for call in tz.calls] == [b"\x01", b"\x01\x01", b"\x01\x01", None, b"\x01", b"\x01", b"\x01"]
    # alpha = 0, gamma = 0, beta = 0 and z = alpha: legal, equal to the restatement under the same forced values, and accepted
    for ell in (4, 5):
        poly, x = instance(0, ell, 300 + ell)
        dP = gpu(fc.vec(poly))
        for force in ({0: 0}, {1: 0}, {4: 0}, {0: 12345, 5: 12345}, {0: 0, 1: 0, 4: 0, 5: 0}):
            wc, we, _ = restated(c, tau, poly, x, force=force)
            comms, evals = one_call(nmx, ck, dP, fc.vec(x).copy(), Forced(p, force))
            assert (to_points(comms), [int.from_bytes(e, "little") for e in evals]) == (wc, we), (ell, force)
            assert accepted(nmx, fv, c, tau, ck, dP, x, comms, evals, force=force) == (True, True, True), (ell, force)


def test_degenerate_challenges_failing_callbacks_and_bad_arguments(nmx, capsys):
    from nova_amd import NmxError, _lib
    cid, ell = 0, 5
    p = fc.FIELDS[1]
    ck = key_for(nmx, cid, 1 << 15)
    poly, x = instance(cid, ell, 3)
    Pv, xv = gpu(fc.vec(poly)), fc.vec(x).copy()
    want = one_call(nmx, ck, Pv, xv, MP.Sha3Transcript(p))

    def fails(tr, code, **kw):
        with pytest.raises(NmxError) as e:
            one_call(nmx, ck, Pv, xv, tr, **kw)
        assert e.value.code == code, (e.value.code, code)
        assert one_call(nmx, ck, Pv, xv, MP.Sha3Transcript(p)) == want, "a good call after the error"
    # the opening points coincide: zeta = 0 (no inverse), zeta^2 = 1, alpha = zeta, alpha = 1 / zeta
    for force in ({2: 0}, {2: 1}, {2: p - 1}, {0: 777, 2: 777}, {0: pow(777, -1, p), 2: 777}):
        fails(Forced(p, force), _lib.E_ZERO)
    # a challenge >= p at each stage that squeezes one
    for stage in (0, 1, 2, 4, 5):
        fails(Forced(p, raw={stage: p if stage % 2 else W256}), _lib.E_SCALAR_RANGE)
    # ... while what the callback writes at stages 3 and 6 is ignored
    assert one_call(nmx, ck, Pv, xv, Forced(p, raw={3: W256, 6: p})) == want
    # a callback that returns non-zero (the Python wrapper turns an exception into 1), at each of the seven stages
    for stage in range(7):
        fails(Forced(p, fail_at=stage), _lib.E_ARG)
    capsys.readouterr()                                                        # (the wrapper prints the tracebacks)
    # n above the key's length; a coordinate of the point >= p
    short = key_for(nmx, cid, 1 << 11, tables=False)
    big, bx = instance(cid, 12, 4)
    with pytest.raises(NmxError) as e:
        one_call(nmx, short, gpu(fc.vec(big)), fc.vec(bx).copy(), MP.Sha3Transcript(p))
    assert e.value.code == _lib.E_HANDLE
    with pytest.raises(NmxError) as e:
        one_call(nmx, ck, Pv, fc.vec(x[:-1] + [p]).copy(), MP.Sha3Transcript(p))
    assert e.value.code == _lib.E_SCALAR_RANGE
    assert one_call(nmx, ck, Pv, xv, MP.Sha3Transcript(p)) == want


def test_every_option_value_gives_the_same_proof(nmx, L):
    p = fc.FIELDS[1]
    ck = key_for(nmx, 0, 1 << 15)
    for ell in (5, 12):
        dP, xv = gpu(fc.rand_vec(1, 1 << ell, 50 + ell)), fc.rand_vec(1, ell, 51 + ell).copy()
        want = one_call(nmx, ck, dP, xv, MP.Sha3Transcript(p))
        try:
            for name, vals in ((b"kzg_fused_quotients", (0, 1)), (b"mercury_s_tile", (16, 64)), (b"mercury_seg_rows", (4,))):
                for val in vals:
                    assert L.nmx_set_option(name, val) == 0
                    assert one_call(nmx, ck, dP, xv, MP.Sha3Transcript(p)) == want, (ell, name, val)
        finally:
            assert L.nmx_set_option(b"kzg_fused_quotients", 2) == 0 and L.nmx_set_option(b"mercury_s_tile", 0) == 0
            assert L.nmx_set_option(b"mercury_seg_rows", 0) == 0


def test_two_threads_prove_on_the_same_key_at_once(nmx):
    cid, ell = 0, 10
    p = fc.FIELDS[1]
    ck = key_for(nmx, cid, 1 << 15)
    insts = [instance(cid, ell, 60 + i) for i in range(2)]
    devs = [(gpu(fc.vec(P)), fc.vec(x).copy()) for P, x in insts]
    single = [one_call(nmx, ck, P, x, MP.Sha3Transcript(p)) for P, x in devs]
    errs = []

    def work(i):
        try:
            for _ in range(3):
                assert one_call(nmx, ck, devs[i][0], devs[i][1], MP.Sha3Transcript(p)) == single[i]
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
