"""nmx_r1cs_is_sat on the GPU, through the C ABI: R1CSShape::is_sat / is_sat_relaxed (src/r1cs/mod.rs:474-574) and the three-check shape
of RecursiveSNARK::verify (src/nova/mod.rs:637-660).  Instances and their corruptions come from tests/r1cs_sat_common.py (checked on the
CPU against oracle.pyref by tests/test_r1cs_sat_abi.py); expected verdicts, counts and rows from the oracle residual, expected
commitments from oracle.cref.commit.  Every "bad" input is a wrong VALUE or a rejected ARGUMENT."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

from oracle import cref
from tests import fv_common as C
from tests import r1cs_sat_common as S
from tests import util

pytestmark = pytest.mark.gpu

NONE = 2 ** 64 - 1
EQ, CW, CE = 1, 2, 4
SHAPES = [(197, 150), (128, 128)]  # rows, cols: not multiples of 64, and one power-of-two shape


class Setup:
    """matrices and key of one instance, resident; expected commitments from the oracle"""

    def __init__(self, nmx, inst, seed=77, bases_mont=False, with_key=True):
        from nova_amd import fieldvec as fv
        self.inst = inst
        self.mats = [fv.SparseMatrix(inst.fid, ip, ix, dt, inst.cols) for ip, ix, dt in inst.csr]
        self.r_W, self.r_E = C.rand_vec(inst.fid, 1, seed), C.rand_vec(inst.fid, 1, seed + 1)
        self.ck = None
        self.bases_mont = bases_mont
        if with_key:
            self.bases, self.h = S.key_points(inst)
            self.cw, self.ce = S.expected_commitments(inst, self.bases, self.h, self.r_W, self.r_E)
            if bases_mont:
                self.ck = nmx.CommitmentKey.from_host(inst.cid, util.to_mont_bases(inst.cid, self.bases),
                                                      util.to_mont_bases(inst.cid, np.frombuffer(self.h, np.uint8)).tobytes(), mont=True)
            else:
                self.ck = nmx.CommitmentKey.from_host(inst.cid, self.bases, self.h)

    def close(self):
        for m in self.mats:
            m.close()
        if self.ck is not None:
            self.ck.close()


def point_arg(cid, pt, bases_mont):
    """(xy64, is_inf) from the oracle -> (array in the ABI form, is_inf)"""
    if pt is None:
        return None, 0
    xy, inf = pt
    a = np.frombuffer(xy, np.uint8).copy()
    if bases_mont and not inf:
        a = util.to_mont_bases(cid, a).reshape(-1)
    return a, int(inf)


def call(L, su, inst=None, *, dev=False, mont=False, ck=True, cw="own", ce="own", r_W=None, r_E=None, mats=None, n_w=None, n_e=None, n_io=None,
         flags=None, E="own", u="own", ckh=None, comm_mont=None):
    """one nmx_r1cs_is_sat call -> (rc, verdict, bad_rows, first_bad_row).  `inst` holds CANONICAL values; mont converts the scalars."""
    import torch
    from nova_amd import _lib
    inst = su.inst if inst is None else inst
    src = S.to_mont(inst) if mont else inst
    keep = []

    def vec_arg(v):
        if v is None:
            return None
        a = np.ascontiguousarray(v)
        if dev:
            t = torch.from_numpy(a.copy()).cuda()
            torch.cuda.synchronize()
            keep.append(t)
            return t.data_ptr()
        keep.append(a)
        return a.ctypes.data

    conv = (lambda r: util.to_mont_scalars(inst.cid, r)) if mont else (lambda r: np.ascontiguousarray(r))
    rw = conv(su.r_W if r_W is None else r_W)
    re_ = conv(su.r_E if r_E is None else r_E)
    Ev = src.E if isinstance(E, str) else E
    uv = src.u if isinstance(u, str) else u
    bm = su.bases_mont if comm_mont is None else comm_mont
    cwa, cwi = point_arg(inst.cid, su.cw if isinstance(cw, str) else cw, bm) if su.ck is not None or not isinstance(cw, str) else (None, 0)
    cea, cei = point_arg(inst.cid, su.ce if isinstance(ce, str) else ce, bm) if su.ck is not None or not isinstance(ce, str) else (None, 0)
    hh = None
    if su.ck is not None:
        hh = np.frombuffer(su.ck.h, np.uint8).copy()
    if flags is None:
        flags = (_lib.SCALARS_DEVICE if dev else 0) | (_lib.SCALARS_MONT if mont else 0) | (_lib.BASES_MONT if su.bases_mont else 0)
    handle = ckh if ckh is not None else (su.ck.handle if (ck and su.ck is not None) else 0)
    hs = [m.handle for m in su.mats] if mats is None else mats
    X = np.ascontiguousarray(src.X)
    uu = None if uv is None else np.ascontiguousarray(uv)
    ptr = lambda a: None if a is None else a.ctypes.data
    verdict, bad, first = ctypes.c_uint32(0xdead), ctypes.c_uint64(0xdead), ctypes.c_uint64(0xdead)
    rc = L.nmx_r1cs_is_sat(hs[0], hs[1], hs[2], handle, vec_arg(src.W), inst.n_w if n_w is None else n_w, vec_arg(Ev),
                           (inst.rows if Ev is not None else 0) if n_e is None else n_e, ptr(uu), ptr(X) if X.size else None,
                           inst.n_io if n_io is None else n_io, ptr(rw), ptr(re_), ptr(hh), ptr(cwa), cwi, ptr(cea), cei, flags,
                           ctypes.byref(verdict), ctypes.byref(bad), ctypes.byref(first))
    return rc, verdict.value, bad.value, first.value


@pytest.fixture(scope="module")
def L(nmx):
    from nova_amd import _lib
    return _lib.lib()


# ---- 1. satisfied instances -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", sorted(C.FIELDS))
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_satisfied_instances(nmx, L, fid, rows, cols):
    import torch
    from nova_amd import fieldvec as fv
    for inst in (S.make_relaxed(fid, rows, cols, seed=100 + fid), S.make_strict(fid, rows, cols, seed=200 + fid)):
        su = Setup(nmx, inst)
        try:
            for mont in (False, True):
                for dev in (False, True):
                    got = call(L, su, dev=dev, mont=mont)
                    print(fid, rows, cols, "relaxed" if inst.relaxed else "strict", "mont" if mont else "canon", "hbm" if dev else "host", got)
                    assert got == (0, 0, 0, NONE), L.nmx_last_error()
            # the composed path agrees: nmx_r1cs_cross_term's residual is all zero
            z = torch.from_numpy(inst.z().copy()).cuda()
            e = torch.from_numpy(inst.E.copy() if inst.relaxed else np.zeros((rows, 32), np.uint8)).cuda()
            torch.cuda.synchronize()
            T = fv.r1cs_cross_term(su.mats[0], su.mats[1], su.mats[2], z, None, e, inst.u if inst.relaxed else C.vec([1]))
            assert not T.cpu().numpy().any()
        finally:
            su.close()


# ---- 2. exactly one corrupted row ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", sorted(C.FIELDS))
@pytest.mark.parametrize("dev,mont", [(False, False), (True, True)])
def test_one_corrupted_row(nmx, L, fid, dev, mont):
    rows, cols = SHAPES[0]
    inst = S.make_relaxed(fid, rows, cols, seed=300 + fid)
    su = Setup(nmx, inst)
    try:
        for j in (0, 63, 64, rows // 2, rows - 1):
            for corrupt in (S.corrupt_E_plus_one, S.corrupt_E_minus_one):
                bad = corrupt(inst, j)
                assert bad.bad_rows() == (1, j)
                # the prover committed to the E it sent: only the equation fails
                _cw, ce = S.expected_commitments(bad, su.bases, su.h, su.r_W, su.r_E)
                got = call(L, su, bad, dev=dev, mont=mont, ce=ce)
                print(fid, corrupt.__name__, j, got)
                assert got == (0, EQ, 1, j)
        # one witness element changed: the rows the oracle residual names, and comm_W no longer matches
        k = S.column_of_row(inst, rows // 2)
        bad = S.corrupt_W(inst, k)
        n_bad, first = bad.bad_rows()
        assert n_bad >= 1
        got = call(L, su, bad, dev=dev, mont=mont)
        print(fid, "W", k, got, (n_bad, first))
        assert got == (0, EQ | CW, n_bad, first)
        # a wrong u
        bad = S.corrupt_u(inst)
        n_bad, first = bad.bad_rows()
        assert n_bad >= 1
        got = call(L, su, bad, dev=dev, mont=mont)
        print(fid, "u", got, (n_bad, first))
        assert got == (0, EQ, n_bad, first)
    finally:
        su.close()
    # strict form: one witness element
    st = S.make_strict(fid, rows, cols, seed=310 + fid)
    su = Setup(nmx, st)
    try:
        bad = S.corrupt_W(st, S.column_of_row(st, rows // 2))
        n_bad, first = bad.bad_rows()
        assert n_bad >= 1
        assert call(L, su, bad, dev=dev, mont=mont) == (0, EQ | CW, n_bad, first)
    finally:
        su.close()


# ---- 3. many violations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", sorted(C.FIELDS))
def test_many_violations_are_counted_exactly(nmx, L, fid):
    rows, cols = 1000, 777
    inst = S.make_relaxed(fid, rows, cols, seed=400 + fid)
    su = Setup(nmx, inst, with_key=False)
    try:
        for step, start in ((7, 3), (1, 0)):
            bad = inst.copy()
            for j in range(start, rows, step):
                S.bump(bad.E, j, 1 + j, inst.p)
            want = bad.bad_rows()
            assert want == (len(range(start, rows, step)), start)
            for dev, mont in ((True, False), (False, True)):
                got = call(L, su, bad, dev=dev, mont=mont)
                print(fid, step, got, want)
                assert got == (0, EQ) + want
    finally:
        su.close()


# ---- 4. the commitment half -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", [1, 3])
def test_commitment_half(nmx, L, fid):
    rows, cols = SHAPES[0]
    inst = S.make_relaxed(fid, rows, cols, seed=500 + fid)
    su = Setup(nmx, inst)
    sm = Setup(nmx, inst, bases_mont=True)  # the same key, h and expected commitments as Montgomery limbs (NMX_BASES_MONT)
    other_r = C.rand_vec(fid, 1, 999)
    bad_eq = S.corrupt_u(inst)
    n_bad, first = bad_eq.bad_rows()
    try:
        for s in (su, sm):
            for dev in (False, True):
                assert call(L, s, dev=dev) == (0, 0, 0, NONE)
                assert call(L, s, dev=dev, cw=s.ce) == (0, CW, 0, NONE)              # wrong comm_W (a valid point, not this one)
                assert call(L, s, dev=dev, ce=s.cw) == (0, CE, 0, NONE)              # wrong comm_E
                assert call(L, s, dev=dev, r_W=other_r) == (0, CW, 0, NONE)          # wrong r_W
                assert call(L, s, dev=dev, r_E=other_r) == (0, CE, 0, NONE)
                assert call(L, s, dev=dev, cw=s.ce, ce=s.cw) == (0, CW | CE, 0, NONE)
                assert call(L, s, dev=dev, cw=(bytes(64), 1)) == (0, CW, 0, NONE)    # identity expected, a point committed
                assert call(L, s, bad_eq, dev=dev, cw=s.ce, ce=s.cw) == (0, EQ | CW | CE, n_bad, first)  # both halves wrong at once
                assert call(L, s, bad_eq, dev=dev) == (0, EQ, n_bad, first)
            # Montgomery scalars, same verdicts
            assert call(L, s, mont=True, dev=True) == (0, 0, 0, NONE)
            assert call(L, s, mont=True, dev=True, cw=s.ce) == (0, CW, 0, NONE)
        # the forgotten flag: Montgomery key, canonical expected commitments -> they match nothing
        assert call(L, sm, comm_mont=False) == (0, CW | CE, 0, NONE)
        # and a Montgomery h / commitments handed over WITHOUT the flag to a canonical key
        from nova_amd import _lib
        rc, v, _b, _f = call(L, su, comm_mont=True, flags=0)
        assert rc == 0 and v == (CW | CE)
    finally:
        su.close()
        sm.close()
    # E = 0 and r_E = 0: comm_E is the identity and must pass; a flag that disagrees must fail
    st = S.make_strict(fid, rows, cols, seed=510 + fid)
    rel = S.Instance(fid, rows, cols, st.n_io, st.csr, st.W, st.X, u=C.vec([1]).copy(), E=np.zeros((rows, 32), np.uint8))
    assert rel.bad_rows() == (0, NONE)
    su = Setup(nmx, rel)
    try:
        zero = np.zeros((1, 32), np.uint8)
        assert cref.commit(rel.cid, rel.E, su.bases[:rows], rows, su.h, zero) == (bytes(64), 1)
        for dev in (False, True):
            assert call(L, su, dev=dev, r_E=zero, ce=(bytes(64), 1)) == (0, 0, 0, NONE)
            assert call(L, su, dev=dev, r_E=zero, ce=(bytes(64), 0)) == (0, CE, 0, NONE)   # identity flag mismatch
            assert call(L, su, dev=dev, r_E=zero, ce=su.cw) == (0, CE, 0, NONE)
            assert call(L, su, dev=dev, cw=(su.cw[0], 1)) == (0, CW, 0, NONE)              # flagged identity, a point committed
    finally:
        su.close()


# ---- 5. argument errors ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing_and_leave_no_ticket(nmx, L):
    from nova_amd import _lib
    rows, cols = SHAPES[0]
    inst = S.make_relaxed(1, rows, cols, seed=600)
    su = Setup(nmx, inst)
    other = Setup(nmx, S.make_relaxed(1, rows + 1, cols, seed=601), with_key=False)    # another shape
    other_f = Setup(nmx, S.make_relaxed(0, rows, cols, seed=602), with_key=False)      # another field
    hs = [m.handle for m in su.mats]

    def expect(code, word, **kw):
        rc, v, b, f = call(L, su, **kw)
        msg = L.nmx_last_error().decode()
        assert rc == code, (rc, msg, kw)
        assert (v, b, f) == (0xdead, 0xdead, 0xdead)  # nothing is written on an error
        assert word in msg, msg

    try:
        for dev in (False, True):
            expect(_lib.E_ARG, "W.len()", dev=dev, n_w=inst.n_w - 1)
            expect(_lib.E_ARG, "W.len()", dev=dev, n_w=inst.n_w + 1)
            expect(_lib.E_ARG, "X.len()", dev=dev, n_io=inst.n_io + 1)
            expect(_lib.E_ARG, "X.len()", dev=dev, n_io=inst.n_io - 1)
            expect(_lib.E_ARG, "E.len()", dev=dev, n_e=rows - 1)
            expect(_lib.E_ARG, "E.len()", dev=dev, n_e=rows + 1)
            expect(_lib.E_ARG, "E and u", dev=dev, u=None)
            expect(_lib.E_ARG, "E and u", dev=dev, E=None)
            expect(_lib.E_ARG, "share field and shape", dev=dev, mats=[hs[0], hs[1], other.mats[2].handle])
            expect(_lib.E_ARG, "share field and shape", dev=dev, mats=[hs[0], other_f.mats[1].handle, hs[2]])
            expect(_lib.E_HANDLE, "matrix handle", dev=dev, mats=[hs[0], hs[1], 0xdeadbeef])
            expect(_lib.E_HANDLE, "base handle", dev=dev, ckh=0xdeadbeef)
            expect(_lib.E_ARG, "unsupported flag", dev=dev, flags=_lib.ASYNC | (_lib.SCALARS_DEVICE if dev else 0))
        # the matrices' field must be the scalar field of the key's curve; a key shorter than W / E is NMX_E_HANDLE as for nmx_commit
        gr = nmx.CommitmentKey.generate(1, 256, k0=3)      # Grumpkin: scalars in BN254 Fq, the matrices are over BN254 Fr
        short = nmx.CommitmentKey.generate(0, 16, k0=3)
        try:
            expect(_lib.E_ARG, "scalar field", ckh=gr.handle)
            expect(_lib.E_HANDLE, "ck shorter", ckh=short.handle)
        finally:
            gr.close()
            short.close()
        # no ticket, no context left behind: a commitment and a full check on the same thread still work
        com = nmx.CommitmentEngine(inst.cid).commit(su.ck, inst.W, su.r_W)
        assert (com.xy, int(com.is_inf)) == su.cw
        assert call(L, su, dev=True) == (0, 0, 0, NONE)
        assert L.nmx_commit_finish(1 << 40, np.zeros(64, np.uint8).ctypes.data, None) == _lib.E_HANDLE
    finally:
        su.close()
        other.close()
        other_f.close()


# ---- 6. the equation-only form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", [0, 2])
def test_equation_only_form_equals_the_equation_half(nmx, L, fid):
    rows, cols = SHAPES[0]
    inst = S.make_relaxed(fid, rows, cols, seed=700 + fid)
    su = Setup(nmx, inst)
    try:
        cases = [inst, S.corrupt_E_plus_one(inst, 64), S.corrupt_u(inst), S.corrupt_W(inst, S.column_of_row(inst, rows // 2))]
        for case in cases:
            for dev in (False, True):
                full = call(L, su, case, dev=dev)
                eq_only = call(L, su, case, dev=dev, ck=False)
                assert full[0] == eq_only[0] == 0
                assert eq_only[1] == (full[1] & EQ) and eq_only[2:] == full[2:] == case.bad_rows()
        st = S.make_strict(fid, rows, cols, seed=710 + fid)
        s2 = Setup(nmx, st, with_key=False)
        try:
            assert call(L, s2, dev=True) == (0, 0, 0, NONE)
            bad = S.corrupt_W(st, S.column_of_row(st, rows // 2))
            assert call(L, s2, bad, dev=True) == (0, EQ) + bad.bad_rows()
        finally:
            s2.close()
    finally:
        su.close()


# ---- 7. the shape of RecursiveSNARK::verify ------------------------------------------------------------------------------------------------------
def _verify_setups(nmx):
    """primary relaxed (BN254 scalars, rows = cols = 2^16), secondary relaxed and secondary strict (Grumpkin scalars, 10 538)"""
    prim = Setup(nmx, S.make_relaxed(1, 1 << 16, 1 << 16, seed=800), seed=81)
    sec_r = Setup(nmx, S.make_relaxed(0, 10538, 10538, seed=801), seed=83)
    sec_s = Setup(nmx, S.make_strict(0, 10538, 10538, seed=802), seed=85)
    return [prim, sec_r, sec_s]


def _three_at_once(L, setups, insts, dev):
    out = [None] * 3
    errs = []

    def work(i):
        try:
            out[i] = call(L, setups[i], insts[i], dev=dev)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(3)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    return out


def test_recursive_snark_verify_shape_from_three_threads(nmx, L):
    setups = _verify_setups(nmx)
    try:
        good = [s.inst for s in setups]
        serial = [call(L, s, dev=True) for s in setups]
        assert serial == [(0, 0, 0, NONE)] * 3, serial
        for rep in range(10):
            assert _three_at_once(L, setups, good, dev=(rep % 2 == 0)) == serial
        # one of the three violated
        bad_sec = S.corrupt_E_minus_one(setups[1].inst, 5000)
        _cw, ce = S.expected_commitments(bad_sec, setups[1].bases, setups[1].h, setups[1].r_W, setups[1].r_E)
        setups[1].ce = ce
        mixed = [good[0], bad_sec, good[2]]
        serial_bad = [call(L, s, i, dev=True) for s, i in zip(setups, mixed)]
        assert serial_bad == [(0, 0, 0, NONE), (0, EQ, 1, 5000), (0, 0, 0, NONE)]
        for rep in range(10):
            assert _three_at_once(L, setups, mixed, dev=(rep % 2 == 0)) == serial_bad
    finally:
        for s in setups:
            s.close()


def test_recursive_snark_verify_shape_over_a_sharded_key(nmx, L):
    assert nmx.init_devices(2, oversubscribe=True) == 2
    assert L.nmx_set_option(b"shard_min_n", 1000) == 0
    try:
        setups = _verify_setups(nmx)  # keys registered now are cut over the two logical devices
        try:
            assert len(setups[0].ck.shard_plan()) == 2
            good = [s.inst for s in setups]
            for dev in (True, False):
                assert _three_at_once(L, setups, good, dev=dev) == [(0, 0, 0, NONE)] * 3
            bad = S.corrupt_W(good[0], S.column_of_row(good[0], 1 << 15))
            want = bad.bad_rows()
            assert _three_at_once(L, setups, [bad, good[1], good[2]], dev=True) == [(0, EQ | CW) + want, (0, 0, 0, NONE), (0, 0, 0, NONE)]
        finally:
            for s in setups:
                s.close()
    finally:
        assert L.nmx_set_option(b"shard_min_n", 1 << 20) == 0
        assert nmx.init_devices(1) == 1


# ---- 8. ordered behind NMX_ASYNC ---------------------------------------------------------------------------------------------------------------
def test_is_ordered_behind_the_async_fold(nmx, L):
    import torch
    from nova_amd import fieldvec as fv
    fid, rows, cols = 1, 60000, 60000
    inst = S.make_relaxed(fid, rows, cols, seed=900)
    su = Setup(nmx, inst)
    p = inst.p
    try:
        # W = W1 + r W2 and E = E1 + r T: the fold's outputs are the satisfying pair, anything else in those buffers is not
        r = C.rand_vec(fid, 1, 901)
        ri = C.ints(r)[0]
        W2, T = C.rand_vec(fid, inst.n_w, 902), C.rand_vec(fid, rows, 903)
        W1 = C.vec([(w - ri * w2) % p for w, w2 in zip(C.ints(inst.W), C.ints(W2))])
        E1 = C.vec([(e - ri * t) % p for e, t in zip(C.ints(inst.E), C.ints(T))])
        dW1, dW2, dE1, dT = (torch.from_numpy(np.ascontiguousarray(v).copy()).cuda() for v in (W1, W2, E1, T))
        torch.cuda.synchronize()
        Ws, Es = fv.nifs_fold(fid, dW1, dW2, dE1, dT, r)  # the synchronous sequence
        assert np.array_equal(Ws.cpu().numpy(), inst.W) and np.array_equal(Es.cpu().numpy(), inst.E)
        cw = nmx.Commitment(*[su.cw[0], bool(su.cw[1])])
        ce = nmx.Commitment(*[su.ce[0], bool(su.ce[1])])
        want = fv.r1cs_is_sat_relaxed(su.mats[0], su.mats[1], su.mats[2], su.ck, Ws, Es, inst.u, inst.X, cw, ce, su.r_W, su.r_E)
        assert want.ok and want.bad_rows == 0 and want.first_bad_row is None
        for _ in range(3):
            Wa, Ea = fv.nifs_fold(fid, dW1, dW2, dE1, dT, r, async_=True)
            got = fv.r1cs_is_sat_relaxed(su.mats[0], su.mats[1], su.mats[2], su.ck, Wa, Ea, inst.u, inst.X, cw, ce, su.r_W, su.r_E)  # no sync in between
            assert (got.verdict, got.bad_rows, got.first_bad_row) == (want.verdict, want.bad_rows, want.first_bad_row), repr(got)
            assert torch.equal(Wa, Ws) and torch.equal(Ea, Es)
        # the Python wrappers: strict form, the equation only, a violated instance
        bad = S.corrupt_E_plus_one(inst, 12345)
        got = fv.r1cs_is_sat_relaxed(su.mats[0], su.mats[1], su.mats[2], None, inst.W, bad.E, inst.u, inst.X, None, None)
        assert (got.ok, got.eq_ok, got.comm_W_ok, got.comm_E_ok, got.bad_rows, got.first_bad_row) == (False, False, True, True, 1, 12345)
    finally:
        su.close()
    st = S.make_strict(fid, 300, 280, seed=910)
    s2 = Setup(nmx, st)
    try:
        cw = nmx.Commitment(s2.cw[0], bool(s2.cw[1]))
        assert fv.r1cs_is_sat(s2.mats[0], s2.mats[1], s2.mats[2], s2.ck, st.W, st.X, cw, s2.r_W).ok
        assert fv.r1cs_is_sat(s2.mats[0], s2.mats[1], s2.mats[2], s2.ck, torch.from_numpy(st.W.copy()).cuda(), st.X, s2.cw, s2.r_W).ok
        res = fv.r1cs_is_sat(s2.mats[0], s2.mats[1], s2.mats[2], s2.ck, st.W, st.X, cw)  # r_W left out (zero): the commitment differs
        assert res.eq_ok and not res.comm_W_ok and not res.ok
    finally:
        s2.close()


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_on_gpu(nmx):
    from tests import test_r1cs_sat_abi as A
    b = A.BIN if os.path.exists(A.BIN) else A.build_cpp()
    r = subprocess.run([b], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "r1cs_sat mirror ok" in r.stdout
