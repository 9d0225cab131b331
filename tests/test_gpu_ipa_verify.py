"""-m gpu: nmx_ipa_verify (InnerProductArgument::verify, /root/reference/src/provider/ipa_pc.rs:286-390) through the C ABI.  Every
expectation -- the verdict, ck_hat, b_hat -- comes from the Python-integer restatement (tests/ipa_verify_common.py, itself checked on
the CPU in tests/test_ipa_verify_abi.py) or the oracle, never from the code under test."""
import os
import subprocess
import threading

import numpy as np
import pytest

from oracle import cref
from oracle import pyref as R
from tests import ipa_common as ic
from tests import ipa_verify_common as V
from tests import util

pytestmark = pytest.mark.gpu
CURVES = [R.BN254_G1, R.GRUMPKIN, R.PALLAS, R.VESTA]


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def les(xs):
    return [ic.le(x) for x in xs]


def key_of(nmx, I, ck=None, **kw):
    return nmx.CommitmentKey.from_host(I["curve"].cid, I["ck"] if ck is None else ck, **kw)


def run(nmx, K, I, b=None, point=None, **over):
    """-> (accepted, ck_hat as (xy, is_inf), b_hat as an integer) for the instance with `over` applied (canonical forms)"""
    J = dict(I, **over)
    ca = (ic.pt_bytes(J["comm_a"]), J["comm_a"] is R.INF)
    if point is not None:
        ok, ckh, bh = nmx.ipa_verify(K, J["ckc"], ca, ic.le(J["c"]), np.frombuffer(b"".join(les(point)), np.uint8).copy(), J["Ls"], J["Rs"],
                                     J["infs"], J["a_hat"], les(J["rs"]), point=True, want_intermediates=True)
    else:
        bb = V.b_array(J["bi"]) if b is None else b
        ok, ckh, bh = nmx.ipa_verify(K, J["ckc"], ca, ic.le(J["c"]), bb, J["Ls"], J["Rs"], J["infs"], J["a_hat"], les(J["rs"]),
                                     want_intermediates=True)
    return ok, (ckh.xy, ckh.is_inf), int.from_bytes(bh, "little")


def expect(I, **over):
    res = V.restate_instance(I, **over)
    return res.verdict, (ic.pt_bytes(res.ck_hat), res.ck_hat is R.INF), res.b_hat


# ---- 1. honest proofs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("n", [1, 2, 4, 256, 1 << 10, 1 << 14])
def test_accepts_proofs_of_the_oracle_and_of_the_library(nmx, curve, n):
    I = V.instance_of(curve, n, seed=60 + (n % 251))
    want = expect(I)
    assert want[0] is True
    K = key_of(nmx, I)
    try:
        assert run(nmx, K, I, b=dev(I["b"])) == want            # the oracle's proof, b in HBM
        assert run(nmx, K, I) == want                           # host b
        tr = ic.IpaTranscript(curve.r)
        Ls, Rs, infs, a_hat = nmx.ipa_prove(K, I["ckc"], dev(I["a"]), dev(I["b"]), tr)   # the library's own proof
        mine = dict(Ls=Ls, Rs=Rs, infs=infs, a_hat=a_hat, rs=list(tr.rs))
        assert (Ls, Rs, a_hat) == (I["Ls"], I["Rs"], I["a_hat"])
        assert run(nmx, K, I, **mine) == want
    finally:
        K.close()


def test_large_2p17(nmx):
    """one size well past a single group of tiles per block; the proof is the library's (the oracle's key-folding prover is slow
    here), the expectations are the restatement's"""
    curve, n = R.GRUMPKIN, 1 << 17
    ck, ckc, a, b = ic.make_instance(curve, n, 7)
    K = nmx.CommitmentKey.from_host(curve.cid, ck)
    try:
        tr = ic.IpaTranscript(curve.r)
        Ls, Rs, infs, a_hat = nmx.ipa_prove(K, ckc, dev(a), dev(b), tr)
        ai, bi = ic.ints(a), ic.ints(b)
        comm_a = ic.pt(*cref.msm(curve.cid, a, ck, n))
        I = dict(curve=curve, n=n, ck=ck, ckc=ckc.tobytes(), a=a, b=b, bi=bi, comm_a=comm_a, c=sum(x * y for x, y in zip(ai, bi)) % curve.r,
                 Ls=Ls, Rs=Rs, infs=infs, a_hat=a_hat, rs=list(tr.rs))
        want = expect(I)
        assert want[0] is True
        assert run(nmx, K, I, b=dev(b)) == want
        bad = list(bi)
        bad[n - 1] = (bad[n - 1] + 1) % curve.r
        assert run(nmx, K, I, bi=bad) == expect(I, bi=bad) and expect(I, bi=bad)[0] is False
    finally:
        K.close()


# ---- 2. every single tamper is refused ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,n", [(R.GRUMPKIN, 256), (R.PALLAS, 8), (R.BN254_G1, 2), (R.VESTA, 1 << 10)], ids=lambda x: getattr(x, "name", str(x)))
def test_rejects_each_single_tamper(nmx, curve, n):
    I = V.instance_of(curve, n, seed=80 + (n % 251))
    K = key_of(nmx, I)
    try:
        for name, over in V.tampers(I).items():
            want = expect(I, **over)
            assert want[0] is False, name
            assert run(nmx, K, I, **over) == want, name
        # a proof for this key verified over a different key
        other = cref.sequential_bases(curve, 5000, n).copy()
        K2 = key_of(nmx, I, ck=other)
        try:
            want = expect(I, ck=other)
            assert want[0] is False and run(nmx, K2, I) == want
        finally:
            K2.close()
    finally:
        K.close()


def test_accepts_an_all_zero_witness(nmx):
    """a = 0: every L and R is the identity (is_inf), comm_a is the identity (null pointer allowed), a_hat = 0"""
    I = V.instance_of(R.GRUMPKIN, 64, seed=3, zero_a=True)
    assert I["comm_a"] is R.INF and all(i == (True, True) for i in I["infs"])
    K = key_of(nmx, I)
    try:
        want = expect(I)
        assert want[0] is True and run(nmx, K, I) == want
    finally:
        K.close()


# ---- 3. forms ----------------------------------------------------------------------------------------------------------------------
def test_montgomery_scalars_and_bases(nmx):
    curve, n = R.PALLAS, 256
    p = curve.r
    I = V.instance_of(curve, n, seed=91)
    want = expect(I)
    M = lambda x: x * (1 << 256) % p  # noqa: E731
    mb = lambda xy: util.to_mont_bases(curve.cid, np.frombuffer(bytes(xy), np.uint8).copy()).tobytes()  # noqa: E731
    K = nmx.CommitmentKey.from_host(curve.cid, util.to_mont_bases(curve.cid, I["ck"]), mont=True)
    try:
        for tamper in (False, True):
            ah = int.from_bytes(I["a_hat"], "little") + (1 if tamper else 0)
            exp = expect(I, a_hat=ic.le(ah % p)) if tamper else want
            bm = util.to_mont_scalars(curve.cid, I["b"])
            for b in (bm, dev(bm)):
                ok, ckh, bh = nmx.ipa_verify(K, mb(I["ckc"]), (mb(ic.pt_bytes(I["comm_a"])), False), ic.le(M(I["c"])), b, [mb(x) for x in I["Ls"]],
                                             [mb(x) for x in I["Rs"]], I["infs"], ic.le(M(ah % p)), les(M(r) for r in I["rs"]), mont=True,
                                             want_intermediates=True)
                assert (ok, (ckh.xy, ckh.is_inf), int.from_bytes(bh, "little")) == (exp[0], exp[1], M(exp[2]))
    finally:
        K.close()


@pytest.mark.parametrize("curve", [R.GRUMPKIN, R.VESTA], ids=lambda c: c.name)
@pytest.mark.parametrize("ell", [0, 1, 5, 10])
def test_point_form_equals_vector_form_with_the_eq_table(nmx, curve, ell):
    from nova_amd import fieldvec as fv
    n = 1 << ell
    I = V.instance_of(curve, n, seed=100 + ell)
    fid = fv.SCALAR_FIELD_OF_CURVE[curve.cid]
    point = [int.from_bytes(bytes(x), "little") for x in util.random_scalars(curve.cid, max(ell, 1), seed=200 + ell).reshape(-1, 32)][:ell]
    table_ref = R.eq_evals(curve.r, point) if ell else [1]
    K = key_of(nmx, I)
    try:
        want = expect(I, bi=table_ref)          # (the proof was made for another b: rejected, with known intermediates)
        assert want[2] == V.b_hat_closed(curve.r, point, I["rs"])
        got_point = run(nmx, K, I, point=point)
        assert got_point == want
        if ell:
            table = fv.eq_evals_from_points(fid, np.frombuffer(b"".join(les(point)), np.uint8).copy(), device=True)
            before = table.clone()
            assert run(nmx, K, I, b=table) == got_point
            import torch
            assert torch.equal(table, before)   # b left as it was
        # an honest evaluation claim in the point form: prove against b = eq(point), verify from the point alone
        bt = V.b_array(table_ref)
        tr = ic.IpaTranscript(curve.r)
        Ls, Rs, infs, a_hat = nmx.ipa_prove(K, I["ckc"], dev(I["a"]), dev(bt), tr)
        ai = ic.ints(I["a"])
        J = dict(I, bi=table_ref, c=sum(x * y for x, y in zip(ai, table_ref)) % curve.r, Ls=Ls, Rs=Rs, infs=infs, a_hat=a_hat, rs=list(tr.rs))
        want = expect(J)
        assert want[0] is True and run(nmx, K, J, point=point) == want
    finally:
        K.close()


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors(nmx):
    from nova_amd import _lib
    curve, n = R.GRUMPKIN, 8
    p = curve.r
    I = V.instance_of(curve, n, seed=120)
    K = key_of(nmx, I)
    short = key_of(nmx, I, ck=I["ck"][:4])

    def code(K_, **over):
        with pytest.raises(nmx.NmxError) as e:
            run(nmx, K_, I, **over)
        return e.value.code
    try:
        assert code(K, rs=[I["rs"][0], 0, I["rs"][2]]) == _lib.E_ZERO
        assert code(K, rs=[I["rs"][0], p, I["rs"][2]]) == _lib.E_SCALAR_RANGE
        assert code(K, rs=[I["rs"][0], I["rs"][1], (1 << 256) - 1]) == _lib.E_SCALAR_RANGE
        off = bytearray(I["Ls"][1])
        off[0] ^= 1
        assert code(K, Ls=[I["Ls"][0], bytes(off), I["Ls"][2]]) == _lib.E_POINT
        assert code(K, Rs=[I["Rs"][0], I["Rs"][1], ic.le(curve.p) + I["Rs"][2][32:]]) == _lib.E_POINT   # not canonical
        assert code(short) == _lib.E_HANDLE
        assert code(K, a_hat=ic.le(p)) == _lib.E_SCALAR_RANGE
        K.close()
        assert code(K) == _lib.E_HANDLE                               # an unknown (closed) handle
        # NMX_SCALARS_DEVICE together with the point form, through the C ABI
        import ctypes
        L = _lib.lib()
        z = np.zeros(256, np.uint8)
        v = ctypes.c_uint32(7)
        q = z.ctypes.data
        assert L.nmx_ipa_verify(short.handle, q, q, 0, q, q, 4, q, q, None, q, q, _lib.SCALARS_DEVICE | _lib.IPA_B_IS_POINT, ctypes.byref(v),
                                None, None, None) == _lib.E_ARG and v.value == 7
    finally:
        short.close()


# ---- 5. sharded keys, threads, ordering ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3])
def test_key_sharded_over_logical_devices(nmx, k):
    from nova_amd import _lib
    L = _lib.lib()
    curve, n = R.GRUMPKIN, 1 << 12
    I = V.instance_of(curve, n, seed=130)
    want = expect(I)
    assert nmx.init_devices(k, oversubscribe=True) == k
    assert L.nmx_set_option(b"shard_min_n", 1000) == 0
    try:
        K = key_of(nmx, I)
        try:
            assert len(K.shard_plan()) == k
            assert run(nmx, K, I, b=dev(I["b"])) == want and run(nmx, K, I) == want
            over = V.tampers(I)["b_last"]
            assert run(nmx, K, I, **over) == expect(I, **over)
        finally:
            K.close()
    finally:
        assert L.nmx_set_option(b"shard_min_n", 1 << 20) == 0
        assert nmx.init_devices(1) == 1


def test_three_threads_at_once(nmx):
    setups = []
    for j, (curve, n) in enumerate([(R.GRUMPKIN, 1 << 12), (R.PALLAS, 256), (R.BN254_G1, 1 << 10)]):
        I = V.instance_of(curve, n, seed=140 + j)
        over = V.tampers(I)["a_hat"] if j == 1 else {}
        setups.append((I, key_of(nmx, I), over, expect(I, **over)))
    try:
        assert [w[0] for _i, _k, _o, w in setups] == [True, False, True]
        for rep in range(5):
            got = [None] * 3

            def work(j):
                I, K, over, _w = setups[j]
                try:
                    got[j] = run(nmx, K, I, b=dev(V.b_array(I["bi"])) if rep % 2 else None, **over)
                except Exception as e:  # noqa: BLE001
                    got[j] = e
            ts = [threading.Thread(target=work, args=(j,)) for j in range(3)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            assert got == [w for _i, _k, _o, w in setups], rep
    finally:
        for _i, K, _o, _w in setups:
            K.close()


def test_is_ordered_behind_async_work_on_the_same_thread(nmx):
    """b = b1 + r b2 produced by an NMX_ASYNC launch and handed to the verifier without a synchronisation in between"""
    import torch
    from nova_amd import fieldvec as fv
    curve, n = R.GRUMPKIN, 1 << 16
    p = curve.r
    fid = fv.SCALAR_FIELD_OF_CURVE[curve.cid]
    ck, ckc, a, b = ic.make_instance(curve, n, 150)
    K = nmx.CommitmentKey.from_host(curve.cid, ck)
    try:
        tr = ic.IpaTranscript(p)
        Ls, Rs, infs, a_hat = nmx.ipa_prove(K, ckc, dev(a), dev(b), tr)
        ai, bi = ic.ints(a), ic.ints(b)
        I = dict(curve=curve, n=n, ck=ck, ckc=ckc.tobytes(), a=a, b=b, bi=bi, comm_a=ic.pt(*cref.msm(curve.cid, a, ck, n)),
                 c=sum(x * y for x, y in zip(ai, bi)) % p, Ls=Ls, Rs=Rs, infs=infs, a_hat=a_hat, rs=list(tr.rs))
        want = expect(I)
        assert want[0] is True
        r = util.random_scalars(curve.cid, 1, seed=151)
        ri = ic.ints(r)[0]
        b2 = util.random_scalars(curve.cid, n, seed=152)
        b1 = V.b_array([(x - ri * y) % p for x, y in zip(bi, ic.ints(b2))])
        d1, d2 = dev(b1), dev(b2)
        torch.cuda.synchronize()
        for _ in range(3):
            folded = fv.axpy(fid, d1, d2, r, async_=True)
            assert run(nmx, K, I, b=folded) == want      # anything else in that buffer is not the b of the proof
    finally:
        K.close()


def test_cpp_mirror(nmx):
    from tests.test_ipa_verify_abi import build_cpp
    r = subprocess.run([build_cpp()], capture_output=True, text=True, env=dict(os.environ))
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "ipa_verify mirror ok" in r.stdout
