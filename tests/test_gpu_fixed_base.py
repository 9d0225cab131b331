"""-m gpu: nmx_bases_from_scalars / nmx_bases_setup_from_tau on the device, bit-exact against pyref.mul(c, s % r, B): the scalar set of
tests/fixed_base_common.py at n = 257 on all four curves at c = 4, 8 and 13 in every form (canonical and Montgomery scalars, host and HBM
scalars, the generator and a caller's base in both base forms), read back with nmx_bases_read and used by an MSM; tau keys at their edge
values; sharded tau keys byte-identical to the unsharded one; the KZG identity commit(f) == f(tau) G and its opening relation, which tie
the key, the MSM and poly_eval together without a pairing; and what a key handle must do afterwards."""
import ctypes
import random

import numpy as np
import pytest

from oracle import pyref as R
from tests import fixed_base_common as fb
from tests import util

pytestmark = pytest.mark.gpu
CURVE_IDS = [c.name for c in fb.CURVES]


@pytest.fixture()
def width(nmx):
    """nmx_set_option("fixed_base_c"); the default (8) restored afterwards"""
    from nova_amd import _lib
    L = _lib.lib()

    def set_c(cw):
        assert L.nmx_set_option(b"fixed_base_c", cw) == 0
    yield set_c
    assert L.nmx_set_option(b"fixed_base_c", 8) == 0


def pt(c):
    return (c.xy, int(c.is_inf))


def want_msm(c, scalars, points):
    P = R.msm_naive(c, scalars, points)
    return (R.point_to_xy64(P), 1 if P is R.INF else 0)


def from_scalars_raw(nmx, c, rows, flags, base=None):
    """the C call itself (the Python wrapper ties the forms of scalars and base together): rows on the host, or a CUDA tensor"""
    from nova_amd import _lib
    L = _lib.lib()
    h = ctypes.c_uint64(0)
    ptr = rows.data_ptr() if hasattr(rows, "data_ptr") else rows.ctypes.data
    n = (rows.numel() if hasattr(rows, "numel") else rows.size) // 32
    rc = L.nmx_bases_from_scalars(c.cid, None if base is None else base.ctypes.data, ptr, n, flags, ctypes.byref(h))
    assert rc == 0, L.nmx_last_error().decode()
    return nmx.CommitmentKey(c.cid, h.value, n, bytes(64))


@pytest.mark.parametrize("cw", fb.WIDTHS)
@pytest.mark.parametrize("c", fb.CURVES, ids=CURVE_IDS)
def test_from_scalars_every_form(nmx, width, c, cw):
    import torch
    from nova_amd import _lib
    width(cw)
    n = 257
    s = fb.scalar_set(c, cw, n)
    G7 = R.mul(c, 7, (c.gx, c.gy))
    g = nmx.DlogGroup(c.cid)
    msm_s = [random.Random(cw).randrange(c.r) for _ in range(n)]
    M, D, BM, PRE = _lib.SCALARS_MONT, _lib.SCALARS_DEVICE, _lib.BASES_MONT, _lib.BASES_PRECOMPUTE
    # (Montgomery scalars, HBM scalars, base, Montgomery base, window tables): every option in both states, every form of the base
    for mont, dev, B, bmont, pre in ((False, False, None, False, True), (True, True, None, False, False), (False, True, G7, False, True),
                                     (True, False, G7, True, True), (True, False, G7, False, False), (False, False, G7, True, False)):
        rows = fb.scalar_rows(c, s, mont)
        arg = torch.from_numpy(rows.copy()).cuda() if dev else rows
        flags = (M if mont else 0) | (D if dev else 0) | (BM if bmont else 0) | (PRE if pre else 0)
        key = from_scalars_raw(nmx, c, arg, flags, None if B is None else fb.base_bytes(c, B, bmont))
        want = fb.expect_points(c, s, B)
        got = key.read(0, n)
        assert np.array_equal(got, fb.xy64_rows(want)), (mont, dev, B is not None, bmont)
        for i in (0, 1, 2, 255):
            assert not got[i].any(), "a zero scalar must read back as 64 zero bytes"
        if B is None or pre:
            assert pt(g.vartime_multiscalar_mul(fb.scalar_rows(c, msm_s), key)) == want_msm(c, msm_s, want), (mont, dev, pre)
            assert pt(g.vartime_multiscalar_mul(fb.scalar_rows(c, msm_s[:9]), key, offset=248)) == want_msm(c, msm_s[:9], want[248:257])
        key.close()


def test_from_scalars_python_wrapper_and_small_sizes(nmx):
    c = R.PALLAS
    G7 = R.mul(c, 7, (c.gx, c.gy))
    rng = random.Random(3)
    for n in (1, 2, 256):
        s = [rng.randrange(c.r) for _ in range(n)]
        for mont in (False, True):
            key = nmx.CommitmentKey.from_scalars(c.cid, fb.scalar_rows(c, s, mont), base=fb.base_bytes(c, G7, mont), mont=mont)
            assert len(key) == n and np.array_equal(key.read(0, n), fb.xy64_rows(fb.expect_points(c, s, G7)))
            key.close()


@pytest.mark.parametrize("c", fb.CURVES, ids=CURVE_IDS)
def test_setup_from_tau_edge_values(nmx, c):
    G, O = (c.gx, c.gy), R.INF
    mG = R.neg(c, G)
    for tau, n, want in ((0, 8, [G] + [O] * 7), (1, 8, [G] * 8), (c.r - 1, 8, [G, mG] * 4)):
        for mont in (False, True):
            key = nmx.CommitmentKey.setup_from_tau(c.cid, n, fb.scalar_rows(c, [tau], mont), mont=mont)
            assert np.array_equal(key.read(0, n), fb.xy64_rows(want)), (tau, mont)
            key.close()


@pytest.mark.parametrize("c", fb.CURVES, ids=CURVE_IDS)
def test_setup_from_tau_two_walks_every_window(nmx, width, c):
    """tau = 2 at n = 300: a single set bit through every window and digit position, and from i = 254 / 255 on the reduction mod r; the
    raw call (no rounding of n), at a width that divides nothing evenly and at the default"""
    from nova_amd import _lib
    L = _lib.lib()
    want = fb.xy64_rows(fb.expect_points(c, fb.tau_powers(c, 2, 300)))
    for cw in (13, 8):
        width(cw)
        h = ctypes.c_uint64(0)
        t = fb.scalar_rows(c, [2])
        assert L.nmx_bases_setup_from_tau(c.cid, t.ctypes.data, 300, 0, ctypes.byref(h)) == 0, L.nmx_last_error().decode()
        key = nmx.CommitmentKey(c.cid, h.value, 300, bytes(64))
        assert np.array_equal(key.read(0, 300), want), cw
        key.close()


@pytest.mark.parametrize("c", [R.BN254_G1, R.VESTA], ids=lambda c: c.name)
def test_setup_from_tau_random_sizes(nmx, c):
    from nova_amd import _lib
    L = _lib.lib()
    tau = random.Random(11 + c.cid).randrange(2, c.r)
    want = fb.xy64_rows(fb.expect_points(c, fb.tau_powers(c, tau, 513)))
    for n in (1, 2, 256, 513):
        h = ctypes.c_uint64(0)
        mont = n in (2, 513)
        t = fb.scalar_rows(c, [tau], mont)
        flags = (_lib.SCALARS_MONT if mont else 0) | (_lib.BASES_PRECOMPUTE if n != 256 else 0)
        assert L.nmx_bases_setup_from_tau(c.cid, t.ctypes.data, n, flags, ctypes.byref(h)) == 0, L.nmx_last_error().decode()
        key = nmx.CommitmentKey(c.cid, h.value, n, bytes(64))
        assert key.registered_len() == n and np.array_equal(key.read(0, n), want[:n]), n
        key.close()
    # the wrappers round n as the reference does (n.next_power_of_two(), hyperkzg.rs:361)
    for n, num in ((0, 1), (1, 1), (3, 4), (200, 256)):
        key = nmx.CommitmentEngine(c.cid).setup_from_tau(n, fb.scalar_rows(c, [tau]))
        assert len(key) == num == key.registered_len() and np.array_equal(key.read(0, num), want[:num])
        key.close()


@pytest.fixture()
def sharded(nmx):
    """k logical devices on the one GPU, as tests/test_gpu_multidev.py enters them; every key from 256 points up sharded"""
    from nova_amd import _lib
    L = _lib.lib()

    def enter(k):
        assert nmx.init_devices(k, oversubscribe=True) == k
        assert L.nmx_set_option(b"shard_min_n", 256) == 0
        return L
    yield enter
    assert nmx.init_devices(1) == 1
    assert L.nmx_set_option(b"shard_min_n", 1 << 20) == 0


@pytest.mark.parametrize("k", [2, 3])
def test_sharded_tau_key_is_byte_identical(nmx, sharded, k):
    from nova_amd import _lib
    c = R.BN254_G1
    n = 700
    tau = random.Random(21).randrange(2, c.r)
    t = fb.scalar_rows(c, [tau])

    def make():
        h = ctypes.c_uint64(0)
        L = _lib.lib()
        assert L.nmx_bases_setup_from_tau(c.cid, t.ctypes.data, n, _lib.BASES_PRECOMPUTE, ctypes.byref(h)) == 0, L.nmx_last_error().decode()
        return nmx.CommitmentKey(c.cid, h.value, n, bytes(64))
    whole = make()
    assert len(whole.shard_plan()) == 1
    ref = whole.read(0, n)
    assert np.array_equal(ref, fb.xy64_rows(fb.expect_points(c, fb.tau_powers(c, tau, n))))
    sharded(k)
    key = make()
    plan = key.shard_plan()
    assert len(plan) == k and sum(p[2] for p in plan) == n, plan
    assert key.read(0, n).tobytes() == ref.tobytes()
    sc = util.random_scalars(c.cid, n)
    g = nmx.DlogGroup(c.cid)
    assert pt(g.vartime_multiscalar_mul(sc, key)) == pt(g.vartime_multiscalar_mul(sc, whole))
    # a key from host scalars is cut the same way: shard p reads its own slice
    s = fb.tau_powers(c, tau, n)
    skey = nmx.CommitmentKey.from_scalars(c.cid, fb.scalar_rows(c, s))
    assert len(skey.shard_plan()) == k and skey.read(0, n).tobytes() == ref.tobytes()
    for x in (key, skey, whole):
        x.close()


@pytest.mark.parametrize("c", [R.BN254_G1, R.PALLAS], ids=lambda c: c.name)
def test_kzg_identity_ties_key_msm_and_poly_eval(nmx, c):
    """commit(ck, f) == f(tau) G for a random f of 512 coefficients, and for w = div_by_monomial(f, u):
    commit(f) - f(u) G == (tau - u) commit(w) -- both sides as points, no pairing"""
    rng = random.Random(31 + c.cid)
    n = 512
    tau, u = rng.randrange(2, c.r), rng.randrange(c.r)
    f = [rng.randrange(c.r) for _ in range(n)]
    G = (c.gx, c.gy)
    ce = nmx.CommitmentEngine(c.cid)
    ck = ce.setup_from_tau(n, fb.scalar_rows(c, [tau]))
    cf = ce.commit(ck, fb.scalar_rows(c, f))
    assert not cf.is_inf and cf.xy == R.point_to_xy64(R.mul(c, R.poly_eval(c.r, f, tau), G))
    w = R.div_by_monomial(c.r, f, u)
    cw = ce.commit(ck, fb.scalar_rows(c, w))
    lhs = R.add(c, R.xy64_to_point(cf.xy), R.neg(c, R.mul(c, R.poly_eval(c.r, f, u), G)))
    rhs = R.mul(c, (tau - u) % c.r, R.xy64_to_point(cw.xy))
    assert lhs == rhs and lhs is not R.INF
    ck.close()


def bad_rows(c, rows, i):
    out = rows.copy()
    out[i] = np.frombuffer(int(c.r).to_bytes(32, "little"), np.uint8)
    return out


def test_key_state_range_error_precompute_and_unregister(nmx):
    import torch
    from nova_amd import _lib
    L = _lib.lib()
    c = R.GRUMPKIN
    n = 300
    s = fb.scalar_set(c, 8, n)
    rows = fb.scalar_rows(c, s)
    # a device scalar >= r: NMX_E_SCALAR_RANGE, *handle untouched, nothing registered (handles are handed out in sequence: the key made
    # after the refused calls gets the number after the key made before them)
    before = nmx.CommitmentKey.from_scalars(c.cid, rows[:4])
    d = torch.from_numpy(bad_rows(c, rows, n - 2)).cuda()
    h = ctypes.c_uint64(12345)
    for fl in (_lib.SCALARS_DEVICE, _lib.SCALARS_DEVICE | _lib.SCALARS_MONT | _lib.BASES_PRECOMPUTE):
        assert L.nmx_bases_from_scalars(c.cid, None, d.data_ptr(), n, fl, ctypes.byref(h)) == _lib.E_SCALAR_RANGE
        assert h.value == 12345
    # with and without window tables: the same key, the same MSM results
    g = nmx.DlogGroup(c.cid)
    sc = util.random_scalars(c.cid, n)
    keys = [nmx.CommitmentKey.from_scalars(c.cid, rows, precompute=p) for p in (True, False)]
    assert keys[0].handle == before.handle + 1, "a refused call registered something"
    before.close()
    assert keys[0].read(0, n).tobytes() == keys[1].read(0, n).tobytes()
    res = [pt(g.vartime_multiscalar_mul(sc, k)) for k in keys]
    assert res[0] == res[1] == want_msm(c, [int.from_bytes(bytes(r), "little") for r in sc], fb.expect_points(c, s))
    # nmx_bases_unregister frees the key: the handle is gone, a second unregister is refused
    handle = keys[0].handle
    keys[0].close()
    out = np.zeros((1, 64), np.uint8)
    assert L.nmx_bases_read(handle, 0, 1, out.ctypes.data) == _lib.E_HANDLE and L.nmx_bases_unregister(handle) == _lib.E_HANDLE
    keys[1].close()
