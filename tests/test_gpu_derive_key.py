"""-m gpu: nmx_bases_derive_by_address on the device.  The source key is CommitmentKey.from_scalars(curve, s) for known s_i, so derived[j] is
pyref.mul(c, sum of s_i over the index's entries mod r, G) and the identity when that sum is 0 mod r; every comparison is on the bytes of
read(), bit-exact.  The smallest shapes at which each stage can go wrong: all four curves; table sizes around the normalisation's block of 256;
bucket sizes around derive_lmax = 4 up to the extra tasks, the big list and the fold passes with T = 64, 512 and 4096; the group-law edges on
one index; a permutation (no arithmetic oracle at all); identity source rows, a prefix of a longer key, a derivation from a derived key, the
source unregistered; addresses wider than 16 bits; host against HBM addresses; the lookup identity commit(ck, L) == commit(derived, T) the
call exists for; and the errors only the device path can raise."""
import ctypes
import random

import numpy as np
import pytest

from oracle import pyref as R
from tests import derive_key_common as dk
from tests import fixed_base_common as fb

pytestmark = pytest.mark.gpu
CURVE_IDS = [c.name for c in dk.CURVES]
TWO = [R.BN254_G1, R.PALLAS]
TWO_IDS = [c.name for c in TWO]


def dev_u64(a):
    """a CUDA tensor holding the 64-bit words of `a`"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint64)
    try:
        return torch.from_numpy(a.copy()).cuda()
    except (TypeError, RuntimeError):   # a torch without uint64 tensors: the same bytes as int64
        return torch.from_numpy(a.view(np.int64).copy()).cuda()


@pytest.fixture()
def lmax(nmx):
    """nmx_set_option("derive_lmax"); the default rule (0) restored afterwards"""
    from nova_amd import _lib
    L = _lib.lib()

    def set_l(v):
        assert L.nmx_set_option(b"derive_lmax", v) == 0
    yield set_l
    assert L.nmx_set_option(b"derive_lmax", 0) == 0


def source(nmx, c, scalars, precompute=True):
    return nmx.CommitmentKey.from_scalars(c.cid, fb.scalar_rows(c, scalars), precompute=precompute)


def check(nmx, c, scalars, addr, T, src=None, precompute=True, device=False):
    """derive over key[i] = scalars[i] G and compare the whole derived key with the expected bytes; returns the derived key's bytes"""
    own = src is None
    src = source(nmx, c, scalars) if own else src
    a = dev_u64(addr) if device else np.asarray(addr, dtype=np.uint64)
    d = src.derive_by_address(a, T, precompute=precompute)
    try:
        assert len(d) == T and d.registered_len() == T and d.h == src.h and d.mont == src.mont and d.curve == src.curve
        got = d.read(0, T)
        assert np.array_equal(got, dk.expect_bytes(c, scalars, addr, T))
    finally:
        d.close()
        if own:
            src.close()
    return got


@pytest.mark.parametrize("c", dk.CURVES, ids=CURVE_IDS)
def test_all_four_curves(nmx, c):
    n, T = 300, 17
    rng = random.Random(c.cid)
    addr = [rng.randrange(T) for _ in range(n)]
    check(nmx, c, list(range(1, n + 1)), addr, T)


@pytest.mark.parametrize("T", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_normalisation_edges(nmx, c, T):
    """n = 64; at 513 every address is below 256, so the lanes of block 1 are all identity and block 2 holds one identity lane"""
    rng = random.Random(T)
    addr = [rng.randrange(min(T, 256)) for _ in range(64)]
    addr[0] = 0
    if T != 513:
        addr[63] = T - 1
    got = check(nmx, c, list(range(1, 65)), addr, T)
    if T == 513:
        assert not got[256:].any()


@pytest.mark.parametrize("Lh", [1, 4, 5, 256, 257, 2049, 16385])
@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_bucket_size_edges_at_lmax_4(nmx, lmax, c, Lh):
    """one index holds L entries, three others one each: no split (1, 4), two tasks (5), 64 tasks (256: the last size without the big
    list), 65 (257: the T = 64 pass), 513 (2049: T = 512) and 4097 (16385: T = 4096)"""
    lmax(4)
    addr, s = dk.heavy_case(Lh)
    check(nmx, c, s, addr, 8, device=(Lh % 2 == 0))


@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_every_point_on_one_index_at_the_default_lmax(nmx, c):
    n = 1 << 15
    check(nmx, c, list(range(1, n + 1)), [0] * n, 1)


@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_group_law_edges_on_one_index(nmx, c):
    s = [7, c.r - 7, 5, 5, 9, 9, c.r - 9, 11]
    addr = [0, 0, 1, 1, 2, 2, 2, 3]
    got = check(nmx, c, s, addr, 4)
    assert not got[0].any(), "s and r - s must give the all-zero encoding"
    assert got[1].tobytes() == R.point_to_xy64(R.mul(c, 10, (c.gx, c.gy))) and got[2].tobytes() == R.point_to_xy64(R.mul(c, 9, (c.gx, c.gy)))
    # each edge alone on a table of one index
    check(nmx, c, [7, c.r - 7], [0, 0], 1)
    check(nmx, c, [5, 5], [0, 0], 1)
    check(nmx, c, [9, 9, c.r - 9], [0, 0, 0], 1)


@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_permutation_moves_rows_without_arithmetic(nmx, c):
    """n = table_size = 1000 over a generated key: the derived key's bytes are the source's rows permuted"""
    n = 1000
    src = nmx.CommitmentKey.generate(c.cid, n)
    perm = list(range(n))
    random.Random(9 + c.cid).shuffle(perm)
    d = src.derive_by_address(np.asarray(perm, dtype=np.uint64), n)
    rows, got = src.read(0, n), d.read(0, n)
    assert np.array_equal(got[np.asarray(perm)], rows) and got.any(axis=1).all()
    assert d.h == src.h
    d.close()
    src.close()


@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_source_subsets(nmx, c):
    rng = random.Random(40 + c.cid)
    # identity source rows (zero scalars) contribute nothing
    s = [rng.randrange(1, 1000) if i % 3 else 0 for i in range(90)]
    addr = [rng.randrange(7) for _ in range(90)]
    check(nmx, c, s, addr, 7)
    # a prefix n = 100 of a 256-point key ignores the rest
    s = [rng.randrange(1, c.r) for _ in range(256)]
    src = source(nmx, c, s)
    addr = [rng.randrange(10) for _ in range(100)]
    check(nmx, c, s[:100], addr, 10, src=src)
    # a derivation from a derived key (which holds identity rows: indices 10 .. 19 are empty), then the same with the first source gone
    d1 = src.derive_by_address(np.asarray(addr, dtype=np.uint64), 20)
    sums1 = dk.expect_sums(c, s[:100], addr, 20)
    assert sums1[10:] == [0] * 10
    addr2 = [rng.randrange(4) for _ in range(20)]
    want2 = dk.expect_bytes(c, sums1, addr2, 4)
    d2 = d1.derive_by_address(addr2, 4)
    assert np.array_equal(d2.read(0, 4), want2)
    d2.close()
    src.close()
    assert np.array_equal(d1.read(0, 20), dk.expect_bytes(c, s[:100], addr, 20)), "the derived key must own its memory"
    d3 = d1.derive_by_address(dev_u64(addr2), 4, precompute=False)
    assert np.array_equal(d3.read(0, 4), want2)
    d3.close()
    d1.close()


@pytest.mark.parametrize("T,pre", [((1 << 16) + 1, True), (1 << 20, False)])
@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_address_widths(nmx, c, T, pre):
    """addresses of 17 and 20 bits, 0 and table_size - 1 among them; n = 200"""
    rng = random.Random(T + c.cid)
    addr = [rng.randrange(T) for _ in range(200)]
    addr[5], addr[6], addr[199] = 0, T - 1, T - 1
    s = list(range(1, 201))
    src = source(nmx, c, s)
    d = src.derive_by_address(dev_u64(addr) if pre else np.asarray(addr, dtype=np.uint64), T, precompute=pre)
    got = d.read(0, T)
    want = np.zeros((T, 64), np.uint8)
    sums = dk.expect_sums(c, s, addr, T)
    used = sorted(set(addr))
    want[used] = fb.xy64_rows(fb.expect_points(c, [sums[j] for j in used]))
    assert np.array_equal(got, want)
    d.close()
    src.close()


@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_host_and_hbm_addresses_give_the_same_bytes(nmx, c):
    rng = random.Random(50 + c.cid)
    n, T = 700, 300
    s = [rng.randrange(1, c.r) for _ in range(n)]
    addr = [rng.randrange(T) for _ in range(n)]
    src = source(nmx, c, s)
    host = check(nmx, c, s, addr, T, src=src)
    hbm = check(nmx, c, s, addr, T, src=src, device=True, precompute=False)
    assert host.tobytes() == hbm.tobytes()
    # the engine's method is the key's
    d = nmx.CommitmentEngine(c.cid).ck_derive_by_address(src, addr, T)
    assert d.read(0, T).tobytes() == host.tobytes()
    d.close()
    src.close()


@pytest.mark.parametrize("skew", [False, True], ids=["uniform", "three_quarters_on_0"])
@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_lookup_identity(nmx, c, skew):
    """Comm(L, ck) == Comm(T, derived) for L[i] = T[addr[i]]: n = 2^12, table_size = 2^8, with and without a blinding term, derived keys
    with and without window tables, L gathered on the device; commit_sparse_binary over the derived key against the sums of its indices"""
    import torch
    from nova_amd import fieldvec as fv
    n, T = 1 << 12, 1 << 8
    rng = random.Random(60 + c.cid + (7 if skew else 0))
    addr = [0 if (skew and i % 4) else rng.randrange(T) for i in range(n)]
    Tv = [rng.randrange(c.r) for _ in range(T)]
    fid = fv.SCALAR_FIELD_OF_CURVE[c.cid]
    T_rows = fb.scalar_rows(c, Tv)
    L_dev = fv.gather(fid, torch.from_numpy(T_rows.copy()).cuda(), torch.from_numpy(fb.scalar_rows(c, addr)).cuda())
    assert L_dev.cpu().numpy().reshape(-1, 32).tobytes() == fb.scalar_rows(c, [Tv[a] for a in addr]).tobytes()
    ce = nmx.CommitmentEngine(c.cid)
    ck = nmx.CommitmentKey.generate(c.cid, n)          # P_i = (1 + i) G, h = P_n
    r = fb.scalar_rows(c, [rng.randrange(1, c.r)])
    want = [ce.commit(ck, L_dev), ce.commit(ck, L_dev, r)]
    assert not want[0].is_inf and want[0] != want[1]
    sums = dk.expect_sums(c, list(range(1, n + 1)), addr, T)
    for pre, dev in ((True, False), (False, True)):
        d = ce.ck_derive_by_address(ck, dev_u64(addr) if dev else addr, T, precompute=pre)
        assert [ce.commit(d, T_rows), ce.commit(d, T_rows, r)] == want, (pre, dev)
        assert [ce.commit(d, torch.from_numpy(T_rows.copy()).cuda()), ce.batch_commit(d, [T_rows, T_rows[:9]])[0]] == [want[0], want[0]]
        idx = [0, 3, 77, T - 1]
        got = ce.commit_sparse_binary(d, idx)
        P = R.mul(c, sum(sums[j] for j in idx) % c.r, (c.gx, c.gy))
        assert (got.xy, got.is_inf) == (R.point_to_xy64(P), P is R.INF)
        d.close()
    ck.close()


def test_errors_on_the_device_path(nmx):
    from nova_amd import _lib
    L = _lib.lib()
    c = R.BN254_G1
    s = list(range(1, 9))
    src = source(nmx, c, s)
    T = 5
    bad = dev_u64([0, 1, 2, 3, 4, 0, 1, T])
    good = dev_u64([0, 1, 2, 3, 4, 0, 1, T - 1])
    h = ctypes.c_uint64(12345)
    for fl in (_lib.SCALARS_DEVICE, _lib.SCALARS_DEVICE | _lib.BASES_PRECOMPUTE):
        assert L.nmx_bases_derive_by_address(src.handle, bad.data_ptr(), 8, T, fl, ctypes.byref(h)) == _lib.E_ARG
        assert h.value == 12345
    # a valid call right after succeeds, and its handle is the next in sequence: the refused calls registered nothing
    assert L.nmx_bases_derive_by_address(src.handle, good.data_ptr(), 8, T, _lib.SCALARS_DEVICE, ctypes.byref(h)) == 0, L.nmx_last_error().decode()
    assert h.value == src.handle + 1
    d = nmx.CommitmentKey(c.cid, h.value, T, bytes(64))
    assert np.array_equal(d.read(0, T), dk.expect_bytes(c, s, [0, 1, 2, 3, 4, 0, 1, T - 1], T))
    d.close()
    # n one above the key length: the reference's InvalidCommitmentKeyLength
    h = ctypes.c_uint64(12345)
    nine = np.zeros(9, np.uint64)
    assert L.nmx_bases_derive_by_address(src.handle, nine.ctypes.data, 9, T, 0, ctypes.byref(h)) == _lib.E_HANDLE and h.value == 12345
    assert L.nmx_bases_derive_by_address(src.handle, dev_u64(nine).data_ptr(), 9, T, _lib.SCALARS_DEVICE, ctypes.byref(h)) == _lib.E_HANDLE and h.value == 12345
    # the option's range
    assert L.nmx_set_option(b"derive_lmax", 1) == _lib.E_ARG and L.nmx_set_option(b"derive_lmax", 1025) == _lib.E_ARG
    assert L.nmx_set_option(b"derive_lmax", 1024) == 0 and L.nmx_set_option(b"derive_lmax", 0) == 0
    src.close()
