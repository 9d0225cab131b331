"""-m gpu: nmx_bases_fold / nmx_bases_scale / nmx_bases_concat on the device.  The source key is CommitmentKey.from_scalars(curve, s) for known
s_i, so a folded row is pyref.mul(c, (w1 s_i + w2 s_{i+h}) mod r, G), a scaled row pyref.mul(c, r s_i mod r, G) and the identity when that
scalar is 0; every comparison is on the bytes of read(), bit-exact.  The smallest shapes at which each part can go wrong: output counts
around the block of 256 lanes, an odd n, all four curves, the digit-edge weights and pairs, equal / opposite / identity source rows and an
all-identity result, both forms of the weights, concat around the block edge and with 8 ranges, the result used as a key by every consumer,
the inner-product argument's round identity and the fold-to-one identity, and the refusals that need a key."""
import ctypes
import random

import numpy as np
import pytest

from oracle import pyref as R
from tests import fixed_base_common as fb
from tests import key_ext_common as kx
from tests.test_gpu_fixed_base import sharded  # noqa: F401  (k logical devices on the one GPU; restores init_devices(1) and shard_min_n)

pytestmark = pytest.mark.gpu
TWO = [R.BN254_G1, R.PALLAS]
TWO_IDS = [c.name for c in TWO]
OTHER = [R.GRUMPKIN, R.VESTA]
OTHER_IDS = [c.name for c in OTHER]


def source(nmx, c, scalars, precompute=False):
    return nmx.CommitmentKey.from_scalars(c.cid, fb.scalar_rows(c, scalars), precompute=precompute)


def w32(c, v, mont=False):
    return fb.scalar_rows(c, [v], mont=mont)


def G(c):
    return (c.gx, c.gy)


def as_point(com):
    return R.INF if com.is_inf else R.xy64_to_point(com.xy)


def check_fold(nmx, c, src, s, w1, w2, n=None, **kw):
    """fold src (key[i] = s[i] G) and compare the whole result with the expected bytes; returns the folded key"""
    n = len(s) if n is None else n
    assert len(src) == n
    f = src.fold(w32(c, w1), w32(c, w2), **kw)
    assert len(f) == n // 2 == f.registered_len() and f.h == src.h and f.mont == src.mont and f.curve == src.curve and f.handle != src.handle
    assert np.array_equal(f.read(0, n // 2), kx.rows(c, kx.fold_scalars(c, s, w1, w2, n))), (hex(w1), hex(w2))
    return f


def check_scale(nmx, c, src, s, r, **kw):
    g = src.scale(w32(c, r), **kw)
    assert len(g) == len(s) == g.registered_len() and g.h == src.h and g.mont == src.mont and g.curve == src.curve
    assert np.array_equal(g.read(0, len(s)), kx.rows(c, kx.scale_scalars(c, s, r))), hex(r)
    return g


@pytest.mark.parametrize("h", kx.SIZES)
@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_fold_sizes(nmx, c, h):
    """h outputs from n = 2 h points (n = 2 h + 1 at h = 255: the last point is ignored); from h = 5 on the source holds an equal pair, an
    opposite pair and identity rows on either side and on both"""
    n = 2 * h + (1 if h == 255 else 0)
    s = kx.source_scalars(c, 2 * h, seed=h) + ([12345] if n % 2 else [])
    src = source(nmx, c, s)
    check_fold(nmx, c, src, s, kx.random_weight(c, 1), kx.random_weight(c, 2)).close()
    src.close()


@pytest.mark.parametrize("n", kx.SIZES)
@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_scale_sizes(nmx, c, n):
    s = kx.source_scalars(c, n, seed=n)
    src = source(nmx, c, s)
    check_scale(nmx, c, src, s, kx.random_weight(c, 3)).close()
    src.close()


@pytest.mark.parametrize("c", OTHER, ids=OTHER_IDS)
def test_the_other_two_curves(nmx, c):
    s = kx.source_scalars(c, 514, seed=4)
    src = source(nmx, c, s)
    check_fold(nmx, c, src, s, kx.random_weight(c, 1), kx.random_weight(c, 2)).close()
    check_scale(nmx, c, src, s, kx.random_weight(c, 3)).close()
    src.close()


@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_digit_edge_weights_and_pairs(nmx, c):
    s = kx.source_scalars(c, 12, seed=3)
    src = source(nmx, c, s)
    for r in kx.edge_weights(c):
        check_scale(nmx, c, src, s, r).close()
    for w1, w2 in kx.all_pairs(c):
        check_fold(nmx, c, src, s, w1, w2).close()
    src.close()


@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_group_law_edges_and_the_identity_mark(nmx, c):
    """equal rows under (w, w) and (w, r - w), opposite rows, identity rows; an all-identity result is still a key: one MSM over a key with
    identity rows equals the oracle's (the key must be marked as holding them, or the MSM would add the all-zero rows as points)"""
    w = kx.random_weight(c, 5)
    ce = nmx.CommitmentEngine(c.cid)
    s = [7, 9, 11, 0, 5, 0, 21] + [7, c.r - 9, 13, 6, 0, 0, 22]       # equal, opposite, ordinary, identity in L, in R, in both, ordinary
    src = source(nmx, c, s)
    for w1, w2 in ((w, w), (w, c.r - w), (w, 3), (0, w), (w, 0), (0, 0)):
        f = check_fold(nmx, c, src, s, w1, w2)
        ks = kx.fold_scalars(c, s, w1, w2)
        v = [random.Random(i).randrange(1, c.r) for i in range(7)]
        want = R.mul(c, sum(a * b for a, b in zip(v, ks)) % c.r, G(c))
        assert as_point(ce.commit(f, fb.scalar_rows(c, v))) == want, (hex(w1), hex(w2))
        if (w1, w2) == (0, 0):
            assert not f.read(0, 7).any() and want is R.INF
        f.close()
    z = check_scale(nmx, c, src, s, 0)
    assert not z.read(0, 14).any() and ce.commit(z, fb.scalar_rows(c, list(range(1, 15)))).is_inf
    z.close()
    g = check_scale(nmx, c, src, s, c.r - 1, precompute=True)                # identity rows stay identity rows; with window tables
    v = list(range(1, 15))
    assert as_point(ce.commit(g, fb.scalar_rows(c, v))) == R.mul(c, sum(a * (c.r - b) for a, b in zip(v, s)) % c.r, G(c))
    g.close()
    src.close()


@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_canonical_and_montgomery_weights_give_the_same_bytes(nmx, c):
    s = kx.source_scalars(c, 40, seed=6)
    src = source(nmx, c, s)
    w1, w2 = kx.random_weight(c, 6), c.r - 1
    f = check_fold(nmx, c, src, s, w1, w2)
    fm = src.fold(w32(c, w1, mont=True), w32(c, w2, mont=True), mont=True)
    assert fm.read(0, 20).tobytes() == f.read(0, 20).tobytes()
    g = check_scale(nmx, c, src, s, w1)
    gm = src.scale(w32(c, w1, mont=True), mont=True)
    assert gm.read(0, 40).tobytes() == g.read(0, 40).tobytes()
    for k in (f, fm, g, gm, src):
        k.close()


@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_concat(nmx, c):
    n = 600
    s = kx.source_scalars(c, n, seed=8)
    src = source(nmx, c, s)
    rows = src.read(0, n)
    assert np.array_equal(rows, kx.rows(c, s))
    for cut in (1, 255, 256, 257, n - 1):
        lo, hi = src.split_at(cut)
        assert (len(lo), len(hi)) == (cut, n - cut) == (lo.registered_len(), hi.registered_len()) and lo.h == src.h and hi.h == src.h
        assert np.array_equal(lo.read(0, cut), rows[:cut]) and np.array_equal(hi.read(0, n - cut), rows[cut:])
        back = lo.combine(hi)
        assert len(back) == n and back.read(0, n).tobytes() == rows.tobytes()
        for k in (lo, hi, back):
            k.close()
    # eight ranges, overlapping and out of order, one of a single row, from two keys -- one of them derived (it holds identity rows)
    addr = [i % 5 for i in range(20)]
    der = src.derive_by_address(np.asarray(addr, dtype=np.uint64), 9, precompute=False)
    drows = der.read(0, 9)
    assert not drows[5:].any() and drows[:5].any(axis=1).all()
    parts = [(src, 300, 200), (der, 3, 4), (src, 0, 1), (src, 255, 2), (der, 0, 9), (src, 599, 1), (src, 100, 300), (der, 8, 1)]
    cat = src.concat(parts, precompute=True)
    want = np.concatenate([(rows if k is src else drows)[o:o + m] for k, o, m in parts])
    assert len(cat) == len(want) == cat.registered_len() and np.array_equal(cat.read(0, len(want)), want)
    # ... which an MSM over it must skip: the result counts as holding identity points
    ks = [0] * 5
    for a, x in zip(addr, s):
        ks[a] = (ks[a] + x) % c.r
    ks += [0] * 4
    flat = [x for k, o, m in parts for x in (s if k is src else ks)[o:o + m]]
    v = [random.Random(i).randrange(1, c.r) for i in range(len(flat))]
    got = nmx.CommitmentEngine(c.cid).commit(cat, fb.scalar_rows(c, v))
    assert as_point(got) == R.mul(c, sum(a * b for a, b in zip(v, flat)) % c.r, G(c))
    # unregistering the sources leaves the result readable
    der.close()
    src.close()
    assert np.array_equal(cat.read(0, len(want)), want)
    cat.close()


@pytest.mark.parametrize("pre", [False, True], ids=["no_tables", "tables"])
@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_the_result_is_a_key(nmx, c, pre):
    """commit, fused batch and sparse commit over a folded key; a fold of a fold; derive-by-address from a scaled key"""
    n = 1024
    rng = random.Random(90 + c.cid)
    s = [rng.randrange(1, c.r) for _ in range(n)]
    src = source(nmx, c, s)
    ce = nmx.CommitmentEngine(c.cid)
    w1, w2 = kx.random_weight(c, 7), kx.random_weight(c, 8)
    f = src.fold(w32(c, w1), w32(c, w2), precompute=pre)
    ks = kx.fold_scalars(c, s, w1, w2)
    vs = [[rng.randrange(c.r) for _ in range(m)] for m in (512, 300, 17, 2)]
    want = [R.mul(c, sum(a * b for a, b in zip(v, ks)) % c.r, G(c)) for v in vs]
    assert as_point(ce.commit(f, fb.scalar_rows(c, vs[0]))) == want[0]
    assert [as_point(x) for x in ce.batch_commit(f, [fb.scalar_rows(c, v) for v in vs])] == want
    idx = [0, 3, 255, 256, 511]
    assert as_point(ce.commit_sparse_binary(f, idx)) == R.mul(c, sum(ks[j] for j in idx) % c.r, G(c))
    ff = f.fold(w32(c, w2), w32(c, w1), precompute=pre)
    assert np.array_equal(ff.read(0, 256), kx.rows(c, kx.fold_scalars(c, ks, w2, w1)))
    g = src.scale(w32(c, w1), precompute=pre)
    addr = [rng.randrange(16) for _ in range(n)]
    d = g.derive_by_address(np.asarray(addr, dtype=np.uint64), 16, precompute=pre)
    sums = [0] * 16
    for a, x in zip(addr, s):
        sums[a] = (sums[a] + w1 * x) % c.r
    assert np.array_equal(d.read(0, 16), kx.rows(c, sums))
    for k in (d, g, ff, f, src):
        k.close()


@pytest.mark.parametrize("n", [16, 512])
@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_ipa_round_identity(nmx, c, n):
    """ipa_pc.rs:212-255: with a' = a_L r + a_R r^-1 and ck' = fold(ck, r^-1, r),
    commit(ck', a') == commit(ck, a) + r^2 <a_L, ck_R> + r^-2 <a_R, ck_L>; every inner product is an MSM over a key in HBM"""
    rng = random.Random(n + c.cid)
    h = n // 2
    ck = source(nmx, c, [rng.randrange(1, c.r) for _ in range(n)], precompute=True)
    a = [rng.randrange(c.r) for _ in range(n)]
    r = rng.randrange(2, c.r)
    ri = pow(r, -1, c.r)
    folded = ck.fold(w32(c, ri), w32(c, r))
    a2 = [(a[i] * r + a[h + i] * ri) % c.r for i in range(h)]
    ce, g = nmx.CommitmentEngine(c.cid), nmx.DlogGroup(c.cid)
    lhs = as_point(ce.commit(folded, fb.scalar_rows(c, a2)))
    Lp = as_point(g.vartime_multiscalar_mul(fb.scalar_rows(c, a[:h]), ck, offset=h))      # <a_L, ck_R>
    Rp = as_point(g.vartime_multiscalar_mul(fb.scalar_rows(c, a[h:]), ck, offset=0))      # <a_R, ck_L>
    rhs = R.add(c, as_point(ce.commit(ck, fb.scalar_rows(c, a))), R.add(c, R.mul(c, r * r % c.r, Lp), R.mul(c, ri * ri % c.r, Rp)))
    assert lhs == rhs and lhs is not R.INF
    folded.close()
    ck.close()


@pytest.mark.parametrize("k", [1, 4, 9])
@pytest.mark.parametrize("c", TWO, ids=TWO_IDS)
def test_fold_to_one(nmx, c, k):
    """folding a 2^k-point key k times with (r_i^-1, r_i) leaves one point equal to commit(ck, s) for the tensor vector s of ipa_pc.rs:335-349"""
    rng = random.Random(k + 10 * c.cid)
    n = 1 << k
    x = [rng.randrange(1, c.r) for _ in range(n)]
    ck = source(nmx, c, x, precompute=True)
    rs = [rng.randrange(2, c.r) for _ in range(k)]
    cur = ck
    for r in rs:
        nxt = cur.fold(w32(c, pow(r, -1, c.r)), w32(c, r))
        if cur is not ck:
            cur.close()
        cur = nxt
    assert len(cur) == 1
    sv = kx.tensor_vector(c, rs)
    com = nmx.CommitmentEngine(c.cid).commit(ck, fb.scalar_rows(c, sv))
    assert cur.read(0, 1).tobytes() == com.xy and not com.is_inf
    assert as_point(com) == R.mul(c, sum(a * b for a, b in zip(sv, x)) % c.r, G(c))
    cur.close()
    ck.close()


def test_refusals_that_need_a_key(nmx, sharded):
    from nova_amd import _lib
    L = _lib.lib()
    c = R.BN254_G1
    src = source(nmx, c, list(range(1, 11)))
    other = source(nmx, R.PALLAS, [1, 2, 3])
    one, big = w32(c, 1), np.frombuffer(int(c.r).to_bytes(32, "little"), np.uint8).copy()
    h = ctypes.c_uint64(12345)
    u64s, szs = lambda *v: (ctypes.c_uint64 * len(v))(*v), lambda *v: (ctypes.c_size_t * len(v))(*v)  # noqa: E731
    E, H = _lib.E_ARG, _lib.E_HANDLE
    # a range that leaves its key
    assert L.nmx_bases_fold(src.handle, 0, 11, one.ctypes.data, one.ctypes.data, 0, ctypes.byref(h)) == H
    assert L.nmx_bases_fold(src.handle, 9, 2, one.ctypes.data, one.ctypes.data, 0, ctypes.byref(h)) == H
    assert L.nmx_bases_fold(src.handle, (1 << 64) - 1, 2, one.ctypes.data, one.ctypes.data, 0, ctypes.byref(h)) == H
    assert L.nmx_bases_scale(src.handle, 10, 1, one.ctypes.data, 0, ctypes.byref(h)) == H
    assert L.nmx_bases_concat(u64s(src.handle), szs(4), szs(7), 1, 0, ctypes.byref(h)) == H
    assert L.nmx_bases_concat(u64s(src.handle), szs(11), None, 1, 0, ctypes.byref(h)) == H
    assert L.nmx_bases_concat(u64s(src.handle, src.handle + 1000), None, None, 2, 0, ctypes.byref(h)) == H
    # a key whole from its very end is empty: a zero total length
    assert L.nmx_bases_concat(u64s(src.handle), szs(10), None, 1, 0, ctypes.byref(h)) == E
    # a weight that is not below the key's r; r itself in Montgomery form is still r
    assert L.nmx_bases_scale(src.handle, 0, 10, big.ctypes.data, 0, ctypes.byref(h)) == _lib.E_SCALAR_RANGE
    assert L.nmx_bases_fold(src.handle, 0, 10, one.ctypes.data, big.ctypes.data, _lib.SCALARS_MONT, ctypes.byref(h)) == _lib.E_SCALAR_RANGE
    # two curves
    assert L.nmx_bases_concat(u64s(src.handle, other.handle), None, None, 2, 0, ctypes.byref(h)) == E
    assert h.value == 12345
    # offsets inside the key work, and the handle is the next in sequence: the refused calls registered nothing
    assert L.nmx_bases_fold(src.handle, 2, 7, one.ctypes.data, one.ctypes.data, 0, ctypes.byref(h)) == 0, L.nmx_last_error().decode()
    assert h.value == other.handle + 1
    f = nmx.CommitmentKey(c.cid, h.value, 3, bytes(64))
    assert np.array_equal(f.read(0, 3), kx.rows(c, [3 + 6, 4 + 7, 5 + 8]))
    f.close()
    assert L.nmx_bases_concat(u64s(src.handle, src.handle), szs(8, 0), None, 2, 0, ctypes.byref(h)) == 0, L.nmx_last_error().decode()
    f = nmx.CommitmentKey(c.cid, h.value, 12, bytes(64))
    assert np.array_equal(f.read(0, 12), kx.rows(c, [9, 10] + list(range(1, 11))))
    f.close()
    # a source sharded over two logical devices
    sharded(2)
    big_key = source(nmx, c, list(range(1, 301)))
    assert len(big_key.shard_plan()) == 2
    h = ctypes.c_uint64(12345)
    assert L.nmx_bases_fold(big_key.handle, 0, 300, one.ctypes.data, one.ctypes.data, 0, ctypes.byref(h)) == E
    assert L.nmx_bases_scale(big_key.handle, 0, 300, one.ctypes.data, 0, ctypes.byref(h)) == E
    assert L.nmx_bases_concat(u64s(src.handle, big_key.handle), None, None, 2, 0, ctypes.byref(h)) == E
    assert h.value == 12345
    # a small key made now stays whole and folds as before
    small = source(nmx, c, [1, 2, 3, 4])
    check_fold(nmx, c, small, [1, 2, 3, 4], 5, 6).close()
    for k in (small, big_key, other, src):
        k.close()
