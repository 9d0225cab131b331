"""-m gpu: the end of the bit-sliced bucket reduction on the host (option host_combine) computes the same, oracle-exact result.

host_combine 1 = the last launch of the reduction combines root + sum_l 2^l O_l on the device, 2 = it leaves the L + 1 points of every
bucket set, which come over in the call's one copy and are combined on the calling thread (host_point4.hpp combine_slices),
0 = by rule.  Every case runs under host_combine 1 and 2 and reduce_form 0 and 2.  Shapes: 128 buckets (a single launch that is
also the last), 2^14 buckets (several fused launches), window widths 17 and 20 forced on small keys (2^16 buckets: the headline's
plan 8 + 4 + 4, L = 16; 2^19 buckets: one-step launches first, L = 19), a fused batch of three vectors (four sets of slices in one
copy); random, all-equal and 16-bit scalars, scalars that cancel pairwise on repeated bases (the sum is the identity: the host's
Horner meets P == -Q), and a key with identity points."""
import numpy as np
import pytest

from oracle import cref
from oracle import pyref as R
from tests import util

pytestmark = pytest.mark.gpu
SETTINGS = [(hc, form) for hc in (1, 2) for form in (0, 2)]
C = R.BN254_G1


def as_pair(com):
    return (com.xy, int(com.is_inf))


def each_setting(L, f):
    out = {}
    try:
        for hc, form in SETTINGS:
            assert L.nmx_set_option(b"host_combine", hc) == 0
            assert L.nmx_set_option(b"reduce_form", form) == 0
            out[(hc, form)] = f()
    finally:
        assert L.nmx_set_option(b"host_combine", 0) == 0
        assert L.nmx_set_option(b"reduce_form", 0) == 0
    return out


def cancelling(sc, r):
    """s, r - s on consecutive rows: over a key that holds every base twice the sum is the identity."""
    out = sc.copy()
    for i in range(0, len(sc), 2):
        s = int.from_bytes(sc[i].tobytes(), "little")
        out[i + 1] = np.frombuffer(((r - s) % r).to_bytes(32, "little"), np.uint8)
    return out


def check_key(nmx, L, key, scalar_sets):
    n = len(key)
    prep = cref.Prepared(C.cid, key, n)
    ck = nmx.CommitmentKey.from_host(C.cid, key)
    g = nmx.DlogGroup(C.cid)
    try:
        for name, sc in scalar_sets:
            exp = prep.msm(sc, n)
            got = each_setting(L, lambda: as_pair(g.vartime_multiscalar_mul(sc, ck)))
            assert all(v == exp for v in got.values()), (name, [k for k, v in got.items() if v != exp])
            if name == "cancelling":
                assert exp == (bytes(64), 1)
    finally:
        ck.close()
        prep.close()


def scalar_sets(n):
    return [(kind, util.scalar_set(C.cid, n, kind)) for kind in ("random", "equal", "u16")]


def repeated(bases):
    rep = bases.copy()
    rep[1::2] = rep[0::2]
    return rep


@pytest.mark.parametrize("lg,width", [(10, 0), (14, 0), (13, 17), (14, 20)], ids=["2p10_c8", "2p14_c15", "2p13_c17", "2p14_c20"])
def test_host_combine_agrees_with_oracle(nmx, lg, width):
    from nova_amd import _lib
    L = _lib.lib()
    n = 1 << lg
    bases = cref.sequential_bases(C, 7300 + lg + width, n)
    assert L.nmx_set_window_bits(width) == 0
    try:
        check_key(nmx, L, bases, scalar_sets(n))
        check_key(nmx, L, repeated(bases), [("cancelling", cancelling(util.random_scalars(C.cid, n, seed=11), C.r))])
    finally:
        assert L.nmx_set_window_bits(0) == 0


def test_host_combine_on_a_key_with_identity_points(nmx):
    from nova_amd import _lib
    L = _lib.lib()
    n = 1 << 14
    dirty = cref.sequential_bases(C, 4242, n).copy()
    dirty[::97] = 0
    check_key(nmx, L, dirty, [("random", util.random_scalars(C.cid, n, seed=8))])


def test_host_combine_on_a_fused_batch(nmx):
    """Three vectors over a 2^14 key: four bucket sets, four sets of slices in the one copy, each combined into its own sum."""
    from nova_amd import _lib
    L = _lib.lib()
    n = 1 << 14
    bases = cref.sequential_bases(C, 9191, n)
    ck = nmx.CommitmentKey.from_host(C.cid, bases)
    g = nmx.DlogGroup(C.cid)
    vecs = [util.random_scalars(C.cid, m, seed=70 + j) for j, m in enumerate((n, n - 5, 9001))]
    exp = [cref.msm(C.cid, v, bases[:len(v)], len(v)) for v in vecs]
    before = _lib.stats()[_lib.STAT_FUSED_RUNS]
    got = each_setting(L, lambda: [as_pair(x) for x in g.batch_vartime_multiscalar_mul(vecs, ck)])
    assert _lib.stats()[_lib.STAT_FUSED_RUNS] - before == len(SETTINGS)   # every setting ran the vectors as ONE pipeline run
    assert all(v == exp for v in got.values()), [k for k, v in got.items() if v != exp]
    ck.close()


def test_host_combine_rejects_other_values(nmx):
    from nova_amd import _lib
    L = _lib.lib()
    assert L.nmx_set_option(b"host_combine", 3) == _lib.E_ARG
    assert L.nmx_set_option(b"host_combine", 0) == 0
