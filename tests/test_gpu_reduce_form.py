"""-m gpu: the two forms of the bucket reduction compute the same, oracle-exact result.  Option reduce_form: 1 = the (D, Y) pair
tree (ReducePairFn / k_reduce_tree), 2 = bit-sliced sums (reduce_bitsliced.hpp: one-step launches + k_reduce_bitsliced),
0 = chosen by bucket count.  Shapes: 128 buckets (one fused launch), 2^14 and 2^15 buckets (several fused
launches), a fused batch (four bucket sets side by side), window widths 17 and 20 forced on small keys (one-step launches with one
lane and with four lanes per addition, the strided view behind them), keys with identity points and without (the clean flag),
and scalars that cancel pairwise on repeated bases (P == -Q and P == Q inside the reduction's additions)."""
import numpy as np
import pytest

from oracle import cref
from oracle import pyref as R
from tests import util

pytestmark = pytest.mark.gpu
FORMS = [1, 2, 0]


def as_pair(com):
    return (com.xy, int(com.is_inf))


def each_form(L, f):
    out = {}
    try:
        for form in FORMS:
            assert L.nmx_set_option(b"reduce_form", form) == 0
            out[form] = f()
    finally:
        assert L.nmx_set_option(b"reduce_form", 0) == 0
    return out


@pytest.mark.parametrize("c,lg", [(R.BN254_G1, 10), (R.PALLAS, 14), (R.BN254_G1, 14), (R.BN254_G1, 17)], ids=lambda v: getattr(v, "name", v))
def test_forms_agree_with_oracle(nmx, c, lg):
    from nova_amd import _lib
    L = _lib.lib()
    n = 1 << lg
    bases = cref.sequential_bases(c, 4100 + lg, n)
    prep = cref.Prepared(c.cid, bases, n)
    ck = nmx.CommitmentKey.from_host(c.cid, bases)
    g = nmx.DlogGroup(c.cid)
    for kind in ("random", "u16", "equal"):
        sc = util.scalar_set(c.cid, n, kind)
        exp = prep.msm(sc, n)
        got = each_form(L, lambda: as_pair(g.vartime_multiscalar_mul(sc, ck)))
        assert all(v == exp for v in got.values()), (kind, [f for f, v in got.items() if v != exp])
    ck.close()
    assert L.nmx_set_option(b"reduce_form", 3) == _lib.E_ARG


@pytest.mark.parametrize("width,lg", [(17, 13), (20, 14)])
def test_forms_agree_at_forced_wide_windows(nmx, width, lg):
    """2^16 and 2^19 buckets over a small key: the steps that take a launch each, then the fused ones."""
    from nova_amd import _lib
    L = _lib.lib()
    c = R.BN254_G1
    n = 1 << lg
    bases = cref.sequential_bases(c, 515 + width, n)
    sc = util.random_scalars(c.cid, n, seed=width)
    exp = cref.msm(c.cid, sc, bases, n)
    assert L.nmx_set_window_bits(width) == 0
    try:
        ck = nmx.CommitmentKey.from_host(c.cid, bases)
        g = nmx.DlogGroup(c.cid)
        got = each_form(L, lambda: as_pair(g.vartime_multiscalar_mul(sc, ck)))
        ck.close()
    finally:
        assert L.nmx_set_window_bits(0) == 0
    assert all(v == exp for v in got.values()), [f for f, v in got.items() if v != exp]


def test_forms_agree_on_a_fused_batch(nmx):
    """Three vectors over a 2^14 key: four bucket sets (the count is rounded up to a power of two) reduced side by side."""
    from nova_amd import _lib
    L = _lib.lib()
    c = R.BN254_G1
    n = 1 << 14
    bases = cref.sequential_bases(c, 9090, n)
    ck = nmx.CommitmentKey.from_host(c.cid, bases)
    g = nmx.DlogGroup(c.cid)
    vecs = [util.random_scalars(c.cid, m, seed=60 + j) for j, m in enumerate((n, n - 5, 9001))]
    exp = [cref.msm(c.cid, v, bases[:len(v)], len(v)) for v in vecs]
    before = _lib.stats()[_lib.STAT_FUSED_RUNS]
    got = each_form(L, lambda: [as_pair(x) for x in g.batch_vartime_multiscalar_mul(vecs, ck)])
    assert _lib.stats()[_lib.STAT_FUSED_RUNS] - before == len(FORMS)   # every form ran the vectors as ONE pipeline run
    assert all(v == exp for v in got.values()), [f for f, v in got.items() if v != exp]
    ck.close()


def test_forms_agree_with_identity_points_and_cancelling_pairs(nmx):
    from nova_amd import _lib
    L = _lib.lib()
    c = R.BN254_G1
    n = 1 << 14
    clean = cref.sequential_bases(c, 777, n)
    dirty = clean.copy()
    dirty[::97] = 0                                            # identity points: the key is not clean
    rep = clean.copy()
    rep[1::2] = rep[0::2]                                      # every base twice
    sc = util.random_scalars(c.cid, n, seed=3)
    r = c.r
    canc = sc.copy()                                           # s, r - s on the same base: every pair cancels, the sum is the identity
    for i in range(0, n, 2):
        s = int.from_bytes(sc[i].tobytes(), "little")
        canc[i + 1] = np.frombuffer(((r - s) % r).to_bytes(32, "little"), np.uint8)
    part = canc.copy()
    part[n // 2:] = sc[n // 2:]                                # half of the pairs cancel
    dbl = sc.copy()
    dbl[1::2] = dbl[0::2]                                      # the same scalar on the same base: equal points meet in the buckets
    g = nmx.DlogGroup(c.cid)
    for key, scalars in ((clean, [sc]), (dirty, [sc]), (rep, [canc, part, dbl])):
        ck = nmx.CommitmentKey.from_host(c.cid, key)
        for s in scalars:
            exp = cref.msm(c.cid, s, key, n)
            got = each_form(L, lambda: as_pair(g.vartime_multiscalar_mul(s, ck)))
            assert all(v == exp for v in got.values()), [f for f, v in got.items() if v != exp]
        ck.close()
    assert cref.msm(c.cid, canc, rep, n) == (bytes(64), 1)


def test_clean_accum_switch_computes_the_same(nmx):
    """Option no_clean_accum, the A/B switch of the clean-key accumulate, on a key without identity points (1 = its rows are tested
    for the identity all the same) and on one with (the switch changes nothing), over the scalar sets that skew the buckets."""
    opt = b"no_clean_accum"
    from nova_amd import _lib
    L = _lib.lib()
    c = R.BN254_G1
    n = 1 << 15
    clean = cref.sequential_bases(c, 2024, n)
    dirty = clean.copy()
    dirty[5::1001] = 0
    g = nmx.DlogGroup(c.cid)
    try:
        for key in (clean, dirty):
            ck = nmx.CommitmentKey.from_host(c.cid, key)
            prep = cref.Prepared(c.cid, key, n)
            for kind in ("random", "equal", "u1", "zero_rm1"):
                sc = util.scalar_set(c.cid, n, kind)
                exp = prep.msm(sc, n)
                for v in (1, 0):
                    assert L.nmx_set_option(opt, v) == 0
                    assert as_pair(g.vartime_multiscalar_mul(sc, ck)) == exp, (kind, v)
            ck.close()
    finally:
        assert L.nmx_set_option(opt, 0) == 0
