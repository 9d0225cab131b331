"""-m gpu: the segment accumulate's progress-keyed wave priority (option accum_prio: 1 = off, 2 = on, 3 = on with the other
schedule; msm_seg.hpp AccumSegFn PRIO) never changes a result.  It only moves s_setprio through the kernel, so every case compares
the affine result byte for byte across priority off / on and across one and two rounds of resident lanes (and a few long segments:
4096 lanes), and against the CPU oracle (oracle.cref.msm).

Shapes, the smallest that reach the segment path on a key with tables (c >= 15; the option seg_min_total = 0 keeps the path on for the
scalar sets with few entries): a 2^14-point key (c = 15) with a full vector and with 2^14 - 37 scalars (the last wave holds shorter
and empty segments), a 2^17-point key (c = 16).  At one and two rounds of resident lanes these segments are seg_min_len = 8 entries
or 11, where the schedule's thresholds coincide or sit one trip apart; at 4096 lanes they are 68 to 512 entries long.
Scalar sets: uniformly random; all equal (one big bucket: waves whose lanes never cross a boundary); 0 / 1 (few entries: segments of
8 and fewer); u16 (many empty buckets: the search inside the loop)."""
import pytest

from oracle import cref
from oracle import pyref as R
from tests import util

pytestmark = pytest.mark.gpu
KINDS = ["random", "equal", "u1", "u16"]
DEFAULTS = {"accum_prio": 0, "seg_lanes": 0, "seg_min_total": 0xFFFFFFFE, "no_clean_accum": 0, "accum_prefetch": 0}


def as_pair(com):
    return (com.xy, int(com.is_inf))


def resident_lanes():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 768  # three 256-thread blocks per CU


def set_options(L, opts):
    for k, v in opts.items():
        assert L.nmx_set_option(k.encode(), v) == 0, k


def runs_agree(L, call, exp, extra, tag):
    """call() under priority off / on x the lane counts, on top of the options in `extra`: all equal to the oracle's `exp`."""
    res = resident_lanes()
    for lanes in (res, 2 * res, 4096):
        for prio in (1, 2):
            set_options(L, {**DEFAULTS, "seg_min_total": 0, **extra, "seg_lanes": lanes, "accum_prio": prio})
            assert call() == exp, (tag, extra, lanes, prio)


@pytest.mark.parametrize("lg,cut", [(14, 0), (14, 37), (17, 0)])
@pytest.mark.parametrize("c", [R.BN254_G1, R.PALLAS], ids=lambda c: c.name)
def test_priority_never_changes_a_result(nmx, c, lg, cut):
    from nova_amd import _lib
    L = _lib.lib()
    n = 1 << lg
    m = n - cut
    bases = cref.sequential_bases(c, 3100 + lg, n)
    ck = nmx.CommitmentKey.from_host(c.cid, bases)
    g = nmx.DlogGroup(c.cid)
    try:
        for kind in KINDS:
            sc = util.scalar_set(c.cid, n, kind)[:m]
            exp = cref.msm(c.cid, sc, bases[:m], m)
            runs_agree(L, lambda: as_pair(g.vartime_multiscalar_mul(sc, ck)), exp, {}, kind)
    finally:
        set_options(L, DEFAULTS)
        ck.close()


@pytest.mark.parametrize("extra", [{"no_clean_accum": 1}, {"accum_prefetch": 2}, {"accum_prefetch": 2, "no_clean_accum": 1}, {"accum_prio": 3}],
                         ids=lambda e: "-".join(f"{k}{v}" for k, v in e.items()))
def test_the_other_instantiations_and_the_other_schedule(nmx, extra):
    """The identity-testing accumulate on a clean key, two gathers in flight, both together -- each with priority off and on -- and the
    equal-quarters schedule (accum_prio 3) on its own."""
    from nova_amd import _lib
    L = _lib.lib()
    c = R.BN254_G1
    n = (1 << 14) - 37
    bases = cref.sequential_bases(c, 3200, 1 << 14)
    ck = nmx.CommitmentKey.from_host(c.cid, bases)
    g = nmx.DlogGroup(c.cid)
    try:
        for kind in ("random", "u16"):
            sc = util.scalar_set(c.cid, n, kind)
            exp = cref.msm(c.cid, sc, bases[:n], n)
            if "accum_prio" in extra:
                for lanes in (resident_lanes(), 4096):
                    set_options(L, {**DEFAULTS, "seg_min_total": 0, "seg_lanes": lanes, **extra})
                    assert as_pair(g.vartime_multiscalar_mul(sc, ck)) == exp, (kind, lanes)
            else:
                runs_agree(L, lambda: as_pair(g.vartime_multiscalar_mul(sc, ck)), exp, extra, kind)
    finally:
        set_options(L, DEFAULTS)
        ck.close()


def test_option_is_ignored_where_the_segment_path_does_not_run(nmx):
    """A key below 2^14 points (c = 8 tables: the small block path) and the same key without tables under the task path: accum_prio = 2
    is accepted and changes nothing; a value outside 0..3 is an argument error."""
    from nova_amd import _lib
    L = _lib.lib()
    c = R.BN254_G1
    n = 5000
    bases = cref.sequential_bases(c, 3300, n)
    sc = util.random_scalars(c.cid, n, seed=33)
    exp = cref.msm(c.cid, sc, bases, n)
    keys = [nmx.CommitmentKey.from_host(c.cid, bases), nmx.CommitmentKey.from_host(c.cid, bases, precompute=False)]
    g = nmx.DlogGroup(c.cid)
    try:
        for small_blocks in (8, 0):
            assert L.nmx_set_option(b"small_blocks", small_blocks) == 0
            for prio in (2, 1, 0):
                assert L.nmx_set_option(b"accum_prio", prio) == 0
                for ck in keys:
                    assert as_pair(g.vartime_multiscalar_mul(sc, ck)) == exp, (small_blocks, prio)
        assert L.nmx_set_option(b"accum_prio", 4) == _lib.E_ARG
    finally:
        assert L.nmx_set_option(b"small_blocks", 8) == 0
        set_options(L, DEFAULTS)
        for ck in keys:
            ck.close()
