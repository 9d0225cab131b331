"""-m gpu: level 1 of the bucket partition with per-chunk count rows (option part_rows: 1 = the counting and placing passes with global
atomics, 2 = k_count_rows / k_scan_rows / k_place_rows wherever the shape allows; msm_partition.hpp) never changes a result: only the
order of the entries inside a first-level bin differs, and bucket sums do not depend on it.  Every case runs the same MSM under
part_rows 2 and 1 and compares both affine results byte for byte with the CPU oracle (oracle.cref.msm), hence with each other.

Shapes: a 2^12-point key whose tables are forced to the three widths the rows cover (15, 16, 17: chunks of 704, 768, 768 scalars,
128 or 256 first-level bins) with n = 1, one short of / exactly / one past a 768-scalar chunk and the whole key (six chunks, a ragged
last one); one 2^17-pair MSM at the key's own width (c = 16: 171 chunks, several 32-chunk ranges of the column scan and more chunks
than a range holds before the last one).  Scalar sets: uniformly random, 0 / 1, below 2^10 (a handful of bins), all equal (one bin per
window takes the whole chunk: the uniform-bin path of the LDS rank), 0 / r - 1 (negative digits, carries through every window)."""
import pytest

from oracle import cref
from oracle import pyref as R
from tests import util

pytestmark = pytest.mark.gpu
KINDS = ["random", "u1", "u10", "equal", "zero_rm1"]
SIZES = [1, 767, 768, 769, 1 << 12]
C = R.BN254_G1


def as_pair(com):
    return (com.xy, int(com.is_inf))


@pytest.fixture(scope="module")
def small_cases():
    """The 2^12-point key's bases and, per (n, scalar set), the scalars and the oracle's sum over the first n points: computed once,
    shared by the three widths."""
    n_key = 1 << 12
    bases = cref.sequential_bases(C, 4100, n_key)
    out = {}
    for n in SIZES:
        for kind in KINDS:
            sc = util.scalar_set(C.cid, n_key, kind)[:n]
            out[(n, kind)] = (sc, cref.msm(C.cid, sc, bases[:n], n))
    return bases, out


def both_paths(L, g, sc, ck, exp, tag):
    for rows in (2, 1):
        assert L.nmx_set_option(b"part_rows", rows) == 0
        assert as_pair(g.vartime_multiscalar_mul(sc, ck)) == exp, (tag, "part_rows", rows)


@pytest.mark.parametrize("width", [15, 16, 17])
def test_rows_never_change_a_result(nmx, small_cases, width):
    from nova_amd import _lib
    L = _lib.lib()
    bases, cases = small_cases
    g = nmx.DlogGroup(C.cid)
    assert L.nmx_set_window_bits(width) == 0
    try:
        ck = nmx.CommitmentKey.from_host(C.cid, bases)
        try:
            for (n, kind), (sc, exp) in cases.items():
                both_paths(L, g, sc, ck, exp, (width, n, kind))
        finally:
            ck.close()
    finally:
        assert L.nmx_set_option(b"part_rows", 0) == 0
        assert L.nmx_set_window_bits(0) == 0


def test_rows_at_2p17_pairs(nmx):
    """The key's own width; by rule (0) as well, whichever way the rule decides at this size."""
    from nova_amd import _lib
    L = _lib.lib()
    n = 1 << 17
    bases = cref.sequential_bases(C, 4200, n)
    ck = nmx.CommitmentKey.from_host(C.cid, bases)
    g = nmx.DlogGroup(C.cid)
    try:
        for kind in KINDS:
            sc = util.scalar_set(C.cid, n, kind)
            exp = cref.msm(C.cid, sc, bases, n)
            both_paths(L, g, sc, ck, exp, kind)
            assert L.nmx_set_option(b"part_rows", 0) == 0
            assert as_pair(g.vartime_multiscalar_mul(sc, ck)) == exp, (kind, "part_rows", 0)
    finally:
        assert L.nmx_set_option(b"part_rows", 0) == 0
        ck.close()


def test_rows_on_a_key_with_identity_points_and_on_a_fused_batch(nmx, small_cases):
    """Identity points among the bases (both passes skip the pair) and the bucket sets of a fused batch of two vectors over c = 15 tables
    (keys of 15 bits: still the narrow geometry, 256 bins); a value outside 0..2 is an argument error."""
    from nova_amd import _lib
    L = _lib.lib()
    bases, cases = small_cases
    n = 1 << 12
    holes = bases.copy()
    holes[5::7] = 0
    g, eng = nmx.DlogGroup(C.cid), nmx.CommitmentEngine(C.cid)
    assert L.nmx_set_window_bits(15) == 0
    try:
        ck, hk = nmx.CommitmentKey.from_host(C.cid, bases), nmx.CommitmentKey.from_host(C.cid, holes)
        try:
            for kind in ("random", "equal"):
                sc = cases[(n, kind)][0]
                both_paths(L, g, sc, hk, cref.msm(C.cid, sc, holes, n), ("identity points", kind))
            vs = [cases[(n, "random")][0], cases[(769, "zero_rm1")][0]]
            exp = [cases[(n, "random")][1], cases[(769, "zero_rm1")][1]]
            for rows in (2, 1):
                assert L.nmx_set_option(b"part_rows", rows) == 0
                assert [as_pair(x) for x in eng.batch_commit(ck, vs)] == exp, ("fused batch", rows)
            assert L.nmx_set_option(b"part_rows", 3) == _lib.E_ARG
        finally:
            ck.close()
            hk.close()
    finally:
        assert L.nmx_set_option(b"part_rows", 0) == 0
        assert L.nmx_set_window_bits(0) == 0
