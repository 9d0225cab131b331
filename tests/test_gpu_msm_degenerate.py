"""-m gpu: the MSM on rank-one keys and digit-edge scalars (tests/msm_degenerate_common.py) in every pipeline form, exact bytes against the
closed form (sum_i sign_i s_i mod r) P.

What the CPU emulation cannot run is aimed at here: the four-lane additions of curve_quad.hpp (quad_add / quad_madd / quad_dbl), whose
P == +-Q case leaves the lane-parallel formula for a vote, a gather, the single-lane formula and a pick.  They run the folds (FoldRawQuadFn,
k_big_all), the small-MSM block path (k_small_accum / k_small_combine), the pair tree, the bit-sliced reduction and the quad final pass.  On a
rank-one key every operand of every one of those additions is a multiple of one point, and the scalar families make them equal (cyc, heavy:
doublings), opposite (cyc_cancel, heavy+-: cancellations) or the identity (mixed key, empty buckets) by construction -- see the module
docstring of tests/msm_degenerate_common.py for the stage each family is aimed at.  The digit-edge scalars run under every window width through
the partition's digit loops (compile-time widths 8 / 15 / 16, run-time otherwise), DigitsFn (no_partition, and the shapes the partition does
not take) and the small-scalar entry points."""
import numpy as np
import pytest

from oracle import cref
from oracle import pyref as R
from tests import msm_degenerate_common as D
from tests import util
from tests.test_gpu_fixed_base import sharded  # noqa: F401  (k logical devices on the one GPU; restores init_devices(1) and shard_min_n)
from tests.test_gpu_pipeline_variants import DEFAULTS, VARIANTS

pytestmark = pytest.mark.gpu
KEYS = {"plus": D.signs_plus, "alt": D.signs_alt, "mixed": D.signs_mixed}


def pt(com):
    return (com.xy, int(com.is_inf))


def lib():
    from nova_amd import _lib
    return _lib.lib()


class RankOne:
    """plus / alt / mixed keys of n rows with the scalar vectors of one test and their closed forms, computed once"""

    def __init__(self, nmx, c, n, vectors, precompute=True, keys=("plus", "alt", "mixed")):
        self.c, self.n = c, n
        self.signs = {k: KEYS[k](n) for k in keys}
        self.keys = {k: nmx.CommitmentKey.from_host(c.cid, D.rank_one_key(c, n, s), precompute=precompute) for k, s in self.signs.items()}
        self.rows = {name: D.rows32(s) for name, s in vectors.items()}
        self.want = {(name, k): D.expect(c, s, self.signs[k]) for name, s in vectors.items() for k in keys}

    def check(self, g, tag):
        for (name, k), want in self.want.items():
            assert pt(g.vartime_multiscalar_mul(self.rows[name], self.keys[k])) == want, (tag, name, k)

    def close(self):
        for k in self.keys.values():
            k.close()


class Edges:
    """the digit-edge set of the given widths as vectors of n scalars over multiples_key, with their closed forms"""

    def __init__(self, nmx, c, n, widths, precompute=True):
        self.key = nmx.CommitmentKey.from_host(c.cid, D.multiples_key(c, n), precompute=precompute)
        self.vecs = D.chunks(D.digit_edges_for(widths, c), n)
        self.rows = [D.rows32(s) for s in self.vecs]
        self.want = [D.expect(c, s, D.multiples_coeffs(n)) for s in self.vecs]

    def check(self, g, tag):
        for j, (rows, want) in enumerate(zip(self.rows, self.want)):
            assert pt(g.vartime_multiscalar_mul(rows, self.key)) == want, (tag, "digit edges", j)

    def close(self):
        self.key.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. every pipeline variant
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,n", [(R.BN254_G1, 20000), (R.PALLAS, 1 << 14)], ids=lambda v: getattr(v, "name", v))
def test_every_variant_on_rank_one_keys(nmx, c, n):
    """The VARIANTS of tests/test_gpu_pipeline_variants.py (partition / sort, tasks / segments with few long or many one-entry pieces, every
    big-bucket slice size, fused and per-level trees, single-lane and quad final pass) over registered keys with window tables (c = 15 for
    the 20000-row BN254 key, c = 16 for the 2^14-row Pallas key): cyc(7) fills 128 buckets with 156 P each (BN254; 128 P on Pallas) and
    leaves all others empty, cyc_cancel(7) is the same over the alternating key, heavy sends all n points of each of the 17 / 16 windows
    into one bucket each (every segment piece, slice and fold input equal), heavy+- cancels pairwise inside every piece, and the mixed key
    puts identity rows between them.  The digit-edge set of the widths 14 .. 16 runs over the multiples key."""
    L = lib()
    g = nmx.DlogGroup(c.cid)
    tw = D.table_width(n, c.r.bit_length())
    assert tw == (15 if c is R.BN254_G1 else 16)
    ro = RankOne(nmx, c, n, {"cyc(7)": D.cyc(n, 7), "heavy": D.heavy(c, n)})
    ed = Edges(nmx, c, n, (tw - 1, tw, tw + 1) if tw < 16 else (tw - 2, tw - 1, tw))
    assert ro.want[("cyc(7)", "alt")][1] == 0 and ro.want[("heavy", "alt")] == (bytes(64), 1)      # -a 2^6 P; n even: the identity
    try:
        for var in VARIANTS:
            for k, v in {**DEFAULTS, **var}.items():
                assert L.nmx_set_option(k.encode(), v) == 0
            ro.check(g, var)
            ed.check(g, var)
    finally:
        for k, v in DEFAULTS.items():
            L.nmx_set_option(k.encode(), v)
    ro.close()
    ed.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the small-MSM block path and the task path
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [17, 200, 5000, 13058])
def test_small_msm_block_path_on_rank_one_keys(nmx, n):
    """MSMs with at most 1024 buckets (c = 8 tables of keys below 2^14 points; plain keys of a few hundred pairs) sum their buckets in
    k_small_accum / k_small_combine: option small_blocks = entries per four-lane group (1: many partials per bucket, 64: one block per
    bucket), 0 = the task path.  heavy puts everything into one bucket per window, so all of a bucket's partials are equal (n odd at 17:
    one shorter piece) and k_small_combine's quad tree doubles; heavy+- makes them identities or single points; cyc fills 2^k buckets
    equally.  Keys with tables and plain keys (precompute=False), whose width follows n: cyc's k is 7 on the tables and
    min(7, c - 1) on the plain key.  The digit-edge set of the widths those keys can get runs in vectors of n scalars."""
    L = lib()
    c = R.BN254_G1
    g = nmx.DlogGroup(c.cid)
    bits = c.r.bit_length()
    pw = D.plain_width(n, bits)
    sets = []
    for pre, k in ((True, 7), (False, min(7, pw - 1))):
        sets.append(RankOne(nmx, c, n, {f"cyc({k})": D.cyc(n, k), "heavy": D.heavy(c, n)}, precompute=pre))
        sets.append(Edges(nmx, c, n, (8,) if pre else sorted({3, pw - 1, pw, pw + 1} - {2}), precompute=pre))
    try:
        for sb in (0, 1, 8, 64):
            assert L.nmx_set_option(b"small_blocks", sb) == 0
            for s in sets:
                s.check(g, ("small_blocks", sb))
    finally:
        assert L.nmx_set_option(b"small_blocks", 8) == 0
    for s in sets:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the two forms of the bucket reduction, finished on the device and on the host
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lg,width", [(10, 0), (14, 0), (13, 17), (14, 20)], ids=["2p10_c8", "2p14_c15", "2p13_c17", "2p14_c20"])
def test_reduction_forms_on_a_tree_that_only_doubles(nmx, lg, width):
    """reduce_form 1 (pair tree) and 2 (bit-sliced sums: one-step launches with BsStepQuadFn and the strided view at c = 20, then
    k_reduce_bitsliced) x host_combine 1 (device) and 2 (host_point4.hpp combine_slices) at 128 buckets (one launch), 2^14, 2^16 and 2^19
    buckets.  cyc(k) with k = min(c - 1, lg): at c = 8 and c = 15 that is k = c - 1 -- EVERY bucket holds the same multiple (8 P, P), every
    D / N / O addition of the whole tree adds two equal points; at c = 17 / 20 over 2^13 / 2^14 rows no key this size can fill the bucket
    set, so the first 2^lg buckets hold P each and the tree doubles through its first lg levels and adds identities above.
    cyc_cancel(k) makes every level-0 pair opposite; heavy reduces one non-empty bucket per window among identities."""
    L = lib()
    c = R.BN254_G1
    n = 1 << lg
    cw = width or D.table_width(n, c.r.bit_length())
    assert cw == (width or (8 if lg == 10 else 15))
    k = min(cw - 1, lg)
    g = nmx.DlogGroup(c.cid)
    assert L.nmx_set_window_bits(width) == 0
    try:
        ro = RankOne(nmx, c, n, {f"cyc({k})": D.cyc(n, k), "heavy": D.heavy(c, n)})
        try:
            for form in (1, 2):
                for hc in (1, 2):
                    assert L.nmx_set_option(b"reduce_form", form) == 0 and L.nmx_set_option(b"host_combine", hc) == 0
                    ro.check(g, ("reduce_form", form, "host_combine", hc))
        finally:
            assert L.nmx_set_option(b"reduce_form", 0) == 0 and L.nmx_set_option(b"host_combine", 0) == 0
        ro.close()
    finally:
        assert L.nmx_set_window_bits(0) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. digit edges under every window width
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", list(R.CURVES.values()), ids=lambda c: c.name)
@pytest.mark.parametrize("width", [3, 7, 8, 13, 15, 16, 17, 20])
def test_digit_edges_under_every_window_width(nmx, width, c):
    """nmx_set_window_bits(width), then a plain key (the width is the call's) and a key with tables (the width is the tables'), 4096 rows:
    the digit-edge set of that width over the multiples key against the closed form and over distinct points against the oracle, with
    canonical and Montgomery scalars, and once under no_partition = 1 (DigitsFn; at width 3 the tables' 85 windows do not fit the
    partition's stage, so that path runs DigitsFn anyway).  Then the u64 edges at the declared widths 1, c - 1, c, c + 1, 63, 64 through
    vartime_multiscalar_mul_small_with_max_num_bits and the batch form (a full vector, a short one and an empty one)."""
    L = lib()
    n = 4096
    g = nmx.DlogGroup(c.cid)
    vals = D.tile(D.digit_edges(width, c), n)
    rows, coeffs = D.rows32(vals), D.multiples_coeffs(n)
    want = D.expect(c, vals, coeffs)
    mont = util.to_mont_scalars(c.cid, rows)
    distinct = cref.sequential_bases(c, 300 + width, n)
    want_distinct = cref.msm(c.cid, rows, distinct, n)
    assert L.nmx_set_window_bits(width) == 0
    try:
        keys = [nmx.CommitmentKey.from_host(c.cid, D.multiples_key(c, n), precompute=pre) for pre in (False, True)]
        dkeys = [nmx.CommitmentKey.from_host(c.cid, distinct, precompute=pre) for pre in (False, True)]
        for pre, ck, dk in zip((False, True), keys, dkeys):
            assert pt(g.vartime_multiscalar_mul(rows, ck)) == want, ("canonical", pre)
            assert pt(g.vartime_multiscalar_mul(mont, ck, mont=True)) == want, ("Montgomery", pre)
            assert pt(g.vartime_multiscalar_mul(rows, dk)) == want_distinct, ("distinct points", pre)
            assert L.nmx_set_option(b"no_partition", 1) == 0
            try:
                assert pt(g.vartime_multiscalar_mul(rows, ck)) == want, ("no_partition", pre)
                assert pt(g.vartime_multiscalar_mul(rows, dk)) == want_distinct, ("no_partition, distinct points", pre)
            finally:
                assert L.nmx_set_option(b"no_partition", 0) == 0
            for b in D.u64_widths(width):
                s = D.tile(D.u64_edges(width, b), n)
                s64 = np.array(s, np.uint64)
                w64 = D.expect(c, s, coeffs)
                assert pt(g.vartime_multiscalar_mul_small_with_max_num_bits(s64, ck, b)) == w64, ("u64", b, pre)
                got = g.batch_vartime_multiscalar_mul_small([s64, s64[:37], s64[:0]], ck, max_num_bits=b)
                assert [pt(x) for x in got] == [w64, D.expect(c, s[:37], coeffs[:37]), (bytes(64), 1)], ("u64 batch", b, pre)
        for ck in keys + dkeys:
            ck.close()
    finally:
        assert L.nmx_set_window_bits(0) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. the other entry points that add points
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", list(R.CURVES.values()), ids=lambda c: c.name)
def test_point_sum_of_equal_opposite_and_identity_partials(nmx, c):
    """nmx_point_sum (the combine of sharded and split calls): A + A, A + (-A), O + A + O and eight copies of A, A = 5 P"""
    g = nmx.DlogGroup(c.cid)
    A = R.mul(c, 5, D.base_point(c))
    pa = util.affine_to_partial(c.p, R.point_to_xy64(A), False)
    pm = util.affine_to_partial(c.p, R.point_to_xy64(R.neg(c, A)), False)
    po = util.affine_to_partial(c.p, bytes(64), True)
    assert pt(g.point_sum([pa, pa])) == (R.point_to_xy64(R.mul(c, 2, A)), 0)
    assert pt(g.point_sum([pa, pm])) == (bytes(64), 1)
    assert pt(g.point_sum([po, pa, po])) == (R.point_to_xy64(A), 0)
    assert pt(g.point_sum([pa] * 8)) == (R.point_to_xy64(R.mul(c, 8, A)), 0)
    assert pt(g.point_sum([pm, pa, pa, pm, po, pa])) == (R.point_to_xy64(A), 0)


@pytest.mark.parametrize("c", [R.BN254_G1, R.VESTA], ids=lambda c: c.name)
def test_commit_whose_blinding_term_equals_or_cancels_the_msm(nmx, c):
    """commit = msm(v, ck) + h r over a rank-one key with h = P: r = sum_i s_i makes the two terms equal (the final addition doubles),
    r = -sum_i s_i opposite (the commitment is the identity)."""
    n = 4096
    P = D.base_point(c)
    ck = nmx.CommitmentKey.from_host(c.cid, D.rank_one_key(c, n, D.signs_plus(n)), R.point_to_xy64(P))
    ce = nmx.CommitmentEngine(c.cid)
    for s in (D.cyc(n, 7), D.heavy(c, n)):
        t = sum(s) % c.r
        assert t != 0
        v = D.rows32(s)
        assert pt(ce.commit(ck, v, D.rows32([t])[0])) == (R.point_to_xy64(R.mul(c, 2 * t % c.r, P)), 0)
        assert pt(ce.commit(ck, v, D.rows32([c.r - t])[0])) == (bytes(64), 1)
        assert pt(ce.commit(ck, v)) == D.expect(c, s, D.signs_plus(n))
    ck.close()


@pytest.mark.parametrize("k", [1, 2, 300, 5000])
def test_sparse_commitments_with_every_index_the_same_row(nmx, k):
    """commit_sparse_binary / commit_sparse with k copies of one index: k copies of one base of an ORDINARY key (rows (11 + i) G) -- the gathered
    MSM sees a rank-one key although the registered one is not.  Row 5 is the identity row."""
    c = R.BN254_G1
    n_key = 1024
    host = cref.sequential_bases(c, 11, n_key).copy()
    host[5] = 0
    ck = nmx.CommitmentKey.from_host(c.cid, host)
    ce = nmx.CommitmentEngine(c.cid)
    G = (c.gx, c.gy)
    s = D.tile(D.digit_edges(8, c), k)

    def at(t):
        p = R.mul(c, t % c.r, G)
        return (R.point_to_xy64(p), 1 if p is R.INF else 0)
    for row in (0, 700, 1023):
        idx = np.full(k, row, np.uint64)
        assert pt(ce.commit_sparse_binary(ck, idx)) == at(k * (11 + row)), row
        assert pt(ce.commit_sparse(ck, idx, D.rows32(s))) == at(sum(s) * (11 + row)), row
        assert pt(ce.commit_sparse(ck, idx, D.rows32([3, c.r - 3] * (k // 2) + [0] * (k % 2)))) == (bytes(64), 1), row   # s, -s on one base
    idx = np.full(k, 5, np.uint64)
    assert pt(ce.commit_sparse_binary(ck, idx)) == (bytes(64), 1)
    assert pt(ce.commit_sparse(ck, idx, D.rows32(s))) == (bytes(64), 1)
    ck.close()


def test_fused_batch_over_one_rank_one_key(nmx):
    """batch_vartime_multiscalar_mul of [cyc, cyc_cancel, heavy on the +P rows, heavy+-, empty] over ONE key with tables: the alternating key,
    where cyc lives on the even (+P) rows alone (1 + (i / 2 mod 2^7) there, 0 on the odd rows) and cyc_cancel is cyc(7) itself.  Fused
    (no_batch_fuse = 0: one pipeline run, a bucket set per vector, STAT_FUSED_RUNS moves) and vector by vector (1)."""
    from nova_amd import _lib
    L = _lib.lib()
    c = R.BN254_G1
    n = 4096
    signs = D.signs_alt(n)
    ck = nmx.CommitmentKey.from_host(c.cid, D.rank_one_key(c, n, signs))
    g = nmx.DlogGroup(c.cid)
    half = D.cyc(n // 2, 7)
    h = D.heavy_scalar(c)
    vecs = [[half[i // 2] if i % 2 == 0 else 0 for i in range(n)], D.cyc(n, 7), [h if i % 2 == 0 else 0 for i in range(n)], D.heavy(c, n - 1), []]
    rows = [D.rows32(v) if v else np.zeros((0, 32), np.uint8) for v in vecs]
    want = [D.expect(c, v, signs[:len(v)]) for v in vecs]
    assert want[4] == (bytes(64), 1) and want[3][1] == 0 and want[0] == D.expect(c, half, D.signs_plus(n // 2))
    try:
        for nofuse in (0, 1):
            assert L.nmx_set_option(b"no_batch_fuse", nofuse) == 0
            before = _lib.stats()[_lib.STAT_FUSED_RUNS]
            assert [pt(x) for x in g.batch_vartime_multiscalar_mul(rows, ck)] == want, nofuse
            assert (_lib.stats()[_lib.STAT_FUSED_RUNS] > before) == (nofuse == 0)
    finally:
        assert L.nmx_set_option(b"no_batch_fuse", 0) == 0
    ck.close()


def test_sharded_key_whose_two_partials_are_equal(nmx, sharded):  # noqa: F811
    """A key of 4096 all-+P rows sharded over k = 2 logical devices, the same 2048 scalars against both halves: the two shard partials are
    the same point, so the host's sum of them is a doubling; with the scalars negated on the second half the partials are opposite and the
    sum is the identity; heavy makes every bucket of both shards equal as well."""
    c = R.BN254_G1
    n = 4096
    sharded(2)
    ck = nmx.CommitmentKey.from_host(c.cid, D.rank_one_key(c, n, D.signs_plus(n)))
    assert [p[2] for p in ck.shard_plan()] == [n // 2, n // 2]
    g = nmx.DlogGroup(c.cid)
    first = D.as_ints(util.random_scalars(c.cid, n // 2, seed=2024))
    for s in (first + first, first + [(c.r - v) % c.r for v in first], D.heavy(c, n)):
        assert pt(g.vartime_multiscalar_mul(D.rows32(s), ck)) == D.expect(c, s, D.signs_plus(n))
    t = sum(first) % c.r
    assert t != 0 and D.expect(c, first + first, D.signs_plus(n)) == (R.point_to_xy64(R.mul(c, 2 * t % c.r, D.base_point(c))), 0)
    ck.close()
