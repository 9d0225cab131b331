"""CPU-side check of the bit-sliced bucket reduction (nova_amd/csrc/reduce_bitsliced.hpp, no GPU):

    sum_k (k + 1) B_k  =  root + sum_l 2^l O_l ,   O_l = the sum of the odd nodes of level l of the plain pair-sum tree.

tests/cpp/reduce_bitsliced_test.cpp runs the device's launch plan, its one-step functor and the body of its fused kernel with
XYZZ::add / dbl_in_place on the host (one fiber per four-lane group, real barriers, LDS bounds checked) and is compared with the
oracle's MSM over the scalars k + 1.  Plans: the product's two (128 / 64 additions in a block's first level), and small limits that
force one-step launches with views and several fused launches at these tiny shapes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import cref
from oracle import pyref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "reduce_bitsliced_test.cpp")
SO = os.path.join(HERE, "cpp", "libreduce_bitsliced_test.so")
CSRC = os.path.join(os.path.dirname(HERE), "nova_amd", "csrc")
PLANS = [(128, 32768), (64, 16384), (8, 24), (4, 2), (16, 100)]   # (additions in a block's first level, one-step launches above)
MS = [1, 2, 4, 128, 1 << 10]
CURVES = [R.BN254_G1, R.PALLAS]


@pytest.fixture(scope="module")
def helper():
    deps = [SRC, os.path.join(HERE, "host_emul", "simt.hpp")] + [os.path.join(CSRC, f) for f in ("fp.hpp", "curve.hpp", "curves.hpp", "reduce_bitsliced.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    L.bs_reduce.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return L


_POINTS = {}


def points(c):
    """2^10 x 4 points of the curve, computed once and never modified (tests take copies)."""
    if c.cid not in _POINTS:
        p = cref.sequential_bases(c, 90001, 4 << 10)
        p.setflags(write=False)
        _POINTS[c.cid] = p
    return _POINTS[c.cid]


def negate(c, pts):
    out = pts.copy()
    for i in range(len(out)):
        y = int.from_bytes(out[i, 32:].tobytes(), "little")
        out[i, 32:] = np.frombuffer(((c.p - y) % c.p).to_bytes(32, "little"), np.uint8)
    return out


def bucket_sets(c, M, WB, kind):
    """WB sets of M buckets each, as an (WB * M, 64) array."""
    n = WB * M
    pts = points(c)[:n].copy()
    if kind == "identity":
        pts[:] = 0
    elif kind == "one":
        keep = pts[n // 2].copy()
        pts[:] = 0
        pts[(n // 2) | (M - 1)] = keep           # the last bucket of a set: every bit of its index is set
    elif kind == "equal_pairs" and M >= 2:        # B_2j = B_2j+1: P == Q in step 0
        pts[1::2] = pts[0::2]
    elif kind == "cancelling_pairs" and M >= 2:   # B_2j = -B_2j+1: P == -Q in step 0
        pts[1::2] = negate(c, pts[0::2])
    elif kind == "sparse":                        # identities among the operands of every level
        pts[np.arange(n) % 3 != 0] = 0
    return pts


def expected(c, pts, M, WB):
    w = np.arange(1, M + 1, dtype=np.uint64)
    return [cref.msm_u64(c.cid, w, pts[s * M:(s + 1) * M], M) for s in range(WB)]


def reduce(L, c, pts, M, WB, cap, wide_above):
    b = np.ascontiguousarray(pts)
    out = np.zeros(64 * WB, np.uint8)
    inf = np.zeros(WB, np.uint8)
    desc = np.zeros(3 * 40, np.uint32)
    rc = L.bs_reduce(c.cid, b.ctypes.data, M, WB, cap, wide_above, out.ctypes.data, inf.ctypes.data, desc.ctypes.data)
    return rc, [(out[64 * s:64 * s + 64].tobytes(), int(inf[s])) for s in range(WB)], desc.reshape(40, 3)[:max(rc, 0)]


@pytest.mark.parametrize("kind", ["random", "identity", "one", "equal_pairs", "cancelling_pairs", "sparse"])
@pytest.mark.parametrize("WB", [1, 4])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_bitsliced_sums_equal_the_weighted_sum(helper, c, WB, kind):
    for M in MS:
        pts = bucket_sets(c, M, WB, kind)
        exp = expected(c, pts, M, WB)
        if M == 1:  # no level, no O_l: the bucket is the sum, and the device keeps the pair tree's path (which returns it)
            assert reduce(helper, c, pts, M, WB, 128, 32768)[0] == -1
            assert [(bytes(pts[s].tobytes()), int(not pts[s].any())) for s in range(WB)] == exp
            continue
        for cap, wide_above in PLANS:
            rc, got, desc = reduce(helper, c, pts, M, WB, cap, wide_above)
            assert rc > 0, (M, cap, wide_above, rc)
            assert got == exp, (M, cap, wide_above, desc.tolist())


def test_plans_cover_the_launch_kinds(helper):
    """The forced plans really run what they are there for: one-step launches (the second one reads a view), a fused launch right
    behind one (view input), several fused launches in a row, more than one block, and the product's plan at 128 buckets is the
    single fused launch."""
    c = R.BN254_G1
    pts = bucket_sets(c, 1 << 10, 1, "random")
    rc, _, d = reduce(helper, c, pts, 1 << 10, 1, 8, 24)
    kinds = d[:, 0].tolist()
    assert kinds[:2] == [1, 1] and 0 in kinds and kinds[-1] == 0
    first_fused = kinds.index(0)
    assert kinds[first_fused - 1] == 1 and d[first_fused, 2] > 1          # view input, many blocks
    assert int(d[:, 1].sum()) == 10                                      # every level exactly once
    rc, _, d = reduce(helper, c, pts, 1 << 10, 1, 16, 100)
    assert d[:, 0].tolist().count(0) >= 3 and int(d[:, 1].sum()) == 10   # fused launches chained through memory
    rc, _, d = reduce(helper, c, pts, 1 << 10, 1, 128, 32768)
    assert d.tolist() == [[0, 8, 4], [0, 2, 1]]                          # eight levels in four blocks, then the last block
    rc, _, d = reduce(helper, c, bucket_sets(c, 128, 1, "random"), 128, 1, 128, 32768)
    assert rc == 1 and d.tolist() == [[0, 7, 1]]
    rc, _, d = reduce(helper, c, bucket_sets(c, 128, 4, "random"), 128, 4, 128, 32768)
    assert rc == 1 and d.tolist() == [[0, 7, 4]]                         # the last launch: one block per bucket set
