"""CPU-side check of the bit-sliced bucket reduction that ends in slices, and of the host combine behind it (no GPU):

    sum_k (k + 1) B_k  =  root + sum_l 2^l O_l ,   the last launch leaves root and O_0 .. O_(L-1), combine_slices adds them up.

tests/cpp/reduce_slices_test.cpp runs the device's launch plan, its one-step functor and the body of its fused kernel with
BsTreeArgs::slices = 1 on the host (a policy of its own: one fiber per four-lane group, real barriers, LDS and output bounds checked),
checks that the error word lands behind the last slice and nothing beyond it is written, and runs combine_slices
(nova_amd/csrc/host_point4.hpp) per bucket set.  Compared with the oracle's MSM over the scalars k + 1, for the plans, shapes and
bucket kinds of tests/test_reduce_bitsliced.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.test_reduce_bitsliced import CURVES, PLANS, bucket_sets, expected

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "reduce_slices_test.cpp")
SO = os.path.join(HERE, "cpp", "libreduce_slices_test.so")
CSRC = os.path.join(os.path.dirname(HERE), "nova_amd", "csrc")
MS = [2, 4, 128, 1 << 10]


@pytest.fixture(scope="module")
def helper():
    deps = [SRC, os.path.join(HERE, "host_emul", "simt.hpp")] + [
        os.path.join(CSRC, f) for f in ("fp.hpp", "curve.hpp", "curves.hpp", "reduce_bitsliced.hpp", "host_fp4.hpp", "host_point4.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    L.bs_reduce_slices.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                   ctypes.c_void_p, ctypes.c_void_p]
    return L


def reduce(L, c, pts, M, WB, cap, wide_above):
    b = np.ascontiguousarray(pts)
    out = np.zeros(64 * WB, np.uint8)
    inf = np.zeros(WB, np.uint8)
    rc = L.bs_reduce_slices(c.cid, b.ctypes.data, M, WB, cap, wide_above, out.ctypes.data, inf.ctypes.data)
    return rc, [(out[64 * s:64 * s + 64].tobytes(), int(inf[s])) for s in range(WB)]


@pytest.mark.parametrize("kind", ["random", "identity", "one", "equal_pairs", "cancelling_pairs", "sparse"])
@pytest.mark.parametrize("WB", [1, 4])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_slices_and_host_combine_equal_the_weighted_sum(helper, c, WB, kind):
    for M in MS:
        pts = bucket_sets(c, M, WB, kind)
        exp = expected(c, pts, M, WB)
        for cap, wide_above in PLANS:
            rc, got = reduce(helper, c, pts, M, WB, cap, wide_above)
            assert rc > 0, (M, cap, wide_above, rc)   # -3: the error word is not behind the last slice, -4: a write beyond it
            assert got == exp, (M, cap, wide_above)
