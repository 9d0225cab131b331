"""CPU-side check of the host point arithmetic on 4 x 64-bit limbs (nova_amd/csrc/host_point4.hpp, no GPU).

tests/cpp/host_point4_test.cpp runs HostPoint4's add and double beside XYZZ<FID>::add / dbl_in_place on the same stored points
(representatives scaled by a random lambda, so zz and zzz are not one) and returns both answers as affine bytes; here they are
compared with each other and with the big-int group law, on the base fields of all four curves.  combine_slices -- the host end of
the bit-sliced bucket reduction, root + sum_l 2^l O_l -- is compared with the oracle's MSM over the weights 1, 1, 2, 4, ...
The same source with its own main() is built with -fsanitize=address,undefined and run as a program of its own."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import cref
from oracle import pyref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "host_point4_test.cpp")
SO = os.path.join(HERE, "cpp", "libhost_point4_test.so")
SAN = os.path.join(HERE, "cpp", "host_point4_san.bin")
CSRC = os.path.join(os.path.dirname(HERE), "nova_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("fp.hpp", "curve.hpp", "curves.hpp", "host_fp4.hpp", "host_point4.hpp")]
CURVES = [R.BN254_G1, R.GRUMPKIN, R.PALLAS, R.VESTA]
ZERO = bytes(64)


def stale(target):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(d) for d in DEPS)


@pytest.fixture(scope="module")
def helper():
    if stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    vp = ctypes.c_void_p
    L.hp4_op.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    L.hp4_combine.argtypes = [ctypes.c_int, vp, vp, ctypes.c_uint32, vp, vp]
    return L


_POINTS = {}


def points(c):
    """64 points of the curve, computed once and never modified."""
    if c.cid not in _POINTS:
        p = cref.sequential_bases(c, 31337, 64)
        p.setflags(write=False)
        _POINTS[c.cid] = p
    return _POINTS[c.cid]


def lam(rng, c):
    return rng.randrange(1, c.p).to_bytes(32, "little")


def op(L, c, which, P, lp, Q, lq):
    out = np.zeros(128, np.uint8)
    inf = np.zeros(2, np.uint8)
    bufs = [np.frombuffer(bytes(b), np.uint8).copy() for b in (P, lp, Q, lq)]
    rc = L.hp4_op(c.cid, which, *[b.ctypes.data for b in bufs], out.ctypes.data, inf.ctypes.data)
    assert rc == 0, rc
    return (out[:64].tobytes(), int(inf[0])), (out[64:].tobytes(), int(inf[1]))


def expect(c, P):
    return (R.point_to_xy64(P), int(P is R.INF))


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_add_and_double_match_xyzz_and_the_group_law(helper, c):
    rng = random.Random(400 + c.cid)
    pts = [bytes(points(c)[i].tobytes()) for i in range(12)]
    one = (1).to_bytes(32, "little")
    cases = [(pts[i], pts[i + 1]) for i in range(0, 8, 2)]                 # random points
    cases += [(ZERO, pts[8]), (pts[9], ZERO), (ZERO, ZERO)]                # identity left, right, both
    cases += [(pts[10], pts[10])]                                          # P == Q
    cases += [(pts[11], R.point_to_xy64(R.neg(c, R.xy64_to_point(pts[11]))))]  # P == -Q
    for P, Q in cases:
        for lp, lq in ((lam(rng, c), lam(rng, c)), (one, one), (one, lam(rng, c))):
            host, dev = op(helper, c, 0, P, lp, Q, lq)
            assert host == dev == expect(c, R.add(c, R.xy64_to_point(P), R.xy64_to_point(Q)))
    for P in pts[:4] + [ZERO]:                                             # doubling, the identity included
        for lp in (lam(rng, c), one):
            host, dev = op(helper, c, 1, P, lp, P, lp)
            A = R.xy64_to_point(P)
            assert host == dev == expect(c, R.add(c, A, A))


def combine(L, c, pts, lams, nl):
    out = np.zeros(64, np.uint8)
    inf = np.zeros(1, np.uint8)
    p = np.ascontiguousarray(pts)
    lm = np.frombuffer(b"".join(lams), np.uint8).copy()
    assert L.hp4_combine(c.cid, p.ctypes.data, lm.ctypes.data, nl, out.ctypes.data, inf.ctypes.data) == 0
    return out.tobytes(), int(inf[0])


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_combine_slices_is_the_weighted_sum(helper, c):
    rng = random.Random(77 + c.cid)
    for nl in (1, 2, 7, 16, 19):
        w = np.array([1] + [1 << l for l in range(nl)], dtype=np.uint64)   # the root, then O_l with weight 2^l
        for kind in ("random", "some_identity", "all_identity", "top_identity", "total_identity"):
            pts = points(c)[:nl + 1].copy()
            if kind == "some_identity":
                pts[1::3] = 0
            elif kind == "all_identity":
                pts[:] = 0
            elif kind == "top_identity":                                   # the Horner accumulator starts as the identity
                pts[nl] = 0
            elif kind == "total_identity":                                 # root = -sum_l 2^l O_l: the last addition meets P == -Q
                s = R.INF
                for l in range(nl):
                    s = R.add(c, s, R.mul(c, 1 << l, R.xy64_to_point(pts[1 + l].tobytes())))
                pts[0] = np.frombuffer(R.point_to_xy64(R.neg(c, s)), np.uint8)
            lams = [lam(rng, c) for _ in range(nl + 1)]
            exp = cref.msm_u64(c.cid, w, pts, nl + 1)
            assert combine(helper, c, pts, lams, nl) == exp, (nl, kind)
            if kind == "total_identity":
                assert exp == (ZERO, 1)


def test_equal_slices_meet_the_doubling(helper):
    """L = 1 with O_0 = root = P (two representatives of it): the one addition of the combine is P == Q."""
    c = R.BN254_G1
    P = points(c)[5]
    pts = np.stack([P, P])
    rng = random.Random(5)
    exp = cref.msm_u64(c.cid, np.array([1, 1], dtype=np.uint64), pts, 2)
    assert combine(helper, c, pts, [lam(rng, c), lam(rng, c)], 1) == exp


def test_sanitized_program():
    """The helper's source with its own main(), address + undefined-behaviour sanitizers on, as a stand-alone program."""
    if stale(SAN):
        # -O0: the instrumented build compiles in a quarter of -O1's time
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-DHP4_MAIN", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-o", SAN, SRC])
    r = subprocess.run([SAN], capture_output=True, text=True)
    assert r.returncode == 0 and "self-check ok" in r.stdout, r.stdout + r.stderr
