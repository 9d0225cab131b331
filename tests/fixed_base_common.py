"""Shared by tests/test_fixed_base_abi.py (CPU) and tests/test_gpu_fixed_base.py: the scalar sets of the fixed-base key calls
(nmx_bases_from_scalars / nmx_bases_setup_from_tau) and their expected points, always pyref.mul(c, s % r, B) -- cached, since the same
scalar meets the same base under several window widths and forms."""
import functools
import random

import numpy as np

from oracle import pyref as R

CURVES = [R.BN254_G1, R.GRUMPKIN, R.PALLAS, R.VESTA]
WIDTHS = (4, 8, 13)          # the default, one that divides neither 32 nor the scalar width evenly (13), the narrowest
R256 = 1 << 256


def windows(c, cw):
    """ceil(BITS / cw) with BITS the bit length of the scalar modulus (nova_amd/csrc/fixed_base.hpp fb_windows)"""
    return (c.r.bit_length() + cw - 1) // cw


def special_scalars(c, cw):
    """0, 1, 2, r - 1, 2^cw - 1, a value whose only non-zero digit is the top window's, and the largest value below r whose lower digits
    are all 2^cw - 1 (its top digit is one below r's, so every digit is at the maximum a canonical scalar lets it take there)"""
    s = cw * (windows(c, cw) - 1)
    top_only = 1 << s
    top_r = c.r >> s
    assert 1 <= top_r < (1 << cw) and top_only < c.r
    all_max = ((top_r - 1) << s) | ((1 << s) - 1)
    assert all_max < c.r and all(((all_max >> (cw * w)) & ((1 << cw) - 1)) == (1 << cw) - 1 for w in range(windows(c, cw) - 1))
    return [0, 1, 2, c.r - 1, (1 << cw) - 1, top_only, all_max]


def scalar_set(c, cw, n, seed=1):
    """n scalars below r: random ones, the special values from lane 2 on, and lanes 0, 1 and 255 zero (identity lanes at both ends of the
    first block); lane 256 -- the second block's only lane at n = 257 -- stays random and non-zero"""
    rng = random.Random(seed * 1000 + c.cid)
    s = [rng.randrange(1, c.r) for _ in range(n)]
    for i, v in enumerate(special_scalars(c, cw)):
        if 2 + i < n:
            s[2 + i] = v
    for i in (0, 1, 255):
        if i < n and n > 2:
            s[i] = 0
    return s


@functools.lru_cache(maxsize=None)
def _mul(cid, k, B):
    return R.mul(R.CURVES_BY_ID[cid], k, B)


def expect_points(c, scalars, B=None):
    """[s * B] as affine tuples / INF; B defaults to the generator"""
    B = (c.gx, c.gy) if B is None else B
    return [_mul(c.cid, s % c.r, B) for s in scalars]


def xy64_rows(points):
    return np.frombuffer(b"".join(R.point_to_xy64(P) for P in points), np.uint8).reshape(-1, 64).copy()


def scalar_rows(c, scalars, mont=False):
    """(n, 32) uint8: canonical little-endian, or s * 2^256 mod r"""
    f = (lambda v: v * R256 % c.r) if mont else (lambda v: v)
    return np.frombuffer(b"".join(int(f(v)).to_bytes(32, "little") for v in scalars), np.uint8).reshape(-1, 32).copy()


def base_bytes(c, B, mont=False):
    """64 bytes x || y of B: canonical, or both coordinates times 2^256 mod p"""
    f = (lambda v: v * R256 % c.p) if mont else (lambda v: v)
    return np.frombuffer(int(f(B[0])).to_bytes(32, "little") + int(f(B[1])).to_bytes(32, "little"), np.uint8).copy()


def tau_powers(c, tau, n, begin=0):
    out, t = [], pow(tau, begin, c.r)
    for _ in range(n):
        out.append(t)
        t = t * tau % c.r
    return out
