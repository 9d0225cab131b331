"""Shared by tests/test_derive_key_abi.py (CPU) and tests/test_gpu_derive_key.py: cases of nmx_bases_derive_by_address and their expected keys.
The source key is always key[i] = s_i * G for known scalars s_i (CommitmentKey.from_scalars on the GPU, pyref.mul for the emulation), so
derived[j] = (sum of s_i over the entries of index j, mod r) * G -- pyref.mul, cached in tests/fixed_base_common.py -- and the identity when
that sum is 0 mod r.  No tolerance anywhere: comparisons are on points or on the bytes of read()."""
import random

import numpy as np

from oracle import pyref as R
from tests import fixed_base_common as fb

CURVES = fb.CURVES
RI = 1 << 261          # the internal residue form: x * 2^261 mod p (nova_amd/csrc/fp.hpp)


def expect_sums(c, scalars, addresses, table_size):
    """per table index: the sum of the scalars whose address it is, mod r; scalars beyond len(addresses) are ignored"""
    sums = [0] * table_size
    for s, a in zip(scalars, addresses):
        sums[a] = (sums[a] + s) % c.r
    return sums


def expect_points(c, scalars, addresses, table_size):
    """the derived key as affine tuples / INF"""
    return fb.expect_points(c, expect_sums(c, scalars, addresses, table_size))


def expect_bytes(c, scalars, addresses, table_size):
    """the derived key as read() returns it: (table_size, 64) uint8, canonical x || y, all zero for the identity"""
    return fb.xy64_rows(expect_points(c, scalars, addresses, table_size))


def internal_rows(c, points):
    """(n, 16) uint32: x || y in the internal form, all zero for INF -- what a resident key holds"""
    b = b"".join(bytes(64) if P is R.INF else (P[0] * RI % c.p).to_bytes(32, "little") + (P[1] * RI % c.p).to_bytes(32, "little") for P in points)
    return np.frombuffer(b, np.uint8).view(np.uint32).reshape(-1, 16).copy()


def points_from_internal(c, words):
    """(m x 16 words, internal form) -> affine tuples / INF; every stored coordinate must be canonical"""
    inv = pow(RI, -1, c.p)
    out = []
    for row in np.ascontiguousarray(words).view(np.uint8).reshape(-1, 64):
        x, y = int.from_bytes(bytes(row[:32]), "little"), int.from_bytes(bytes(row[32:]), "little")
        assert x < c.p and y < c.p, "a stored coordinate is not canonical"
        out.append(R.INF if x == 0 and y == 0 else (x * inv % c.p, y * inv % c.p))
    return out


def heavy_case(L, table_size=8, heavy=5, others=(0, 3, 7)):
    """addresses: index `heavy` holds L entries, three other indices one each, spread through the array; scalars i + 1"""
    n = L + len(others)
    addr = [heavy] * n
    for pos, o in zip(random.Random(L).sample(range(n), len(others)), others):
        addr[pos] = o
    assert addr.count(heavy) == L and heavy not in others
    return addr, list(range(1, n + 1))
