"""Shared by tests/test_key_ext_abi.py (CPU) and tests/test_gpu_key_ext.py: the weights, pairs and source rows of nmx_bases_fold /
nmx_bases_scale / nmx_bases_concat and their expected keys.  The source key is always key[i] = s_i * G for known scalars s_i
(CommitmentKey.from_scalars on the GPU, pyref.mul for the emulation), so fold gives ((w1 s_i + w2 s_{i+h}) mod r) * G and scale gives
((r s_i) mod r) * G -- pyref.mul, cached in tests/fixed_base_common.py -- the identity when that scalar is 0.  No tolerance anywhere:
comparisons are on points or on the bytes of read()."""
import random

from oracle import pyref as R
from tests import fixed_base_common as fb

CURVES = fb.CURVES
SIZES = (1, 2, 255, 256, 257, 513)      # outputs: below, at and above the block of 256 lanes; three blocks with one lane in the last


def bits(c):
    return c.r.bit_length()             # 254 (BN254 G1, Grumpkin) or 255 (Pallas, Vesta)


def edge_weights(c):
    """0, 1, 2, r - 1, the largest 2^k - 1 below r, 0x5555... and 0x3333... (cut below bit BITS - 1, so both are below r), a value with bit
    BITS - 1 set"""
    B = bits(c)
    low = (1 << (B - 1)) - 1
    ws = [0, 1, 2, c.r - 1, low, int("55" * 32, 16) & low, int("33" * 32, 16) & low, (1 << (B - 1)) | 0x1234567]
    assert all(0 <= w < c.r for w in ws) and low + 1 < c.r <= 2 * low + 1 and ws[-1] >> (B - 1) == 1
    return ws


def edge_pairs(c, w):
    """(w, w), (w, w + 1), (w, r - w), (0, w), (w, 0), (r - 1, r - 1)"""
    assert 0 < w < c.r - 1
    return [(w, w), (w, w + 1), (w, c.r - w), (0, w), (w, 0), (c.r - 1, c.r - 1)]


def random_weight(c, seed):
    return random.Random(7000 + 10 * seed + c.cid).randrange(2, c.r - 1)


def all_pairs(c):
    """every pair the fold tests run: the edge pairs of a random w, every edge weight against a random partner on either side"""
    w = random_weight(c, 1)
    out = edge_pairs(c, w)
    for i, e in enumerate(edge_weights(c)):
        out.append((e, random_weight(c, 2 + i)))
        out.append((random_weight(c, 20 + i), e))
    return out


def source_scalars(c, n, seed=1):
    """n scalars for a key that is folded at h = n // 2, with the group-law edges in its first rows (as many as fit): row 0 equal
    (L == R), row 1 opposite (R == -L), row 2 an identity in L, row 3 an identity in R, row 4 identities in both; every other row random
    and non-zero.  For scale the same key holds identity rows at 2, h + 3, 4 and h + 4."""
    rng = random.Random(seed * 977 + c.cid)
    s = [rng.randrange(1, c.r) for _ in range(n)]
    h = n // 2
    if h > 0:
        s[h] = s[0]
    if h > 1:
        s[h + 1] = c.r - s[1]
    if h > 2:
        s[2] = 0
    if h > 3:
        s[h + 3] = 0
    if h > 4:
        s[4] = s[h + 4] = 0
    return s


def fold_scalars(c, s, w1, w2, n=None, offset=0):
    n = len(s) - offset if n is None else n
    h = n // 2
    return [(w1 * s[offset + i] + w2 * s[offset + h + i]) % c.r for i in range(h)]


def scale_scalars(c, s, r):
    return [r * x % c.r for x in s]


def points(c, scalars):
    return fb.expect_points(c, scalars)


def rows(c, scalars):
    """the key [s G] as read() returns it: (n, 64) uint8, all zero for the identity"""
    return fb.xy64_rows(fb.expect_points(c, scalars))


def decode(codes, length, names):
    """(codes of ke_recode, one per position) -> (w1, w2) as the integers the digit stream stands for; names: emul_ke_geometry"""
    P0, P1, SUM, DIFF, NEG = names
    a = b = 0
    for j in range(length):
        code = int(codes[j])
        sel, sign = code & 7, -1 if code & NEG else 1
        if sel == 0:
            assert code == 0, "a sign without a point"
            continue
        assert sel in (P0, P1, SUM, DIFF), code
        if sel in (P0, SUM, DIFF):
            a += sign << j
        if sel in (P1, SUM):
            b += sign << j
        if sel == DIFF:
            b -= sign << j
    return a, b


def tensor_vector(c, rs):
    """the vector s of ipa_pc.rs:335-349 for the challenges rs (first round first), with the reference's indexing: s[0] = prod of the
    r_j^-1, s[i] = s[i - 2^pos] * r^2[(k - 1) - pos] for pos the top bit of i -- so that folding a 2^k-point key k times with
    (r_j^-1, r_j) leaves <s, ck>"""
    k = len(rs)
    s = [0] * (1 << k)
    s[0] = 1
    for x in rs:
        s[0] = s[0] * pow(x, -1, c.r) % c.r
    for i in range(1, 1 << k):
        pos = i.bit_length() - 1
        s[i] = s[i - (1 << pos)] * rs[(k - 1) - pos] ** 2 % c.r
    return s
