"""Inputs with a closed-form answer that put equal, opposite and identity operands into every point addition of the MSM, and scalars
that hold the signed-digit recoding at its boundaries (tests/test_msm_degenerate.py on the CPU emulation, tests/test_gpu_msm_degenerate.py
on the device).

Rank-one keys.  Every row of the key is +P, -P or the identity row (64 zero bytes), P = 7 G, so the MSM is (sum_i sign_i s_i mod r) P: one
big-int sum and one pyref.mul whatever n is, and whatever two partial sums meet in an addition are multiples aP and bP of one point -- equal
(the doubling branch) as soon as a == b, opposite (the cancellation branch) when a == -b, the identity when a == 0.  The scalar families
below choose a and b stage by stage:

  cyc(k)         scalars 1 + (i mod 2^k) over the all-+P key.  With k <= c - 1 every scalar is its own window-0 digit (<= M = 2^(c-1): positive,
                 no carry), so buckets 0 .. 2^k - 1 of window 0 (the only bucket set a key with window tables has) each hold a P with
                 a = n / 2^k, and nothing else is non-empty.  The pair tree (ReducePairFn / k_reduce_tree: D'_j = 2 (D_2j + D_2j+1),
                 Y'_j = Y_2j + Y_2j+1 + D_2j+1, Y = D = B on entry) then adds two EQUAL points in every D addition of its first k levels
                 (level l: all D are 4^l a P), and the bit-sliced reduction (reduce_bitsliced.hpp: N = sums of halves, O = sums of the
                 odd-indexed elements of each level) sums arrays whose elements are all equal: every addition is a doubling.
                 The rows past the last whole cycle get the scalar 0 (dropped by the digit stage), so the buckets stay equal at any n;
                 with n < 2^k the cycle never completes and buckets 0 .. n - 1 hold one P each (the tree doubles through log2(n) levels).
  cyc_cancel(k)  the same scalars over the alternating key (+P on even rows, -P on odd rows: odd scalars meet +P, even scalars -P).  Bucket
                 2j holds +aP and bucket 2j+1 holds -aP: every level-0 pair of the tree cancels to the identity (D' = 2 * O), while
                 Y' = B_2j + 2 B_2j+1 = -aP and the odd-element arrays (all -aP) still double.  Total: -a 2^(k-1) P, not the identity.
  heavy          one full-width scalar on every row: each window puts all n points into ONE bucket.  Over the all-+P key the accumulate
                 stage cuts that bucket into equal-length pieces whose partial sums are equal, so the strided folds (FoldFn,
                 FoldRawQuadFn, k_big_all), the lane tree above them and k_small_accum / k_small_combine double at every step; in a lane's
                 own run the second addition is P + P (add_affine_signed's doubling branch) and later ones jP + P.  Over the alternating key
                 (heavy+-) every second addition inside a run is P + (-P) and every even-length piece sums to the identity: with n even
                 the whole MSM is the identity, with n odd one point survives.  Over the mixed key (+P, -P, identity, ...) identity rows
                 sit between them.

Digit edges.  The recoding d_w = window_w + carry, negative (d - 2^c, carry 1) iff d > M, exists three times in the library (DigitSrc::digit,
the bit-buffer loop of DigitsFn / for_each_digit<0>, the funnel-shift form of for_each_digit<8 | 15 | 16>).  digit_edges(cw, curve) holds, for
every window: a digit exactly M (stays positive), exactly M + 1 (the first negative one), M + 1 reached through a carry (all-M plus one),
the digit 2^c that a carry makes of an all-ones window (a zero digit with carry 1: 2^k - 1), a single bit walked through every position
(2^k: every 32-bit word boundary a window read straddles), and the values next to r whose top window is the partial one.  They run over
multiples_key (rows kP, k = 1 .. 8 cycled), whose closed form is sum_i k_i s_i, and once over distinct points against the oracle.
"""
import functools
import hashlib

import numpy as np

from oracle import pyref as R


# ---------------------------------------------------------------------------------------------------------------------------------------
# keys
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _multiples(name):
    c = R.CURVES[name]
    P = R.mul(c, 7, (c.gx, c.gy))
    return [R.INF] + [R.mul(c, k, P) for k in range(1, 9)]


def base_point(c):
    """P = 7 G: not the generator, whose small coordinates could hide a wrong limb"""
    return _multiples(c.name)[1]


def signs_plus(n):
    return np.ones(n, np.int64)


def signs_alt(n):
    """+P on even rows, -P on odd rows"""
    s = np.ones(n, np.int64)
    s[1::2] = -1
    return s


def signs_mixed(n):
    """+P, -P, identity, +P, -P, identity, ..."""
    return np.resize(np.array([1, -1, 0], np.int64), n)


def rank_one_key(c, n, signs):
    """(n, 64) uint8: row i is P (signs[i] = 1), -P (-1) or the all-zero identity row (0)"""
    P = base_point(c)
    table = np.frombuffer(R.point_to_xy64(R.neg(c, P)) + bytes(64) + R.point_to_xy64(P), np.uint8).reshape(3, 64)
    signs = np.asarray(signs, np.int64)
    assert len(signs) == n and np.all(np.abs(signs) <= 1)
    return np.ascontiguousarray(table[signs + 1])


def multiples_coeffs(n):
    return (np.arange(n, dtype=np.int64) % 8) + 1


def multiples_key(c, n):
    """(n, 64) uint8: rows kP for k = 1 .. 8, cycled -- eight distinct points, so unequal operands meet too"""
    pts = _multiples(c.name)
    table = np.frombuffer(b"".join(R.point_to_xy64(p) for p in pts), np.uint8).reshape(9, 64)
    return np.ascontiguousarray(table[multiples_coeffs(n)])


# ---------------------------------------------------------------------------------------------------------------------------------------
# scalars as Python integers, and their byte forms
# ---------------------------------------------------------------------------------------------------------------------------------------
def as_ints(scalars):
    if isinstance(scalars, np.ndarray):
        if scalars.dtype == np.uint64:
            return [int(v) for v in scalars]
        return [int.from_bytes(bytes(row), "little") for row in scalars.reshape(-1, 32)]
    return [int(v) for v in scalars]


def rows32(ints):
    """-> (n, 32) uint8 canonical little-endian"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), np.uint8).reshape(-1, 32).copy()


def tile(vals, n):
    return [vals[i % len(vals)] for i in range(n)]


def chunks(vals, n):
    """the whole of vals as vectors of exactly n scalars: one (tiled) when n >= len(vals), else consecutive slices, the last one tiled"""
    return [tile(vals[i:i + n], n) for i in range(0, len(vals), n)]


def expect(c, scalars, coeffs):
    """(xy64, is_inf) of (sum_i coeffs[i] * scalars[i] mod r) * P"""
    s = as_ints(scalars)
    assert len(s) == len(coeffs)
    t = sum(int(k) * v for k, v in zip(coeffs, s)) % c.r
    pt = R.mul(c, t, base_point(c))
    return (R.point_to_xy64(pt), 1 if pt is R.INF else 0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the model: signed digits and bucket multiplicities in Python integers
# ---------------------------------------------------------------------------------------------------------------------------------------
def n_windows(cw, bits):
    return (bits + cw) // cw            # ceil((bits + 1) / cw): the top window absorbs the last carry


def signed_digits(s, cw, bits):
    """d_w in [-(M - 1), M], M = 2^(cw-1), with sum_w d_w 2^(cw w) == s: a window plus the carry is negative iff it exceeds M"""
    M, out, carry = 1 << (cw - 1), [], 0
    for w in range(n_windows(cw, bits)):
        d = ((s >> (cw * w)) & ((1 << cw) - 1)) + carry
        carry = 1 if d > M else 0
        out.append(d - (carry << cw))
    assert carry == 0 and sum(d << (cw * w) for w, d in enumerate(out)) == s
    return out


def bucket_mults(r, scalars, signs, cw, bits):
    """m[w][d] for d = 1 .. M: bucket d of window w of a rank-one key holds m[w][d] * P (mod r); buckets no point reaches are absent"""
    m = [dict() for _ in range(n_windows(cw, bits))]
    for s, sg in zip(scalars, signs):
        if sg == 0 or s == 0:
            continue                   # identity rows and zero digits never reach a bucket
        for w, d in enumerate(signed_digits(s, cw, bits)):
            if d:
                m[w][abs(d)] = (m[w].get(abs(d), 0) + (int(sg) if d > 0 else -int(sg))) % r
    return m


# the library's window-width rules (msm_pipeline.hpp settle_c / choose_c / choose_c_precomp), only to pick k = c - 1 and the widths whose
# digit edges a default-width call should see; a wrong guess here weakens an input, never an expected value
def _settle_c(c0, lo, hi, bits):
    best, best_score = c0, -1
    for cw in (c0 - 1, c0, c0 + 1):
        if cw < lo or cw > hi:
            continue
        top = bits + 1 - (n_windows(cw, bits) - 1) * cw
        score = (1000 if top * 2 >= cw else top * 10) - (0 if cw == c0 else 1)
        if score > best_score:
            best, best_score = cw, score
    return best


def table_width(n_key, bits):
    lg = max(n_key, 2).bit_length() - 1
    if lg >= 22:
        return 20
    if lg >= 20:
        return 17
    return _settle_c(16 if lg >= 17 else 15 if lg >= 14 else 8, 8, 16, bits)


def plain_width(n, bits):
    cw = min(max(max(n, 2).bit_length() - 1 - 4, 3), 16)
    return _settle_c(cw, 5, 16, bits) if cw >= 6 else cw


# ---------------------------------------------------------------------------------------------------------------------------------------
# scalar families
# ---------------------------------------------------------------------------------------------------------------------------------------
def cyc(n, k):
    """1 + (i mod 2^k) on the whole cycles, 0 on the rows behind them (every one of the 2^k buckets then holds the same count); with
    n < 2^k no cycle completes and the scalars are 1 .. n"""
    full = (n >> k) << k or n
    return [1 + (i & ((1 << k) - 1)) if i < full else 0 for i in range(n)]


def cyc_total(n, k):
    """sum of cyc(n, k) (the all-+P key) and the alternating-key sum (cyc_cancel) as integers, for the asserts on the totals"""
    s = cyc(n, k)
    return sum(s), sum(v if i % 2 == 0 else -v for i, v in enumerate(s))


def heavy_scalar(c):
    """one full-width scalar, the same for every caller: SHA-256 of the curve's name, reduced mod r"""
    return int.from_bytes(hashlib.sha256(b"heavy " + c.name.encode()).digest(), "little") % c.r


def heavy(c, n):
    return [heavy_scalar(c)] * n


def _stacked(v, cw, W, bound):
    """every window equal to v, added from the bottom while the value stays below bound (never reduced: that would destroy the pattern)"""
    s = 0
    for w in range(W):
        if s + (v << (cw * w)) >= bound:
            break
        s += v << (cw * w)
    return s


def _dedup(vals):
    return list(dict.fromkeys(vals))


def digit_edges(cw, c):
    """the scalars of the module docstring for window width cw on curve c, all in [0, r)"""
    r, bits = c.r, c.r.bit_length()
    W, M = n_windows(cw, bits), 1 << (cw - 1)
    all_m = _stacked(M, cw, W, r)
    out = [0, all_m, all_m + 1, _stacked(M + 1, cw, W, r)]
    out += [(1 << k) - 1 for k in range(bits)] + [1 << k for k in range(bits)]
    out += [r - 1, r - 2] + [r - (1 << k) for k in range(2 * cw)] + [(r + 1) // 2, (r - 1) // 2]
    out += [(M + 1) << (cw * w) for w in range(W) if (M + 1) << (cw * w) < r]      # exactly M + 1 with no carry coming in
    assert all(0 <= v < r for v in out)
    return _dedup(out)


def digit_edges_for(widths, c):
    return _dedup([v for cw in widths for v in digit_edges(cw, c)])


def u64_edges(cw, b):
    """u64 scalars for a declared width of b bits: 2^b - 1, M, M + 1, the stacked-M pattern and its successor, 0 and 1 -- those below 2^b"""
    M, W = 1 << (cw - 1), n_windows(cw, b)
    all_m = _stacked(M, cw, W, 1 << b)
    return _dedup([v for v in (0, 1, (1 << b) - 1, M, M + 1, all_m, all_m + 1, _stacked(M + 1, cw, W, 1 << b)) if v < 1 << b])


def u64_widths(cw):
    return _dedup([b for b in (1, cw - 1, cw, cw + 1, 63, 64) if 1 <= b <= 64])
