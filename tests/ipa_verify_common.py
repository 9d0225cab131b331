"""The yardstick of nmx_ipa_verify: InnerProductArgument::verify (/root/reference/src/provider/ipa_pc.rs:286-390) restated with Python
integers and the oracle's MSM, returning every intermediate value -- (s, ck_hat, b_hat, P_hat, verdict) -- so that the device's work
is pinned value by value instead of through one boolean.  Checked against tests/ipa_common.verify, the pyref eq table and the
recurrence of :335-349 in tests/test_ipa_verify_abi.py (CPU); tests/test_gpu_ipa_verify.py takes every expectation from here."""
from collections import namedtuple

import numpy as np

from oracle import cref
from oracle import pyref as R
from tests import ipa_common as ic

Restated = namedtuple("Restated", "s ck_hat b_hat P_hat verdict")
R261 = 1 << 261


def s_vector(p, rs):
    """the recurrence of ipa_pc.rs:335-349, literally"""
    rounds = len(rs)
    n = 1 << rounds
    r_sq = [r * r % p for r in rs]
    r_inv = [pow(r, p - 2, p) for r in rs]
    s = [0] * n
    v = 1
    for x in r_inv:
        v = v * x % p
    s[0] = v
    for i in range(1, n):
        pos = i.bit_length() - 1
        s[i] = s[i - (1 << pos)] * r_sq[(rounds - 1) - pos] % p
    return s


def s_tiled(p, rs, low_bits=8):
    """the decomposition the kernel uses: s[i] = T[i mod 2^lb] * H[i >> lb] with T built by doubling from prod r^-1 and H a chain of
    r^2 factors over the set bits (nova_amd/csrc/ipa_verify.hpp)"""
    ell = len(rs)
    lb = min(ell, low_bits)
    rinv = [pow(r, p - 2, p) for r in rs]
    by_pos_sq = [rs[ell - 1 - pos] ** 2 % p for pos in range(ell)]
    t0 = h0 = 1
    for pos in range(ell):
        if pos < lb:
            t0 = t0 * rinv[ell - 1 - pos] % p
        else:
            h0 = h0 * rinv[ell - 1 - pos] % p
    T = [t0]
    for pos in range(lb):
        T += [x * by_pos_sq[pos] % p for x in T]
    out = []
    for hi in range(1 << (ell - lb)):
        H = h0
        for pos in range(lb, ell):
            if (hi >> (pos - lb)) & 1:
                H = H * by_pos_sq[pos] % p
        out += [t * H % p for t in T]
    return out


def kernel_constants(p, rs, low_bits=8):
    """(t0 internal, hs0 plain, [r^2 by bit position, internal]) as the host half of the call hands them to the kernel"""
    ell = len(rs)
    lb = min(ell, low_bits)
    rinv = [pow(r, p - 2, p) for r in rs]
    t0 = h0 = 1
    for pos in range(ell):
        if pos < lb:
            t0 = t0 * rinv[ell - 1 - pos] % p
        else:
            h0 = h0 * rinv[ell - 1 - pos] % p
    return t0 * R261 % p, h0, [rs[ell - 1 - pos] ** 2 * R261 % p for pos in range(ell)]


def b_hat_closed(p, point, rs):
    """<eq(point), s> without the table: prod_k ((1 - x_k) r_k^-1 + x_k r_k), point[0] the most significant variable"""
    out = 1
    for x, r in zip(point, rs):
        out = out * ((1 - x) * pow(r, p - 2, p) + x * r) % p
    return out


def restate(curve, ck, ckc, comm_a, c, b, Ls, Rs, infs, a_hat, rs):
    """ck: (n, 64) uint8 array; ckc: 64 bytes; comm_a: pyref point (None = identity); c, a_hat, rs, b: Python integers / lists.
    Returns Restated, or None where the reference returns InvalidInputLength / an inversion fails."""
    p = curve.r
    n = len(b)
    rounds = len(Ls)
    if n != 1 << rounds or len(Rs) != rounds or len(rs) != rounds or rounds >= 32 or any(r % p == 0 for r in rs):
        return None
    ck = np.asarray(ck).reshape(-1, 64)
    keypts = [ic.pt(ck[i].tobytes()) for i in range(n)]
    U = ic.pt(bytes(ckc))
    P = R.add(curve, comm_a, R.mul(curve, c % p, U))                                      # :313
    r_sq = [r * r % p for r in rs]
    r_inv_sq = [pow(r, p - 2, p) ** 2 % p for r in rs]
    s = s_vector(p, rs)
    ck_hat = ic.msm_pts(curve, s, keypts) if n > 16 else R.msm_naive(curve, s, keypts)    # :351-354
    b_hat = sum(x * y for x, y in zip(b, s)) % p                                          # :356
    infs = infs or [(False, False)] * rounds
    pts = [ic.pt(L, i[0]) for L, i in zip(Ls, infs)] + [ic.pt(Rr, i[1]) for Rr, i in zip(Rs, infs)] + [P]
    P_hat = R.msm_naive(curve, r_sq + r_inv_sq + [1], pts)                                # :358-376
    rhs = R.add(curve, R.mul(curve, a_hat % p, ck_hat), R.mul(curve, a_hat * b_hat % p, U))   # :378-388
    return Restated(s, ck_hat, b_hat, P_hat, P_hat == rhs)


def instance_of(curve, n, seed, zero_a=False):
    """An instance and an honest proof from the oracle's prover (the key-folding restatement): dict with ck, ckc, a, b (arrays),
    comm_a (pyref point), c, Ls, Rs, infs, a_hat (bytes), rs (integers)."""
    ck, ckc, a, b = ic.make_instance(curve, n, seed)
    if zero_a:
        a[:] = 0
    tr = ic.IpaTranscript(curve.r)
    Ls, Rs, infs, a_hat = cref.ipa_prove(curve.cid, ck, ckc, a, b, n, cref.make_ipa_transcript(tr))
    ai, bi = ic.ints(a), ic.ints(b)
    keypts = [ic.pt(ck[i].tobytes()) for i in range(n)]
    comm_a = ic.msm_pts(curve, ai, keypts) if n > 16 else R.msm_naive(curve, ai, keypts)
    return dict(curve=curve, n=n, ck=ck, ckc=ckc.tobytes(), a=a, b=b, bi=bi, comm_a=comm_a,
                c=sum(x * y for x, y in zip(ai, bi)) % curve.r, Ls=list(Ls), Rs=list(Rs), infs=list(infs), a_hat=bytes(a_hat), rs=list(tr.rs))


def restate_instance(I, **over):
    J = dict(I, **over)
    return restate(J["curve"], J["ck"], J["ckc"], J["comm_a"], J["c"], J["bi"], J["Ls"], J["Rs"], J["infs"],
                   int.from_bytes(J["a_hat"], "little"), J["rs"])


def other_point(curve, k=424242):
    """some point of the curve that is none of the instance's"""
    return R.mul(curve, k, (curve.gx, curve.gy))


def tampers(I):
    """name -> overrides of the instance, each a single change that must be rejected (the cases of the issue)"""
    curve, p, n = I["curve"], I["curve"].r, I["n"]
    X = ic.pt_bytes(other_point(curve))
    out = {}
    if I["Ls"]:
        k = len(I["Ls"]) // 2
        out["L_k"] = dict(Ls=I["Ls"][:k] + [X] + I["Ls"][k + 1:], infs=[(False, i[1]) if j == k else i for j, i in enumerate(I["infs"])])
        out["R_k"] = dict(Rs=I["Rs"][:k] + [X] + I["Rs"][k + 1:], infs=[(i[0], False) if j == k else i for j, i in enumerate(I["infs"])])
        out["L_R_swapped"] = dict(Ls=I["Ls"][:k] + [I["Rs"][k]] + I["Ls"][k + 1:], Rs=I["Rs"][:k] + [I["Ls"][k]] + I["Rs"][k + 1:],
                                  infs=[(i[1], i[0]) if j == k else i for j, i in enumerate(I["infs"])])
        out["challenge"] = dict(rs=I["rs"][:k] + [(I["rs"][k] + 1) % p or 1] + I["rs"][k + 1:])
    out["a_hat"] = dict(a_hat=ic.le((int.from_bytes(I["a_hat"], "little") + 1) % p))
    out["c"] = dict(c=(I["c"] + 1) % p)
    out["comm_a"] = dict(comm_a=R.add(curve, I["comm_a"], other_point(curve)))
    if I["Ls"]:  # (without a round the equation is comm_a + c U = a_hat ck[0] + a_hat b[0] U: it holds for every U)
        out["ck_c"] = dict(ckc=X)
    for name, j in (("b_first", 0), ("b_last", n - 1), ("b_middle", n // 2)):
        if name == "b_first" or n > 2 or (name == "b_last" and n == 2):
            bi = list(I["bi"])
            bi[j] = (bi[j] + 1) % p
            out[name] = dict(bi=bi)
    return out


def b_array(bi):
    return np.frombuffer(b"".join(ic.le(x) for x in bi), np.uint8).copy()
