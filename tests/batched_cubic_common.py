"""Shared checks for the batched cubic sum-check (SumcheckProof::prove_batched_cubic, /root/reference/src/spartan/sumcheck.rs:509-577):

    sum_x eq(tau, x) * sum_i alpha_i (A_i(x) B_i(x) - C_i(x)) = claim        for K triples under one sum-check.

One driver, check_batched_cubic, runs against the host prover (CPU, tests/test_sumcheck_batched_abi.py), the plain restatement below
and the HIP path through the C ABI (GPU, tests/test_gpu_sumcheck_batched.py).  As in tests/spartan_common.py what pins a prover is the
reference's VERIFIER restated with Python big integers (SumcheckProof::verify, sumcheck.rs:87-129, and the final-claim equation), the
final evaluations, and at small sizes the DEFINITION of every round polynomial by brute force.  Everything is exact."""
import numpy as np

from tests import fv_common as fc
from tests.spartan_common import StandInTranscript, eq_eval, ints, le, mle_eval, poly_at, verify_rounds


def eq_table(p, taus):
    """EqPolynomial::evals (eq.rs:54-73): [eq(taus, x) for x in 0 .. 2^len), the first tau the most significant bit"""
    t = [1]
    for tau in taus:
        t = [v * f % p for v in t for f in ((1 - tau) % p, tau)]
    return t


def brute_round_poly_batched(p, taus, As, Bs, Cs, alphas, rs_so_far, x):
    """s_j(x) = sum_{y in {0,1}^(l-j)} eq(tau, (r_1..r_{j-1}, x, y)) sum_i alpha_i (A_i B_i - C_i)(r_1..r_{j-1}, x, y): the definition
    (spartan_common.brute_round_poly_cubic with the alpha sum)."""
    l, j = len(taus), len(rs_so_far)
    rest = l - j - 1
    tot = 0
    for y in range(1 << rest):
        pt = list(rs_so_far) + [x] + [(y >> (rest - 1 - t)) & 1 for t in range(rest)]
        inner = sum(al * (mle_eval(p, A, pt) * mle_eval(p, B, pt) - mle_eval(p, C, pt)) for al, A, B, C in zip(alphas, As, Bs, Cs))
        tot = (tot + eq_eval(p, taus, pt) * inner) % p
    return tot


def zeroing_challenge(p, tau):
    """the r with eq(tau, r) = 1 - tau - r + 2 r tau = 0: after it eval_eq_left is zero and derive_from_claim_deg2 returns None in every
    later round (l(1) p = 0 has no inverse, sumcheck.rs:694-696)"""
    return (1 - tau) * pow((1 - 2 * tau) % p, -1, p) % p


def make_instance(fid, l, k, seed, taus=None, alphas=None, fill=None):
    """-> (A, B, C lists of (2^l, 32) uint8 arrays, taus (l, 32), alphas (k, 32)).  fill: every table entry is that value."""
    p = fc.FIELDS[fid]
    n = 1 << l
    if fill is None:
        As, Bs, Cs = ([fc.edge_vectors(fid, n, seed + 10 * i + w) for i in range(k)] for w in range(3))
    else:
        As, Bs, Cs = ([fc.vec([fill % p] * n) for _ in range(k)] for _ in range(3))
    tv = fc.rand_vec(fid, l, seed + 7).copy() if taus is None else fc.vec(taus)
    av = fc.rand_vec(fid, k, seed + 8).copy() if alphas is None else fc.vec(alphas)
    return As, Bs, Cs, tv, av


def check_batched_cubic(prove, fid, l, k, seed, force=None, taus=None, alphas=None, fill=None, brute=None):
    """prove(fid, claim, taus_vec, As, Bs, Cs, alphas_vec, transcript_callable) -> (polys [l][4], r [l], claims [k][3]) as 32-byte strings."""
    p = fc.FIELDS[fid]
    n = 1 << l
    As, Bs, Cs, tv, av = make_instance(fid, l, k, seed, taus, alphas, fill)
    Ai, Bi, Ci, ti, al = [ints(v) for v in As], [ints(v) for v in Bs], [ints(v) for v in Cs], ints(tv), ints(av)
    eqt = eq_table(p, ti)
    claim = sum(eqt[x] * sum(al[i] * (Ai[i][x] * Bi[i][x] - Ci[i][x]) for i in range(k)) for x in range(n)) % p   # brute force over the hypercube
    tr = StandInTranscript(p, force=force)
    polys, rs, claims = prove(fid, le(claim), tv, As, Bs, Cs, av, tr)
    polys_i = [[int.from_bytes(c, "little") for c in row] for row in polys]
    rs_i = [int.from_bytes(x, "little") for x in rs]
    assert len(polys_i) == l and all(len(row) == 4 for row in polys_i)
    assert polys_i == tr.polys and rs_i == tr.rs, "the prover must hand the transcript exactly what it returns"
    e = verify_rounds(p, claim, polys_i, rs_i, 3)
    cl = [[int.from_bytes(c, "little") for c in row] for row in claims]
    assert cl == [[mle_eval(p, Ai[i], rs_i), mle_eval(p, Bi[i], rs_i), mle_eval(p, Ci[i], rs_i)] for i in range(k)], \
        "claims[i] = [A_i(r), B_i(r), C_i(r)] (sumcheck.rs:566-568)"
    assert e == eq_eval(p, ti, rs_i) * sum(al[i] * (cl[i][0] * cl[i][1] - cl[i][2]) for i in range(k)) % p, \
        "e == eq(tau, r) * sum_i alpha_i (A_i(r) B_i(r) - C_i(r))"
    if brute if brute is not None else l <= 5:
        for j in range(l):
            for x in (0, 1, 2, p - 1):
                assert poly_at(p, polys_i[j], x) == brute_round_poly_batched(p, ti, Ai, Bi, Ci, al, rs_i[:j], x), (j, x)
    return polys, rs, claims


def py_prove(fid, claim, taus, As, Bs, Cs, alphas, tr):
    """prove_batched_cubic restated line by line in Python integers (sumcheck.rs:509-577 with evaluation_points_batched_cubic,
    derive_from_claim_deg2 -- its None branch included -- and fallback_eval_inf_batched_cubic, :680-715, :749-894): the CPU-side `prove`."""
    p = fc.FIELDS[fid]
    A, B, C = [ints(v) for v in As], [ints(v) for v in Bs], [ints(v) for v in Cs]
    ti, al = ints(taus) if len(taus) else [], ints(alphas)
    k, l = len(A), len(ti)
    assert k > 0 and k == len(B) == len(C) == len(al)
    claim = int.from_bytes(bytes(claim), "little")
    inv2 = pow(2, -1, p)
    eval_eq_left, polys, rs = 1, [], []
    for j in range(l):
        tau = ti[j]
        eq_0, eq_slope = (1 - tau) % p, (2 * tau - 1) % p
        eq_m1 = (eq_0 - eq_slope) % p
        fac = eq_table(p, ti[j + 1:])      # poly_eq_left[..][id >> s] * poly_eq_right[..][id & mask] / poly_eq_right[..][id], spelled out
        h = len(A[0]) // 2
        t_0 = t_inf = 0
        for idx in range(h):
            s0 = sq = 0
            for i in range(k):
                s0 += al[i] * (A[i][idx] * B[i][idx] - C[i][idx])
                sq += al[i] * (A[i][idx + h] - A[i][idx]) * (B[i][idx + h] - B[i][idx])
            t_0, t_inf = (t_0 + s0 * fac[idx]) % p, (t_inf + sq * fac[idx]) % p
        l_0_p, l_1_p = eq_0 * eval_eq_left % p, tau * eval_eq_left % p
        s_0, s_lead = l_0_p * t_0 % p, eq_slope * eval_eq_left * t_inf % p
        if l_1_p != 0:                     # derive_from_claim_deg2 -> Some
            t_1 = (claim - s_0) * pow(l_1_p, -1, p) % p
            t_m1 = (2 * t_inf + 2 * t_0 - t_1) % p
        else:                              # -> None: fallback_eval_inf_batched_cubic, the third sum
            t_m1 = 0
            for idx in range(h):
                s = 0
                for i in range(k):
                    ma, mb, mc = (2 * X[i][idx] - X[i][idx + h] for X in (A, B, C))
                    s += al[i] * (ma * mb - mc)
                t_m1 = (t_m1 + s * fac[idx]) % p
        s_m1 = eq_m1 * eval_eq_left * t_m1 % p
        s_1 = (claim - s_0) % p            # UniPoly::from_evals_deg3([s(0), s(1), cubic coefficient, s(-1)]) (univariate.rs:103-113)
        c2 = ((s_1 + s_m1) * inv2 - s_0) % p
        co = [s_0, (s_1 - s_lead - s_0 - c2) % p, c2, s_lead]
        r = int.from_bytes(tr([le(c) for c in co]), "little")
        polys.append([le(c) for c in co])
        rs.append(le(r))
        claim = poly_at(p, co, r)
        for X in (A, B, C):
            for i in range(k):
                X[i] = [(X[i][idx] + r * (X[i][idx + h] - X[i][idx])) % p for idx in range(h)]
        eval_eq_left = eval_eq_left * ((1 - tau - r + 2 * r * tau) % p) % p
    return polys, rs, [[le(A[i][0]), le(B[i][0]), le(C[i][0])] for i in range(k)]


def montgomery_wrapped(prove_m, fid):
    """a prover that takes and returns halo2curves Montgomery words (x 2^256), behind the canonical interface of check_batched_cubic"""
    p = fc.FIELDS[fid]
    Rm = 1 << 256
    to_m = lambda v: fc.vec([x * Rm % p for x in ints(v)])  # noqa: E731
    un_m = lambda b: int(int.from_bytes(b, "little") * pow(Rm, -1, p) % p).to_bytes(32, "little")  # noqa: E731

    def prove(fid_, claim, taus, As, Bs, Cs, alphas, tr):
        def tr_m(coeffs):                                   # the stand-in transcript sees canonical coefficients
            ch = tr([un_m(c) for c in coeffs])
            return int(int.from_bytes(ch, "little") * Rm % p).to_bytes(32, "little")
        polys, rs, claims = prove_m(fid_, to_m(np.frombuffer(claim, np.uint8)).tobytes(), to_m(taus), [to_m(x) for x in As], [to_m(x) for x in Bs],
                                    [to_m(x) for x in Cs], to_m(alphas), tr_m)
        return [[un_m(c) for c in row] for row in polys], [un_m(r) for r in rs], [[un_m(c) for c in row] for row in claims]
    return prove
