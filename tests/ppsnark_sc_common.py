"""Shared checks for ppsnark's batched inner sum-check (RelaxedR1CSSNARK::prove_helper, src/spartan/ppsnark.rs:886-983):
one sum-check over sixteen tables for nine claims -- MemorySumcheckInstance (:520-670, claims 0-5), InnerBatchedSumcheckInstance
(:725-786, claims 6-7) and WitnessBoundSumcheck (:293-325, claim 8) -- batched by powers of one challenge.

The same drivers run against the host prover (CPU, tests/test_sumcheck_ppsnark_abi.py), the restatement below and the HIP path through the
C ABI (GPU, tests/test_gpu_sumcheck_ppsnark.py).  Two kinds of instance:
  make_random   sixteen independent tables: not satisfiable (the seven zero claims are false), so no verifier accepts it -- it pins a
                prover to py_prove, the reference restated line by line in Python integers, output for output;
  make_honest   a small true instance; check_honest is the reference's verifier (SumcheckProof::verify, sumcheck.rs:87-129, and the
                final-claim expression of ppsnark.rs:1566-1597), the sixteen final evaluations and, at small sizes, the DEFINITION of
                every round polynomial by brute force over the hypercube.
Everything is exact.  Table order: include/nova_mi355x.h NMX_PPS_*."""
import random

import numpy as np

from tests import fv_common as fc
from tests.batched_cubic_common import eq_table, zeroing_challenge  # noqa: F401  (zeroing_challenge: re-exported for the tests)
from tests.spartan_common import StandInTranscript, eq_eval, ints, le, mle_eval, poly_at, verify_rounds

(T_ROW, TINV_ROW, W_ROW, WINV_ROW, TS_ROW, T_COL, TINV_COL, W_COL, WINV_COL, TS_COL, L_ROW, L_COL, VAL, E, W, MASKED_EQ) = range(16)
NT = 16


# ---- the reference, restated ---------------------------------------------------------------------------------------------------------
class EqInst:
    """EqSumCheckInstance (sumcheck.rs:593-1253) in Python integers; the sqrt-size tables are spelled out as one table per round"""

    def __init__(self, p, taus):
        self.p, self.taus, self.eval_eq_left, self.round, self._fac = p, list(taus), 1, 1, (0, None)

    def consts(self):
        tau = self.taus[self.round - 1]
        eq_0, eq_slope = (1 - tau) % self.p, (2 * tau - 1) % self.p
        return eq_0, eq_slope, (eq_0 - eq_slope) % self.p

    def fac(self):
        # poly_eq_left[..][id >> s] * poly_eq_right[..][id & mask] (first half) / poly_eq_right[..][id] (last half): eq over taus[round ..]
        if self._fac[0] != self.round:
            self._fac = (self.round, eq_table(self.p, self.taus[self.round:]))
        return self._fac[1]

    def derive_deg2(self, t_0, t_inf, claim):
        """derive_from_claim_deg2 (:680-715); None when l(1) p has no inverse"""
        p, pl = self.p, self.eval_eq_left
        eq_0, eq_slope, eq_m1 = self.consts()
        l_0_p, l_1_p = eq_0 * pl % p, (eq_0 + eq_slope) * pl % p
        if l_1_p == 0:
            return None
        s_0 = l_0_p * t_0 % p
        t_1 = (claim - s_0) * pow(l_1_p, -1, p) % p
        t_m1 = (2 * t_inf + 2 * t_0 - t_1) % p
        return s_0, eq_slope * pl * t_inf % p, eq_m1 * pl * t_m1 % p

    def derive_deg1(self, t_0, claim):
        """derive_from_claim_deg1 (:720-747)"""
        p, pl = self.p, self.eval_eq_left
        eq_0, eq_slope, eq_m1 = self.consts()
        l_0_p, l_1_p = eq_0 * pl % p, (eq_0 + eq_slope) * pl % p
        if l_1_p == 0:
            return None
        s_0 = l_0_p * t_0 % p
        t_1 = (claim - s_0) * pow(l_1_p, -1, p) % p
        return s_0, 0, eq_m1 * pl * ((2 * t_0 - t_1) % p) % p

    def cubic(self, A, B, C, claim):
        """evaluation_points_cubic_with_three_inputs (:900-966; C given) / _with_two_inputs (:972-1033; C None: the constant ONE) with
        fallback_eval_inf_three_inputs / _two_inputs (:1085-1181)"""
        p, h, fac = self.p, len(A) // 2, self.fac()
        c = (lambda i: C[i]) if C is not None else (lambda i: 1)
        t_0 = sum((A[i] * B[i] - c(i)) * fac[i] for i in range(h)) % p
        t_inf = sum((A[i + h] - A[i]) * (B[i + h] - B[i]) * fac[i] for i in range(h)) % p
        got = self.derive_deg2(t_0, t_inf, claim)
        if got is not None:
            return got
        eq_0, eq_slope, eq_m1 = self.consts()
        cm1 = (lambda i: 2 * C[i] - C[i + h]) if C is not None else (lambda i: 1)
        t_m1 = sum(((2 * A[i] - A[i + h]) * (2 * B[i] - B[i + h]) - cm1(i)) * fac[i] for i in range(h)) % p
        pl = self.eval_eq_left
        return eq_0 * pl * t_0 % p, eq_slope * pl * t_inf % p, eq_m1 * pl * t_m1 % p

    def one_input(self, A, claim):
        """evaluation_points_quadratic_with_one_input (:1039-1080) with fallback_eval_inf_one_input (:1185-1222)"""
        p, h, fac = self.p, len(A) // 2, self.fac()
        t_0 = sum(A[i] * fac[i] for i in range(h)) % p
        got = self.derive_deg1(t_0, claim)
        if got is not None:
            return got
        eq_0, _slope, eq_m1 = self.consts()
        t_m1 = sum((2 * A[i] - A[i + h]) * fac[i] for i in range(h)) % p
        return eq_0 * self.eval_eq_left * t_0 % p, 0, eq_m1 * self.eval_eq_left * t_m1 % p

    def bound(self, r):
        tau = self.taus[self.round - 1]
        self.eval_eq_left = self.eval_eq_left * ((1 - tau - r + 2 * r * tau) % self.p) % self.p
        self.round += 1


def update_claim(p, claim, evals, r):
    """SumcheckProof::update_claim (sumcheck.rs:68-75)"""
    e0, c3, em1 = evals
    e1 = (claim - e0) % p
    half = pow(2, -1, p)
    a1, a2 = ((e1 - em1) * half - c3) % p, ((e1 + em1) * half - e0) % p
    return (e0 + r * (a1 + r * (a2 + r * c3))) % p


def points_linear(p, A, B):
    """compute_eval_points_linear (sumcheck.rs:356-379)"""
    h = len(A) // 2
    return (sum(A[i] - B[i] for i in range(h)) % p, 0, sum((2 * A[i] - A[i + h]) - (2 * B[i] - B[i + h]) for i in range(h)) % p)


def points_quadratic(p, A, B):
    """compute_eval_points_quadratic (sumcheck.rs:384-407)"""
    h = len(A) // 2
    return sum(A[i] * B[i] for i in range(h)) % p, 0, sum((2 * A[i] - A[i + h]) * (2 * B[i] - B[i + h]) for i in range(h)) % p


def points_cubic(p, A, B, C):
    """compute_eval_points_cubic (sumcheck.rs:416-443)"""
    h = len(A) // 2
    d = lambda X, i: X[i + h] - X[i]  # noqa: E731
    return (sum(A[i] * B[i] * C[i] for i in range(h)) % p, sum(d(A, i) * d(B, i) * d(C, i) for i in range(h)) % p,
            sum((A[i] - d(A, i)) * (B[i] - d(B, i)) * (C[i] - d(C, i)) for i in range(h)) % p)


def py_prove(fid, tables, rhos, r_outer, claims2, coeffs, tr):
    """prove_helper (ppsnark.rs:886-983) with the three instances' evaluation_points / bound (:307-320, :540-653, :741-778), line by line
    in Python integers: the CPU-side `prove`.  -> (polys [l][4], r [l], the sixteen tables at r) as 32-byte strings."""
    p = fc.FIELDS[fid]
    T = [ints(t) for t in tables]
    rho, ro = (ints(rhos) if len(rhos) else []), (ints(r_outer) if len(r_outer) else [])
    c2, co9 = ints(np.frombuffer(b"".join(claims2), np.uint8)), ints(np.frombuffer(b"".join(coeffs), np.uint8))
    l = len(rho)
    assert len(T) == NT and len(ro) == l and all(len(t) == 1 << l for t in T) and len(c2) == 2 and len(co9) == 9
    mem_eq, inner_eq = EqInst(p, rho), EqInst(p, ro)
    running = [0] * 6                         # MemorySumcheckInstance::running_claims (:514)
    running_E = c2[1]                         # InnerBatchedSumcheckInstance::running_claim_E (:719)
    claims = [0] * 6 + [c2[0], c2[1]] + [0]   # initial_claims chained (:913-918)
    e = sum(c * k for c, k in zip(claims, co9)) % p
    polys, rs = [], []
    for _ in range(l):
        mem = [points_linear(p, T[TINV_ROW], T[WINV_ROW]), points_linear(p, T[TINV_COL], T[WINV_COL]),
               mem_eq.cubic(T[TINV_ROW], T[T_ROW], T[TS_ROW], running[2]), mem_eq.cubic(T[WINV_ROW], T[W_ROW], None, running[3]),
               mem_eq.cubic(T[TINV_COL], T[T_COL], T[TS_COL], running[4]), mem_eq.cubic(T[WINV_COL], T[W_COL], None, running[5])]
        ev_E = inner_eq.one_input(T[E], running_E)
        inner = [points_cubic(p, T[L_ROW], T[L_COL], T[VAL]), (ev_E[0], 0, ev_E[2])]
        wit = [points_quadratic(p, T[MASKED_EQ], T[W])]
        evals = mem + inner + wit
        c0, lead, cm1 = (sum(ev[w] * k for ev, k in zip(evals, co9)) % p for w in range(3))
        s_1 = (e - c0) % p                    # UniPoly::from_evals_deg3([e0, e - e0, lead, em1]) (univariate.rs:103-113)
        q2 = ((s_1 + cm1) * pow(2, -1, p) - c0) % p
        co = [c0, (s_1 - lead - c0 - q2) % p, q2, lead]
        r = int.from_bytes(tr([le(c) for c in co]), "little")
        polys.append([le(c) for c in co])
        rs.append(le(r))
        running = [update_claim(p, running[i], mem[i], r) for i in range(6)]
        running_E = update_claim(p, running_E, ev_E, r)
        h = len(T[0]) // 2
        T = [[(t[i] + r * (t[i + h] - t[i])) % p for i in range(h)] for t in T]
        mem_eq.bound(r), inner_eq.bound(r)
        e = poly_at(p, co, r)
    return polys, rs, [le(t[0]) for t in T]


# ---- instances -----------------------------------------------------------------------------------------------------------------------
class Instance:
    def __init__(self, fid, l, tables, rhos, r_outer, claims2, coeffs):
        self.fid, self.l, self.p = fid, l, fc.FIELDS[fid]
        self.tables = tables                                  # sixteen (2^l, 32) uint8 arrays
        self.rhos, self.r_outer = fc.vec(rhos).copy() if l else np.zeros((0, 32), np.uint8), fc.vec(r_outer).copy() if l else np.zeros((0, 32), np.uint8)
        self.claims2, self.coeffs = [le(c) for c in claims2], [le(c) for c in coeffs]
        self.rho_i, self.ro_i, self.c2_i, self.co_i = list(rhos), list(r_outer), list(claims2), list(coeffs)

    def args(self):
        """what a `prove` takes after fid (fresh copies of the tables: provers bind in place)"""
        return [t.copy() for t in self.tables], self.rhos, self.r_outer, self.claims2, self.coeffs


def _scalars(fid, l, seed, rhos, r_outer):
    p = fc.FIELDS[fid]
    rng = random.Random(seed * 7919 + l)
    rho = [rng.randrange(p) for _ in range(l)] if rhos is None else list(rhos)
    ro = [rng.randrange(p) for _ in range(l)] if r_outer is None else list(r_outer)
    s = rng.randrange(1, p)
    return rng, rho, ro, [pow(s, i, p) for i in range(9)]    # powers(s, 9) (ppsnark.rs:920-921)


def make_random(fid, l, seed, rhos=None, r_outer=None, fill=None):
    """sixteen independent tables (fc.edge_vectors), random scalars and claims.  fill: every table entry AND every scalar is that value."""
    p = fc.FIELDS[fid]
    rng, rho, ro, coeffs = _scalars(fid, l, seed, rhos, r_outer)
    if fill is None:
        tables = [fc.edge_vectors(fid, 1 << l, seed + 13 * t) for t in range(NT)]
        claims2 = [rng.randrange(p), rng.randrange(p)]
    else:
        tables = [fc.vec([fill % p] * (1 << l)).copy() for _ in range(NT)]
        rho, ro, coeffs, claims2 = [fill % p] * l, [fill % p] * l, [fill % p] * 9, [fill % p] * 2
    return Instance(fid, l, tables, rho, ro, claims2, coeffs)


def make_honest(fid, l, seed, rhos=None, r_outer=None):
    """a true instance over 2^l entries: two memories of 2^l cells read at random addresses.  As compute_oracles does
    (ppsnark.rs:389-443): T = mem gamma + i, W = L gamma + addr, t_plus_r_inv = ts / (T + r), w_plus_r_inv = 1 / (W + r)."""
    p = fc.FIELDS[fid]
    n = 1 << l
    rng, rho, ro, coeffs = _scalars(fid, l, seed, rhos, r_outer)
    T = [None] * NT
    while True:
        gamma, r = rng.randrange(p), rng.randrange(p)
        ok = True
        for g in (0, 1):
            mem = [rng.randrange(p) for _ in range(n)]
            addr = [rng.randrange(n) for _ in range(n)]
            L = [mem[a] for a in addr]
            ts = [0] * n
            for a in addr:
                ts[a] += 1
            tpr = [(mem[i] * gamma + i + r) % p for i in range(n)]
            wpr = [(L[i] * gamma + addr[i] + r) % p for i in range(n)]
            if 0 in tpr or 0 in wpr:
                ok = False
                break
            T[5 * g + T_ROW], T[5 * g + W_ROW], T[5 * g + TS_ROW] = tpr, wpr, ts
            T[5 * g + TINV_ROW] = [ts[i] * pow(tpr[i], -1, p) % p for i in range(n)]
            T[5 * g + WINV_ROW] = [pow(x, -1, p) for x in wpr]
            T[L_ROW + g] = L
        if ok:
            break
    T[VAL] = [rng.randrange(p) for _ in range(n)]
    T[E] = [rng.randrange(p) for _ in range(n)]
    m = l // 2                                                 # W is zero from 2^m on; the masked eq is zero below 2^m
    T[W] = [rng.randrange(p) if i < (1 << m) else 0 for i in range(n)]
    eqo = eq_table(p, ro)
    T[MASKED_EQ] = [0 if i < (1 << m) else eqo[i] for i in range(n)]
    claim_ABC = sum(a * b * c for a, b, c in zip(T[L_ROW], T[L_COL], T[VAL])) % p
    claim_E = sum(x * y for x, y in zip(eqo, T[E])) % p
    return Instance(fid, l, [fc.vec(t).copy() for t in T], rho, ro, [claim_ABC, claim_E], coeffs)


# ---- checks --------------------------------------------------------------------------------------------------------------------------
def run(prove, inst, force=None):
    """-> (polys, rs, finals) as the prover returned them; the transcript must have received exactly the returned polynomials"""
    tr = StandInTranscript(inst.p, force=force)
    polys, rs, finals = prove(inst.fid, *inst.args(), tr)
    polys_i = [[int.from_bytes(c, "little") for c in row] for row in polys]
    rs_i = [int.from_bytes(x, "little") for x in rs]
    assert len(polys_i) == inst.l and all(len(row) == 4 for row in polys_i) and len(finals) == NT
    assert polys_i == tr.polys and rs_i == tr.rs, "the prover must hand the transcript exactly what it returns"
    return polys, rs, finals


def summand(inst, Ti, pt):
    """the nine weighted summands at a point: what the batched sum-check sums over the hypercube"""
    p, co = inst.p, inst.co_i
    v = [mle_eval(p, t, pt) for t in Ti]
    eq_rho, eq_ro = eq_eval(p, inst.rho_i, pt), eq_eval(p, inst.ro_i, pt)
    return (co[0] * (v[TINV_ROW] - v[WINV_ROW]) + co[1] * (v[TINV_COL] - v[WINV_COL])
            + co[2] * eq_rho * (v[TINV_ROW] * v[T_ROW] - v[TS_ROW]) + co[3] * eq_rho * (v[WINV_ROW] * v[W_ROW] - 1)
            + co[4] * eq_rho * (v[TINV_COL] * v[T_COL] - v[TS_COL]) + co[5] * eq_rho * (v[WINV_COL] * v[W_COL] - 1)
            + co[6] * v[L_ROW] * v[L_COL] * v[VAL] + co[7] * eq_ro * v[E] + co[8] * v[MASKED_EQ] * v[W]) % p


def check_honest(prove, inst, force=None, brute=None):
    p, l = inst.p, inst.l
    polys, rs, finals = run(prove, inst, force)
    polys_i = [[int.from_bytes(c, "little") for c in row] for row in polys]
    rs_i = [int.from_bytes(x, "little") for x in rs]
    Ti = [ints(t) for t in inst.tables]
    fin = [int.from_bytes(f, "little") for f in finals]
    want = [mle_eval(p, t, rs_i) for t in Ti]
    assert fin == want, "every one of the sixteen finals is its table at r"
    e = verify_rounds(p, inst.co_i[6] * inst.c2_i[0] + inst.co_i[7] * inst.c2_i[1], polys_i, rs_i, 3)
    co, eq_rho, eq_ro = inst.co_i, eq_eval(p, inst.rho_i, rs_i), eq_eval(p, inst.ro_i, rs_i)
    tpr_row, wpr_row, tpr_col, wpr_col = want[T_ROW], want[W_ROW], want[T_COL], want[W_COL]    # t_plus_r / w_plus_r: the original tables at r
    expected = (co[0] * (fin[TINV_ROW] - fin[WINV_ROW]) + co[1] * (fin[TINV_COL] - fin[WINV_COL])
                + co[2] * eq_rho * (fin[TINV_ROW] * tpr_row - fin[TS_ROW]) + co[3] * eq_rho * (fin[WINV_ROW] * wpr_row - 1)
                + co[4] * eq_rho * (fin[TINV_COL] * tpr_col - fin[TS_COL]) + co[5] * eq_rho * (fin[WINV_COL] * wpr_col - 1)
                + co[6] * fin[L_ROW] * fin[L_COL] * fin[VAL] + co[7] * eq_ro * fin[E] + co[8] * fin[MASKED_EQ] * fin[W]) % p
    assert e == expected, "ppsnark.rs:1566-1597: the final claim"
    if brute if brute is not None else l <= 4:
        for j in range(l):
            rest = l - j - 1
            for x in (0, 1, 2, p - 1):
                tot = sum(summand(inst, Ti, rs_i[:j] + [x] + [(y >> (rest - 1 - t)) & 1 for t in range(rest)]) for y in range(1 << rest)) % p
                assert poly_at(p, polys_i[j], x) == tot, (j, x)
    return polys, rs, finals


def montgomery_wrapped(prove_m, fid):
    """a prover that takes and returns halo2curves Montgomery words (x 2^256), behind the canonical interface of run / check_honest"""
    p = fc.FIELDS[fid]
    Rm = 1 << 256
    to_m = lambda v: fc.vec([x * Rm % p for x in ints(v)]).copy() if len(v) else v  # noqa: E731
    un_m = lambda b: int(int.from_bytes(b, "little") * pow(Rm, -1, p) % p).to_bytes(32, "little")  # noqa: E731
    lst_m = lambda bs: [le(int.from_bytes(b, "little") * Rm % p) for b in bs]  # noqa: E731

    def prove(fid_, tables, rhos, r_outer, claims2, coeffs, tr):
        def tr_m(co):                                         # the stand-in transcript sees canonical coefficients
            ch = tr([un_m(c) for c in co])
            return int(int.from_bytes(ch, "little") * Rm % p).to_bytes(32, "little")
        polys, rs, finals = prove_m(fid_, [to_m(t) for t in tables], to_m(rhos), to_m(r_outer), lst_m(claims2), lst_m(coeffs), tr_m)
        return [[un_m(c) for c in row] for row in polys], [un_m(r) for r in rs], [un_m(f) for f in finals]
    return prove
