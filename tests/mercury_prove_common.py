"""The yardstick of the Mercury prover tests: EvaluationEngineTrait::prove (src/provider/mercury.rs:891-1268) with make_s_polynomial
(:391-475, in the reference's FFT form) and generate_batch_evaluate_arg (:567-770), and ::verify (:1270-1486 with
extract_pairing_to_verify_batch_evaluation, :773-871) restated line by line in Python integers over tests/mercury_common.py and
oracle/pyref.  The transcript is tests/hyperkzg_common.Sha3Transcript in the shape of nmx_transcript_fn_kzg, driven with the seven stages
of nmx_mercury_prove.

The key is made from a KNOWN tau (ck[i] = tau^i G), so
  * commit(f) = f(tau) G -- one scalar multiplication instead of an MSM, and
  * each pairing equation e(L, g2) == e(R, tau_H) is L == tau R in G1.
Nothing here touches the library, and nothing here uses the correlation form the kernel computes except s_definition, which
tests/test_mercury_prove_abi.py checks against the FFT form on the three fields that have the roots of unity."""
from oracle import pyref as R
from tests import mercury_common as MC
from tests.hyperkzg_common import Sha3Transcript, commit_tau  # noqa: F401  (re-exported for the tests)


# ---- make_s_polynomial ---------------------------------------------------------------------------------------------------------------
def root_of_unity(p, order):
    """a primitive `order`-th root (order a power of two) as x^((p - 1) / order) for x = 2, 3, 5, ... until w^(order / 2) == p - 1;
    None when order does not divide p - 1 (BN254 Fq: p - 1 = 2 * odd)"""
    if (p - 1) % order:
        return None
    for x in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        w = pow(x, (p - 1) // order, p)
        if pow(w, order // 2, p) == p - 1:
            return w
    raise AssertionError("no generator among the small primes")


def fft(p, a, omega):
    """best_fft: [sum_j a[j] omega^(i j) for i] (the definition; the sizes here are tiny)"""
    n = len(a)
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * omega % p
    return [sum(a[j] * pw[i * j % n] for j in range(n)) % p for i in range(n)]


def make_s_polynomial_fft(p, a_polys, b_polys, log_b, gamma):
    """:391-475, line by line.  Raises IndexError-like AssertionError where the reference's drain(..b) panics (the trimmed result shorter
    than b) -- callers that want the wider corner take s_definition."""
    b = 1 << log_b
    b2 = b * 2
    omega = root_of_unity(p, b2)
    assert omega is not None, "this field has no root of unity of order 2b"
    (a1, a2), (b1, b2_) = a_polys, b_polys
    assert len(a1) == len(a2) == len(b1) == len(b2_) == b
    ev = [fft(p, list(v) + [0] * b, omega) for v in (a1, a2, b1, b2_)]                       # :410-428
    a_e1, a_e2, b_e1, b_e2 = ev
    evals = [0] * b2
    evals[0] = (a_e1[0] * b_e1[0] + a_e2[0] * b_e2[0] * gamma) % p                            # :435-436
    evals[0] = (evals[0] + evals[0]) % p
    for i in range(1, b2):                                                                    # :438-444
        s1 = a_e1[i] * b_e1[b2 - i] + a_e1[b2 - i] * b_e1[i]
        s2 = a_e2[i] * b_e2[b2 - i] + a_e2[b2 - i] * b_e2[i]
        evals[i] = (s1 + s2 * gamma) % p
    omega_n_1 = pow(omega, b - 1, p)                                                          # :448-455
    omega_pow = omega_n_1
    for i in range(1, b2):
        evals[i] = evals[i] * omega_pow % p
        omega_pow = omega_pow * omega_n_1 % p
    res = MC.UniPoly(fft(p, evals, pow(omega, -1, p)), p)                                     # :458-468
    res.trim()
    b_inv = pow(b2, -1, p)
    res.coeffs = [x * b_inv % p for x in res.coeffs]
    assert len(res.coeffs) < b2                                                               # :470
    assert len(res.coeffs) >= b, "drain(..b) panics: the trimmed result has fewer than b coefficients"
    return res.coeffs[b:]                                                                     # :472


def s_definition(p, a1, b1, a2, b2, gamma):
    """nmx_mercury_s_poly's definition: b - 1 coefficients, untrimmed; words are read mod p"""
    a1, b1, a2, b2 = ([x % p for x in v] for v in (a1, b1, a2, b2))
    b = len(a1)
    return [(sum(a1[i + k + 1] * b1[i] + a1[i] * b1[i + k + 1] for i in range(b - 1 - k))
             + gamma * sum(a2[i + k + 1] * b2[i] + a2[i] * b2[i + k + 1] for i in range(b - 1 - k))) % p for k in range(b - 1)]


def make_s(p, a_polys, b_polys, log_b, gamma):
    """the FFT form where the field has the root and the reference does not panic, the definition elsewhere; always b - 1 coefficients"""
    b = 1 << log_b
    want = s_definition(p, a_polys[0], b_polys[0], a_polys[1], b_polys[1], gamma)
    if root_of_unity(p, 2 * b) is not None and any(want):
        got = make_s_polynomial_fft(p, a_polys, b_polys, log_b, gamma)
        assert got == MC.trimmed(p, want), "the FFT form and the correlation differ"
    return want


# ---- UniPoly helpers of the batch opening -----------------------------------------------------------------------------------------
def from_evals_with_xs(p, xs, evals):
    """:205-: the Vandermonde system solved by Gaussian elimination; ZeroDivisionError-like ValueError when two xs coincide"""
    if len(evals) == 1:
        return [evals[0] % p]
    n = len(evals)
    m = [[pow(x, j, p) for j in range(n)] + [e % p] for x, e in zip(xs, evals)]
    for i in range(n):
        piv = next((r for r in range(i, n) if m[r][i]), None)
        if piv is None:
            raise ValueError("singular interpolation system")
        m[i], m[piv] = m[piv], m[i]
        inv = pow(m[i][i], -1, p)
        m[i] = [v * inv % p for v in m[i]]
        for r in range(n):
            if r != i and m[r][i]:
                f = m[r][i]
                m[r] = [(v - f * w) % p for v, w in zip(m[r], m[i])]
    return [m[i][n] for i in range(n)]


def multiply_by_linear_polynomial(p, coeffs, a):                                              # :264-276: f (X + a)
    a_f = [c * a % p for c in coeffs]
    out = [0] + list(coeffs)
    for i, rhs in enumerate(a_f):
        out[i] = (out[i] + rhs) % p
    return out


class Challenges:
    """alpha, gamma, zeta, beta, z as squeezed; `force` = {stage: value} replaces a squeezed value (edge challenges) -- the transcript still
    absorbs everything, so prover and verifier stay aligned when both are given the same `force`"""

    def __init__(self, tr, force=None):
        self.tr, self.force = tr, dict(force or {})

    def points(self, stage, pts):
        ch = self.tr.decode(self.tr.stage(stage, b"".join(R.point_to_xy64(P) for P in pts), len(pts), bytes(int(P is None) for P in pts)))
        return self.force.get(stage, ch)

    def scalars(self, stage, vals):
        self.tr.stage(stage, b"".join(self.tr.encode(v) for v in vals), len(vals), None)


def generate_batch_evaluate_arg(p, commit, ev, polys, beta, squeeze_z):
    """:567-770 from the squeeze of beta on.  commit(coefficients) -> a commitment; ev: dict of the eight evaluations and zeta, zeta_inv,
    alpha; polys = (g, h, s, d); squeeze_z(comm_w) -> z.  -> (comm_w, comm_w_prime, W, W')"""
    zeta, zeta_inv, alpha = ev["zeta"], ev["zeta_inv"], ev["alpha"]
    beta_2, beta_3 = beta * beta % p, beta * beta * beta % p
    stars = [from_evals_with_xs(p, [zeta, zeta_inv], [ev["g_zeta"], ev["g_zeta_inv"]]),      # :592-614
             from_evals_with_xs(p, [zeta, zeta_inv, alpha], [ev["h_zeta"], ev["h_zeta_inv"], ev["h_alpha"]]),
             from_evals_with_xs(p, [zeta, zeta_inv], [ev["s_zeta"], ev["s_zeta_inv"]]),
             from_evals_with_xs(p, [zeta], [ev["d_zeta"]])]
    work = [MC.UniPoly(f, p) for f in polys]                                                  # :626-642
    for poly, rhs in zip(work, stars):
        poly.batch_add_with_polynomials([rhs], [p - 1])
    for poly, vanishing in zip(work, ([alpha], [], [alpha], [alpha, zeta_inv])):              # :644-653
        for pt in vanishing:
            poly.coeffs = multiply_by_linear_polynomial(p, poly.coeffs, (-pt) % p)
    m_poly = work[0]                                                                          # :655-664
    m_poly.batch_add_with_polynomials([work[1].coeffs, work[2].coeffs, work[3].coeffs], [beta, beta_2, beta_3])
    quot_m = m_poly                                                                           # :668-674
    for pt in (alpha, zeta, zeta_inv):
        assert quot_m.divide_by_linear_polynomial(pt) == 0
    W = list(quot_m.coeffs)
    comm_w = commit(W)                                                                        # :677
    z = squeeze_z(comm_w)                                                                     # :678-682
    t_s1 = (z - alpha) % p                                                                    # :688-692
    t_s4 = t_s1 * (z - zeta_inv) % p
    t = t_s4 * (z - zeta) % p
    star_eval = [MC.UniPoly(s_, p).evaluate(z) for s_ in stars]                               # :703-706
    shifted = []
    for f, se in zip(polys, star_eval):                                                       # :708-720
        u = list(f)
        u[0] = (u[0] - se) % p
        shifted.append(u)
    scalars = [t_s1, beta % p, t_s1 * beta_2 % p, t_s4 * beta_3 % p]                          # :725-730
    mz = MC.UniPoly([x * scalars[0] % p for x in shifted[0]], p)                              # :732-738
    mz.batch_add_with_polynomials(shifted[1:], scalars[1:])
    mz.batch_add_with_polynomials([W], [(-t) % p])                                            # :744-750
    assert mz.divide_by_linear_polynomial(z) == 0                                             # :754-761
    Wp = list(mz.coeffs)
    return comm_w, commit(Wp), W, Wp


# ---- prove ------------------------------------------------------------------------------------------------------------------------
COMM_NAMES = ("comm_h", "comm_g", "comm_q", "comm_s", "comm_d", "comm_quot_f", "comm_w", "comm_w_prime")
EVAL_NAMES = ("g_zeta", "g_zeta_inv", "h_zeta", "h_zeta_inv", "s_zeta", "s_zeta_inv")


def prove(c, tau, poly, point, tr, force=None):
    """-> (comms: the eight points in the order of COMM_NAMES (None = the identity), evals: the six integers of EVAL_NAMES, trace: a dict of
    the intermediate polynomials and challenges).  The caller's transcript has absorbed f, u and e (:905-907) already."""
    p = c.r
    ch = Challenges(tr, force)
    original_size = len(poly)
    log_n = len(point)                                                                        # :911-928
    assert log_n > 1 and original_size == 1 << log_n
    point, f_poly = list(point), list(poly)
    if log_n % 2 == 1:
        log_n += 1
        point.insert(0, 0)
        f_poly += [0] * ((1 << log_n) - len(f_poly))
    log_b = log_n // 2
    b = 1 << log_b
    b_row = original_size // b                                                                # :931
    u_row, u_col = point[:log_b], point[log_b:]                                               # :933-938
    eq_row, eq_col = MC.eq_evals(p, u_row), MC.eq_evals(p, u_col)
    h = MC.compute_h_poly(p, f_poly, eq_col, b_row, b)                                        # :966-970
    h += [0] * (b - len(h))
    comm_h = commit_tau(c, tau, h)                                                            # :987
    alpha = ch.points(0, [comm_h])                                                            # :988-991
    q_full, g = MC.divide_by_binomial(p, f_poly[:original_size], b_row, b, alpha)             # :995
    q = MC.trimmed(p, q_full)
    assert len(g) == b
    comm_q, comm_g = commit_tau(c, tau, q), commit_tau(c, tau, g)                             # :1046-1049
    gamma = ch.points(1, [comm_q, comm_g])                                                    # :1050-1051, :1068
    s = make_s(p, (eq_col, eq_row), (g, h), log_b, gamma)                                     # :1072-1077
    d = list(reversed(g))                                                                     # :1113-1120
    comm_s, comm_d = commit_tau(c, tau, s), commit_tau(c, tau, d)                             # :1123-1126
    zeta = ch.points(2, [comm_s, comm_d])                                                     # :1128-1132
    if zeta == 0:
        raise ZeroDivisionError("zeta.invert().unwrap()")
    zeta_inv = pow(zeta, -1, p)                                                               # :1134
    E = lambda f, x: MC.UniPoly(f, p).evaluate(x)  # noqa: E731                                 :1136-1159
    ev = {"g_zeta": E(g, zeta), "g_zeta_inv": E(g, zeta_inv), "h_zeta": E(h, zeta), "h_zeta_inv": E(h, zeta_inv), "h_alpha": E(h, alpha),
          "s_zeta": E(s, zeta), "s_zeta_inv": E(s, zeta_inv), "d_zeta": E(d, zeta), "zeta": zeta, "zeta_inv": zeta_inv, "alpha": alpha}
    quot_f, rem = MC.quot_f(p, f_poly[:original_size], q, zeta, b, alpha, ev["g_zeta"])        # :1163-1180
    assert rem == 0
    evals = [ev[k] for k in EVAL_NAMES]
    ch.scalars(3, evals)                                                                      # :1203-1208
    comm_quot_f = commit_tau(c, tau, MC.trimmed(p, quot_f[:original_size]))                   # :1212-1217
    beta = ch.points(4, [comm_quot_f])                                                        # :1218, :586
    comm_w, comm_w_prime, W, Wp = generate_batch_evaluate_arg(p, lambda f_: commit_tau(c, tau, f_), ev, (g, h, s, d), beta, lambda cw: ch.points(5, [cw]))
    ch.points(6, [comm_w_prime])                                                              # :1249-1250
    comms = [comm_h, comm_g, comm_q, comm_s, comm_d, comm_quot_f, comm_w, comm_w_prime]
    trace = dict(ev, h=h, q=q, g=g, s=s, d=d, quot_f=quot_f, W=W, W_prime=Wp, gamma=gamma, beta=beta, b=b, b_row=b_row, eq_row=eq_row, eq_col=eq_col)
    return comms, evals, trace


# ---- verify -----------------------------------------------------------------------------------------------------------------------
def eval_pu_poly(p, u, x):
    """the univariate whose coefficients are EqPolynomial::new(u).evals(), at x: prod_i (1 - u_i + u_i x^(2^(len - 1 - i)))"""
    return MC.UniPoly(MC.eq_evals(p, list(u)), p).evaluate(x)


def verify(c, tau, comm_f, point, ev_claim, comms, evals, tr, force=None, prover_trace=None):
    """:1270-1486 with each pairing equation replaced by L == tau R.  -> (pair 1 holds, pair 2 holds, the combination with d holds).  With
    prover_trace the implicit d_zeta and h_alpha (:1358-1369) are compared with the prover's values (AssertionError on a difference)."""
    p = c.r
    G = (c.gx, c.gy)
    comm_h, comm_g, comm_q, comm_s, comm_d, comm_quot_f, comm_w, comm_w_prime = comms
    g_zeta, g_zeta_inv, h_zeta, h_zeta_inv, s_zeta, s_zeta_inv = evals
    ch = Challenges(tr, force)
    alpha = ch.points(0, [comm_h])                                                            # :1283-1325
    gamma = ch.points(1, [comm_q, comm_g])
    zeta = ch.points(2, [comm_s, comm_d])
    ch.scalars(3, list(evals))
    beta = ch.points(4, [comm_quot_f])
    point = list(point)                                                                       # :1327-1343
    if len(point) % 2 == 1:
        point.insert(0, 0)
    log_n = len(point)
    u_row = point[:log_n // 2]
    u_col = point[log_n - len(u_row):]
    zeta_inv = pow(zeta, -1, p)                                                               # :1345-1352
    zeta_b_one = pow(zeta, (1 << (log_n // 2)) - 1, p)
    pu_col_zeta, pu_col_zeta_inv = eval_pu_poly(p, u_col, zeta), eval_pu_poly(p, u_col, zeta_inv)
    pu_row_zeta, pu_row_zeta_inv = eval_pu_poly(p, u_row, zeta), eval_pu_poly(p, u_row, zeta_inv)
    d_zeta = zeta_b_one * g_zeta_inv % p                                                      # :1358
    denom = (g_zeta * pu_col_zeta_inv + g_zeta_inv * pu_col_zeta                              # :1361-1369
             + gamma * (h_zeta * pu_row_zeta_inv + h_zeta_inv * pu_row_zeta - ev_claim - ev_claim) - zeta * s_zeta - zeta_inv * s_zeta_inv) % p
    h_alpha = denom * pow(2, -1, p) % p
    if prover_trace is not None:
        assert (d_zeta, h_alpha) == (prover_trace["d_zeta"], prover_trace["h_alpha"]), "the implicit d_zeta / h_alpha differ from the prover's"
    mul, add = (lambda k, P: R.mul(c, k % p, P)), (lambda P, Q: R.add(c, P, Q))
    zeta_b_alpha = (zeta_b_one * zeta - alpha) % p                                            # :1414-1438
    ll1 = add(comm_f, add(add(mul(-zeta_b_alpha, comm_q), mul(-g_zeta, G)), mul(zeta, comm_quot_f)))
    rl1 = comm_quot_f
    # extract_pairing_to_verify_batch_evaluation (:773-871); its beta is the one squeezed above, then it absorbs comm_w and squeezes z
    beta_2, beta_3 = beta * beta % p, beta * beta * beta % p
    z = ch.points(5, [comm_w])
    stars = [from_evals_with_xs(p, [zeta, zeta_inv], [g_zeta, g_zeta_inv]), from_evals_with_xs(p, [zeta, zeta_inv, alpha], [h_zeta, h_zeta_inv, h_alpha]),
             from_evals_with_xs(p, [zeta, zeta_inv], [s_zeta, s_zeta_inv]), from_evals_with_xs(p, [zeta], [d_zeta])]
    g_se, h_se, s_se, d_se = (MC.UniPoly(s_, p).evaluate(z) for s_ in stars)
    van_zeta, van_zeta_inv, van_alpha = (z - zeta) % p, (z - zeta_inv) % p, (z - alpha) % p
    t1, t2, t3, t4 = van_alpha, 1, van_alpha, van_zeta_inv * van_alpha % p
    t = t4 * van_zeta % p
    scalar = (t1 * g_se + beta * t2 * h_se + beta_2 * t3 * s_se + beta_3 * t4 * d_se) % p
    scalars = [t1, beta * t2, beta_2 * t3, beta_3 * t4, -scalar, -t, z]                       # :831-846
    bases = [comm_g, comm_h, comm_s, comm_d, G, comm_w, comm_w_prime]                         # :848-856
    ll2 = None
    for k, B in zip(scalars, bases):
        ll2 = add(ll2, mul(k, B))
    rl2 = comm_w_prime                                                                        # :868
    d = ch.points(6, [comm_w_prime])                                                          # :1469-1470
    ll, rl = add(ll1, mul(d, ll2)), add(rl1, mul(d, rl2))                                     # :1473-1474
    return ll1 == mul(tau, rl1), ll2 == mul(tau, rl2), ll == mul(tau, rl)
