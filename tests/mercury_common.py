"""Mercury's prover passes restated in Python integers, line by line after the reference (src/provider/mercury.rs) and deliberately NOT in
the closed form the kernels use (nova_amd/csrc/mercury.hpp): compute_h_poly (:369-386), divide_by_linear_polynomial (:281-288), expand,
transpose (:291-312), trim (:233-237), divide_by_binomial (:319-356), batch_add_with_polynomials (:239-261) and the quot_f block (:1163-1180).
The reference's own debug identities are the check functions at the end.  Polynomials are lists of integers mod p, low to high."""
import random

from oracle import pyref as R


class UniPoly:
    def __init__(self, coeffs, p):
        self.coeffs, self.p = list(coeffs), p

    def expand(self, size):                                     # resize with zeros, never shrinks
        if len(self.coeffs) < size:
            self.coeffs += [0] * (size - len(self.coeffs))

    def trim(self):                                             # :233-237
        while self.coeffs and self.coeffs[-1] == 0:
            self.coeffs.pop()

    def evaluate(self, x):
        acc = 0
        for c in reversed(self.coeffs):
            acc = (acc * x + c) % self.p
        return acc

    def divide_by_linear_polynomial(self, a):                   # :281-288: f(X) / (X - a), returns the remainder
        for i in reversed(range(len(self.coeffs) - 1)):
            last = self.coeffs[i + 1] * a % self.p
            self.coeffs[i] = (self.coeffs[i] + last) % self.p
        return self.coeffs.pop(0)

    def transpose(self, num_rows, num_cols, check_shape=True):  # :291-312
        if check_shape:
            assert num_rows <= num_cols
        b = num_cols
        self.expand(b * b)
        new = []
        for c in range(b):
            new += self.coeffs[c::b][:b]
        self.coeffs = new

    def batch_add_with_polynomials(self, polynomials, scalars):  # :239-261
        p = self.p
        rhs_max_len = max(len(q) for q in polynomials)
        self.expand(max(len(self.coeffs), rhs_max_len))
        for i in range(rhs_max_len):
            for rhs_poly, scalar in zip(polynomials, scalars):
                if i < len(rhs_poly):
                    rhs = rhs_poly[i]
                    if scalar == p - 1:
                        self.coeffs[i] = (self.coeffs[i] - rhs) % p
                    elif scalar != 0 and rhs != 0:
                        self.coeffs[i] = (self.coeffs[i] + scalar * rhs) % p


def compute_h_poly(p, f_poly, eq_col, num_rows, num_cols):      # :369-386
    return [sum(f_poly[row * num_cols + col] * eq_col[col] for col in range(num_cols)) % p for row in range(num_rows)]


def divide_by_binomial(p, coeffs, num_rows, num_cols, alpha):
    """:319-356 -> (quotient before trim(), remainder).  The reference's transpose pads to num_cols^2 and asserts num_rows <= num_cols; for
    shapes with more rows than columns (which the reference never calls with) the same column-major -> row-major step is taken over
    max(num_rows, num_cols) slots per column, which is what its expand / transpose pair does when it applies."""
    quotients, remainder = [], []
    width = max(num_cols, num_rows)
    for col_id in range(num_cols):
        quotient = UniPoly(coeffs[col_id::num_cols], p)
        assert len(quotient.coeffs) == num_rows
        remainder.append(quotient.divide_by_linear_polynomial(alpha))
        quotient.expand(width)
        quotients += quotient.coeffs
    if num_rows <= num_cols:
        q = UniPoly(quotients, p)
        q.transpose(num_rows, num_cols)
        return q.coeffs, remainder
    out = []                                                    # column c holds `width` slots: slot k of every column, k by k
    for k in range(width):
        out += [quotients[c * width + k] for c in range(num_cols)]
    return out, remainder


def q_in_abi_layout(q_untrimmed, num_rows, num_cols):
    """the (num_rows - 1) * num_cols elements nmx_mercury_divide_by_binomial writes: the reference's vector without its all-zero tail"""
    n = (num_rows - 1) * num_cols
    assert all(x == 0 for x in q_untrimmed[n:]), "the tail the ABI layout drops is not all zero"
    return q_untrimmed[:n]


def trimmed(p, coeffs):
    u = UniPoly(coeffs, p)
    u.trim()
    return u.coeffs


def quot_f(p, f_poly, q_coeffs, zeta, b, alpha, g_zeta):
    """:1163-1180 -> (quot_f coefficients, the remainder the reference asserts to be zero)"""
    zeta_b_alpha = (pow(zeta, b, p) - alpha) % p
    quot = UniPoly(f_poly, p)
    quot.batch_add_with_polynomials([q_coeffs], [(-zeta_b_alpha) % p])
    quot.coeffs[0] = (quot.coeffs[0] - g_zeta) % p
    rem = quot.divide_by_linear_polynomial(zeta)
    return quot.coeffs, rem


# ---- the reference's debug identities ---------------------------------------------------------------------------------------------
def dot(p, a, b):
    return sum(x * y for x, y in zip(a, b)) % p


def check_h_against_eval(p, eq_row, h, ev):                     # :972-984  <eq_row, h> = eval (h zero-padded to b)
    assert dot(p, eq_row, list(h) + [0] * (len(eq_row) - len(h))) == ev


def check_g_against_h_alpha(p, eq_col, g, h, alpha):            # :1053-1065  <eq_col, g> = h(alpha)
    assert dot(p, eq_col, g) == UniPoly(h, p).evaluate(alpha)


def check_division(p, f_poly, q, g, b, alpha, r):               # :1026-1042  f(r) = (r^b - alpha) q(r) + g(r)
    f_r, q_r, g_r = UniPoly(f_poly, p).evaluate(r), UniPoly(q, p).evaluate(r), UniPoly(g, p).evaluate(r)
    assert f_r == ((pow(r, b, p) - alpha) * q_r + g_r) % p


def check_quot_f(p, f_poly, q, quot, rem, zeta, b, alpha, g_zeta, r):   # :1177 rem == 0 and :1182-1199
    assert rem == 0
    f_r, q_r, quot_r = UniPoly(f_poly, p).evaluate(r), UniPoly(q, p).evaluate(r), UniPoly(quot, p).evaluate(r)
    assert quot_r * (r - zeta) % p == (f_r - (pow(zeta, b, p) - alpha) * q_r - g_zeta) % p


def restate(p, f_poly, num_rows, num_cols, eq_col, alpha):
    """-> (h, q in the ABI layout, g) with the division identity checked at a point of its own"""
    h = compute_h_poly(p, f_poly, eq_col, num_rows, num_cols)
    q_full, g = divide_by_binomial(p, f_poly, num_rows, num_cols, alpha)
    q = q_in_abi_layout(q_full, num_rows, num_cols)
    check_division(p, f_poly, q, g, num_cols, alpha, random.Random(len(f_poly)).randrange(p))
    check_g_against_h_alpha(p, eq_col, g, h, alpha)
    return h, q, g


def eq_evals(p, point):
    return R.eq_evals(p, list(point))
