"""The yardstick of nmx_field_gather and nmx_ppsnark_mem_oracles: the definitions restated in Python integers.

  gather       R1CSShapeSparkRepr::evaluation_oracles (src/spartan/ppsnark.rs:220-253):  out[i] = mem[addr[i]]
  mem_oracles  MemorySumcheckInstance::compute_oracles (ppsnark.rs:371-489) without its commitments, per memory:
                   t_plus_r[i] = mem[i] gamma + i + r            t_plus_r_inv[i] = ts[i] / t_plus_r[i]
                   w_plus_r[i] = L[i] gamma + addr[i] + r        w_plus_r_inv[i] = 1 / w_plus_r[i]
               (tests/ppsnark_sc_common.make_honest writes the same formulas to build its honest instance)
Values are canonical integers here; the Montgomery form (x 2^256) is applied to whole operand sets by to_form / from_form."""
import random

from tests import fv_common as fc

R256 = 1 << 256


class ZeroDenominator(Exception):
    """some T + r or W + r is zero: the reference's batch_invert(..)? fails (ppsnark.rs:430)"""


def gather(mem, addr):
    return [mem[a] for a in addr]


def inverses(p, xs):
    """1 / x for every x (none zero).  One modular inversion for the whole list (prefix products) instead of one each -- pow(x, -1, p) costs
    ~50 us, which at 2^14 elements and eight memories is a quarter of a minute -- and every result is CHECKED against the definition of an
    inverse, x y = 1 mod p, so nothing rests on the shortcut."""
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % p
    inv, out = pow(acc, -1, p), [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % p
        inv = inv * xs[i] % p
    assert all(x * y % p == 1 for x, y in zip(xs, out))
    return out


def oracles_one(p, mem, addr, L, ts, gamma, r):
    n = len(mem)
    assert len(addr) == len(L) == len(ts) == n
    tpr = [(mem[i] * gamma + i + r) % p for i in range(n)]
    wpr = [(L[i] * gamma + addr[i] + r) % p for i in range(n)]
    if 0 in tpr or 0 in wpr:
        raise ZeroDenominator()
    inv = inverses(p, tpr + wpr)
    return tpr, wpr, [ts[i] * inv[i] % p for i in range(n)], inv[n:]


def oracles(p, mems, addrs, Ls, tss, gamma, r):
    """per memory (t_plus_r, w_plus_r, t_plus_r_inv, w_plus_r_inv), in the order the call returns them"""
    return [oracles_one(p, m, a, L, t, gamma, r) for m, a, L, t in zip(mems, addrs, Ls, tss)]


def to_form(p, v, mont):
    return [x * R256 % p for x in v] if mont else list(v)


def from_form(p, v, mont):
    inv = pow(R256, -1, p)
    return [x * inv % p for x in v] if mont else list(v)


class Case:
    """k memories of n cells: mems, addrs (integers below n), Ls = the gathers, tss, gamma, r -- all canonical integers"""

    def __init__(self, fid, k, n, mems, addrs, tss, gamma, r, Ls=None):
        self.fid, self.p, self.k, self.n = fid, fc.FIELDS[fid], k, n
        self.mems, self.addrs, self.tss, self.gamma, self.r = mems, addrs, tss, gamma, r
        self.Ls = Ls if Ls is not None else [gather(m, a) for m, a in zip(mems, addrs)]

    def want(self):
        return oracles(self.p, self.mems, self.addrs, self.Ls, self.tss, self.gamma, self.r)


def trace_counts(addr, n):
    ts = [0] * n
    for a in addr:
        ts[a] += 1
    return ts


def random_case(fid, k, n, seed):
    """random memories read at random addresses, ts the read counts of the trace; gamma and r are drawn until no denominator is zero (with
    random gamma and r the first draw does)"""
    p = fc.FIELDS[fid]
    rng = random.Random(1000003 * seed + 8191 * k + n)
    mems = [[rng.randrange(p) for _ in range(n)] for _ in range(k)]
    addrs = [[rng.randrange(n) for _ in range(n)] for _ in range(k)]
    tss = [trace_counts(a, n) for a in addrs]
    while True:
        c = Case(fid, k, n, mems, addrs, tss, rng.randrange(p), rng.randrange(p))
        try:
            c.want()
            return c
        except ZeroDenominator:
            continue


def edge_cases(fid, k, n, seed):
    """the edge contents: mem entries 0 and p - 1, ts entries 0 and n, and gamma = 0, gamma = p - 1, r = 0 in turn (the other scalar random).
    None has a zero denominator:
      gamma = 0:      T + r = i + r and W + r = addr + r with i, addr < n: non-zero for r in [1, p - n];
      gamma = p - 1:  T + r = i - mem + r, W + r = addr - L + r: r is redrawn until the reference accepts (a random r does);
      r = 0:          T = mem gamma + i, W = L gamma + addr: T[0] = mem[0] gamma, so THIS case has mem[0] = 1 where the others have 0 (its
                      zero entry moves to cell 1 when there is one); gamma is redrawn likewise."""
    p = fc.FIELDS[fid]
    rng = random.Random(7 * seed + 31 * k + n)
    mems = [[rng.randrange(p) for _ in range(n)] for _ in range(k)]
    addrs = [[rng.randrange(n) for _ in range(n)] for _ in range(k)]
    for m in range(k):
        mems[m][0] = 0
        mems[m][n - 1] = p - 1 if n > 1 else 0
        addrs[m][0] = n - 1                      # the last cell is read at least once, and (below) one cell n times in the last memory
    addrs[k - 1] = [n // 2] * n                  # every address equal: ts has one entry n and n - 1 entries 0
    tss = [trace_counts(a, n) for a in addrs]
    out = []
    for gamma, r in ((0, None), (p - 1, None), (None, 0)):
        while True:
            g = rng.randrange(p) if gamma is None else gamma
            rr = rng.randrange(1, p - n) if r is None else r
            ms = mems
            if r == 0:
                ms = [[1] + ([0] if n > 2 else []) + list(m[(2 if n > 2 else 1):]) for m in mems]
            c = Case(fid, k, n, ms, addrs, tss, g, rr)
            try:
                c.want()
                out.append(c)
                break
            except ZeroDenominator:
                continue
    return out
