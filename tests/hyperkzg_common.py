"""The yardstick of the HyperKZG tests: EvaluationEngineTrait::prove (src/provider/hyperkzg.rs:926-1116) and ::verify up to the pairing
(:1119-1230) restated in Python integers over oracle/pyref, a SHA3 transcript in the shape of nmx_transcript_fn_kzg, and the big-integer
definition of the batched multi-point quotients (nmx_poly_lincomb_quotients).

The key is made from a KNOWN tau (ck[i] = tau^i G, hyperkzg.rs:357-410), so
  * commit(f) = f(tau) G -- one scalar multiplication instead of an MSM, and
  * the pairing equation e(L, H) == e(R, tau_H) (:1232-1240) is L == tau R in G1.
Nothing here touches the library: tests/test_hyperkzg_abi.py checks this restatement on the reference's own known answers."""
import hashlib

from oracle import pyref as R


def le32(x):
    return int(x).to_bytes(32, "little")


def num(b):
    return int.from_bytes(bytes(b), "little")


class Sha3Transcript:
    """stage(stage, data, count, is_inf) -> 32 challenge bytes: absorbs exactly the bytes the callback is handed (stage 0: the commitments
    and their identity bytes, stage 1: the scalars of v, stage 2: the three w) and squeezes SHA3-256 of the state reduced mod p -- canonical
    bytes, or Montgomery limbs (x 2^256 mod p) with mont=True, the form NMX_SCALARS_MONT names.  `calls` records what was absorbed."""

    def __init__(self, p, seed=b"hyperkzg", mont=False):
        self.p, self.mont = p, mont
        self.state = hashlib.sha3_256(seed).digest()
        self.calls = []

    def encode(self, x):
        return le32(x * (1 << 256) % self.p if self.mont else x)

    def decode(self, b):
        return num(b) * pow(1 << 256, -1, self.p) % self.p if self.mont else num(b)

    def stage(self, stage, data, count, is_inf):
        self.calls.append((int(stage), bytes(data), int(count), None if is_inf is None else bytes(is_inf)))
        h = hashlib.sha3_256(self.state + bytes([stage]) + int(count).to_bytes(8, "little") + bytes(data))
        if is_inf is not None:
            h.update(b"inf" + bytes(is_inf))
        self.state = h.digest()
        return self.encode(num(hashlib.sha3_256(self.state + b"squeeze").digest()) % self.p)


def commit_tau(c, tau, f):
    """commit(ck, f, 0) for ck[i] = tau^i G: f(tau) G"""
    return R.mul(c, R.poly_eval(c.r, f, tau), (c.gx, c.gy))


def folded_polys(p, hat_P, x):
    """[hat_P, Pi_1, ..., Pi_{ell-1}] (:1085-1095): fold i uses x[ell - i - 1]"""
    ell = len(x)
    assert len(hat_P) == 1 << ell and ell >= 1
    polys = [list(hat_P)]
    for i in range(ell - 1):
        polys.append(R.fold_pairs(p, polys[-1], x[ell - i - 1]))
    return polys


def prove(c, tau, hat_P, x, tr):
    """-> (com, v, w): com / w affine points (None = the identity), v[i] = [f_i(r), f_i(-r), f_i(r^2)] as integers (:1076-1116, :1007-1072)"""
    p = c.r
    polys = folded_polys(p, hat_P, x)
    com = [commit_tau(c, tau, f) for f in polys[1:]]                                                  # :1100
    r = tr.decode(tr.stage(0, b"".join(R.point_to_xy64(P) for P in com), len(com), bytes(int(P is None) for P in com)))   # :1105
    u = [r, (-r) % p, r * r % p]                                                                      # :1106
    v = [[R.poly_eval(p, f, uj) for uj in u] for f in polys]                                          # :1049-1056
    q = tr.decode(tr.stage(1, b"".join(tr.encode(e) for row in v for e in row), 3 * len(v), None))    # :1058
    B = R.lincomb_powers(p, polys, q, len(hat_P))                                                     # :1059
    w = [commit_tau(c, tau, R.div_by_monomial(p, B, uj)) for uj in u]                                 # :1062-1065
    tr.stage(2, b"".join(R.point_to_xy64(P) for P in w), 3, bytes(int(P is None) for P in w))         # :1069
    return com, v, w


def verify(c, tau, C, x, y, com, v, w, tr, msm=None):
    """EvaluationEngineTrait::verify (:1119-1230) with the pairing replaced by L == tau R.  C: the commitment to hat_P (affine or None),
    y the claimed evaluation; com / w affine points or None; v integers; msm(scalars, points) -> point computes the L of :1207-1225
    (default: the oracle's definition).  -> (recurrence holds, L == tau R)"""
    p, ell = c.r, len(x)
    if len(v) != ell or len(com) != ell - 1:
        return False, False
    r = tr.decode(tr.stage(0, b"".join(R.point_to_xy64(P) for P in com), len(com), bytes(int(P is None) for P in com)))
    u = [r, (-r) % p, r * r % p]
    ok = True
    for i in range(ell):                                                                              # :1143-1153
        ypos, yneg = v[i][0], v[i][1]
        Y = v[i + 1][2] if i + 1 < ell else y
        xi = x[ell - i - 1]
        ok &= (2 * r * Y - (r * (1 - xi) * (ypos + yneg) + xi * (ypos - yneg))) % p == 0
    q = tr.decode(tr.stage(1, b"".join(tr.encode(e) for row in v for e in row), 3 * len(v), None))
    d0 = tr.decode(tr.stage(2, b"".join(R.point_to_xy64(P) for P in w), 3, bytes(int(P is None) for P in w)))
    d1 = d0 * d0 % p
    qpm, qp = [], (1 + d0 + d1) % p                                                                   # :1185-1190
    for _ in range(ell):
        qpm.append(qp)
        qp = qp * q % p
    B_u = []
    for j in range(3):                                                                                # :1194-1202
        acc = 0
        for row in reversed(v):
            acc = (acc * q + row[j]) % p
        B_u.append(acc)
    scal = qpm + [u[0], u[1] * d0 % p, u[2] * d1 % p, (-(B_u[0] + d0 * B_u[1] + d1 * B_u[2])) % p]   # :1207-1225
    L = (msm or (lambda s, pts: R.msm_naive(c, s, pts)))(scal, [C] + list(com) + list(w) + [(c.gx, c.gy)])
    Rp = R.add(c, R.add(c, w[0], R.mul(c, d0, w[1])), R.mul(c, d1, w[2]))                             # :1227-1230
    return bool(ok), L == R.mul(c, tau, Rp)


def lincomb_quotients(p, polys, q, points):
    """the definition of nmx_poly_lincomb_quotients: out_j[0] = B(u_j), out_j[1:] = div_by_monomial(B, u_j), B = sum q^i polys[i] (words mod p)"""
    n_out = max([len(f) for f in polys], default=0)
    B = R.lincomb_powers(p, [[e % p for e in f] for f in polys], q, n_out)
    return [([R.poly_eval(p, B, u)] + R.div_by_monomial(p, B, u)) if n_out else [] for u in points]


def lq_plan(n_out, chunk_opt=0):
    """the launch plan of the pass restated (nova_amd/csrc/hyperkzg.hpp lq_plan): level 0 in chunks of 4 (option: 8), every level above in
    chunks of 16, until one chunk is left -> (chunk, [n_0, n_1, ...])"""
    chunk = 8 if chunk_opt == 8 else 4
    ns = [n_out]
    while ns[-1] > (chunk if len(ns) == 1 else 16):
        K = chunk if len(ns) == 1 else 16
        ns.append((ns[-1] + K - 1) // K)
    return chunk, ns


def lq_point_power_exponents(chunk, levels):
    """level l works at u^(elements of level 0 per element of level l): 1, K, 16 K, ..."""
    out, e = [], 1
    for l in range(levels):
        out.append(e)
        e *= chunk if l == 0 else 16
    return out
