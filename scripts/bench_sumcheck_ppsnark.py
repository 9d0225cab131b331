"""nmx_sumcheck_prove_ppsnark against the path a caller had to compose before it existed, in ONE process, alternating.

  new        nmx_sumcheck_prove_ppsnark over the sixteen HBM-resident tables (copied fresh before every call: the prover binds in place)
  composed   per round the nine sums calls -- nmx_sumcheck_plain_sums kind 2 (claims 0, 1), nmx_sumcheck_eq_sums mode 3 (claims 2, 4),
             mode 2 (claims 3, 5) and mode 1 (claim 7), nmx_sumcheck_plain_sums kind 4 (claim 6) and kind 3 (claim 8) -- then sixteen
             nmx_mle_bind_top in place; derive_from_claim_deg2 / _deg1, update_claim, the batching, from_evals_deg3 and the claim update
             in Python integers, the same transcript.  The sqrt-size eq tables of every round are built once, outside the timing.

Both paths see the same transcript (SHA3 stand-in, tests/spartan_common.StandInTranscript) and must return the same round polynomials;
that is asserted once per shape before anything is timed.  Times are a host clock around synchronous calls and include the device-side
copy of the tables, which both paths pay.  Prints a table and one JSON line.

  python scripts/bench_sumcheck_ppsnark.py                       # BN254 Fr, 2^14 and 2^20, 10 repetitions
  python scripts/bench_sumcheck_ppsnark.py --sizes 10 --reps 3
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FID = 1  # BN254_FR


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    return {"median": statistics.median(s), "min": s[0], "max": s[-1], "p10": q(0.1), "p90": q(0.9), "n": len(s)}


def run_shape(lg, reps, warm):
    import torch
    from nova_amd import fieldvec as fv
    from tests import batched_cubic_common as bc
    from tests import fv_common as fc
    from tests import ppsnark_sc_common as pc
    from tests import spartan_common as sp
    p = fc.FIELDS[FID]
    n = 1 << lg
    up = lambda v: torch.from_numpy(fc.vec(v).copy()).cuda()  # noqa: E731
    src = [torch.from_numpy(fc.rand_vec(FID, n, 100 + t + lg).copy()).cuda() for t in range(pc.NT)]
    rho_v, ro_v = fc.rand_vec(FID, lg, 7).copy(), fc.rand_vec(FID, lg, 8).copy()
    rho, ro = fc.ints(rho_v), fc.ints(ro_v)
    claims2 = [12345, 6789]  # any claims give a well-formed transcript; the verifier equation is the tests' business
    s = 0x1234567
    coeffs = [pow(s, i, p) for i in range(9)]
    first_half = lg // 2

    def eq_tables(taus):    # per round j (1-based): eq over taus[j:], split as EqSumCheckInstance does (sumcheck.rs:1233-1253)
        out = []
        for j in range(1, lg + 1):
            if j < first_half:
                left, right = taus[j:first_half], taus[first_half:]
                out.append((up(bc.eq_table(p, left)), up(bc.eq_table(p, right)), len(right)))
            else:
                out.append((None, up(bc.eq_table(p, taus[j:])), 0))
        return out
    eq_rho, eq_ro = eq_tables(rho), eq_tables(ro)
    inv2 = pow(2, -1, p)
    i32 = lambda b: int.from_bytes(b, "little")  # noqa: E731

    def new_path():
        T = [t.clone() for t in src]
        torch.cuda.synchronize()  # the copies run on torch's stream; the library's stream is not ordered behind it
        tr = sp.StandInTranscript(p)
        polys, _r, _fin = fv.sumcheck_prove_ppsnark(FID, T, rho_v, ro_v, [sp.le(c) for c in claims2], [sp.le(c) for c in coeffs], tr)
        return polys

    def derive(tau, left_p, t0, tinf, claim, deg1):   # derive_from_claim_deg2 / _deg1 (random taus and challenges: never the fallback)
        eq0, slope = (1 - tau) % p, (2 * tau - 1) % p
        s0 = eq0 * left_p * t0 % p
        t1 = (claim - s0) * pow(tau * left_p % p, -1, p) % p
        tm1 = (2 * t0 - t1) % p if deg1 else (2 * tinf + 2 * t0 - t1) % p
        return s0, (0 if deg1 else slope * left_p * tinf % p), (eq0 - slope) * left_p * tm1 % p

    def composed_path():
        T = [t.clone() for t in src]
        torch.cuda.synchronize()  # the copies run on torch's stream; the library's stream is not ordered behind it
        tr = sp.StandInTranscript(p)
        running = [0] * 6 + [None, claims2[1], None]
        e = (coeffs[6] * claims2[0] + coeffs[7] * claims2[1]) % p
        lp_rho = lp_ro = 1
        polys = []
        for j in range(1, lg + 1):
            (eL, eR, sh), (oL, oR, osh) = eq_rho[j - 1], eq_ro[j - 1]
            ev = [None] * 9
            for g in (0, 1):
                b = 5 * g
                d = fv.sumcheck_plain_sums(FID, 2, T[b + pc.TINV_ROW], T[b + pc.WINV_ROW])
                ev[g] = (i32(d[0]), 0, i32(d[1]))
                a = fv.sumcheck_eq_sums(FID, 3, T[b + pc.TINV_ROW], T[b + pc.T_ROW], T[b + pc.TS_ROW], eR, eL, sh)
                ev[2 + 2 * g] = derive(rho[j - 1], lp_rho, i32(a[0]), i32(a[1]), running[2 + 2 * g], False)
                a = fv.sumcheck_eq_sums(FID, 2, T[b + pc.WINV_ROW], T[b + pc.W_ROW], None, eR, eL, sh)
                ev[3 + 2 * g] = derive(rho[j - 1], lp_rho, i32(a[0]), i32(a[1]), running[3 + 2 * g], False)
            c = fv.sumcheck_plain_sums(FID, 4, T[pc.L_ROW], T[pc.L_COL], T[pc.VAL])
            ev[6] = tuple(i32(x) for x in c)
            a = fv.sumcheck_eq_sums(FID, 1, T[pc.E], None, None, oR, oL, osh)
            ev[7] = derive(ro[j - 1], lp_ro, i32(a[0]), 0, running[7], True)
            w = fv.sumcheck_plain_sums(FID, 3, T[pc.MASKED_EQ], T[pc.W])
            ev[8] = (i32(w[0]), 0, i32(w[1]))
            c0, lead, cm1 = (sum(x[k] * co for x, co in zip(ev, coeffs)) % p for k in range(3))
            s1 = (e - c0) % p
            q2 = ((s1 + cm1) * inv2 - c0) % p
            co = [c0, (s1 - lead - c0 - q2) % p, q2, lead]
            polys.append([sp.le(x) for x in co])
            r = i32(tr(polys[-1]))
            e = sp.poly_at(p, co, r)
            for i in (2, 3, 4, 5, 7):
                running[i] = pc.update_claim(p, running[i], ev[i], r)
            rb = sp.le(r)
            T = [fv.bind_poly_var_top(FID, t, rb, in_place=True) for t in T]
            lp_rho = lp_rho * ((1 - rho[j - 1] - r + 2 * r * rho[j - 1]) % p) % p
            lp_ro = lp_ro * ((1 - ro[j - 1] - r + 2 * r * ro[j - 1]) % p) % p
        torch.cuda.synchronize()
        return polys

    assert new_path() == composed_path(), "the two paths disagree"
    for _ in range(warm):
        new_path(), composed_path()
    t_new, t_old = [], []
    for _ in range(reps):
        for fn, acc in ((new_path, t_new), (composed_path, t_old)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t) * 1e3)
    return {"log2n": lg, "new_ms": stats(t_new), "composed_ms": stats(t_old)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="14,20")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from nova_amd import _lib
    assert _lib.lib().nmx_init(0) == 0, _lib.lib().nmx_last_error().decode()
    rows = [run_shape(int(lg), a.reps, a.warmup) for lg in a.sizes.split(",")]
    print(f"{'log2n':>5} {'new median ms':>14} {'[p10, p90]':>20} {'composed median ms':>19} {'[p10, p90]':>20}")
    for r in rows:
        n_, c_ = r["new_ms"], r["composed_ms"]
        print(f"{r['log2n']:>5} {n_['median']:>14.3f} {'[%.3f, %.3f]' % (n_['p10'], n_['p90']):>20} {c_['median']:>19.3f} "
              f"{'[%.3f, %.3f]' % (c_['p10'], c_['p90']):>20}")
    print(json.dumps({"bench": "sumcheck_ppsnark", "field": "BN254_FR", "rows": rows}))


if __name__ == "__main__":
    main()
