"""nmx_sumcheck_prove_batched_cubic against the path a caller had to compose before it existed, in ONE process, alternating.

  new        nmx_sumcheck_prove_batched_cubic over 3 k HBM-resident tables (copied fresh before every call: the prover binds in place)
  composed   per round: k x nmx_sumcheck_eq_sums (round 1) / k x nmx_sumcheck_bind_eq_sums mode 3 (later rounds), the alpha combination,
             derive_from_claim_deg2, from_evals_deg3 and the claim update in Python integers, the same transcript; the last bind (tables
             of two elements) with nmx bind_poly_var_top.  The sqrt-size eq tables of every round are built once, outside the timing.

Both paths see the same transcript (SHA3 stand-in, tests/spartan_common.StandInTranscript) and must return the same round polynomials;
that is asserted once per shape before anything is timed.  Times are a host clock around synchronous calls and include the device-side
copy of the tables, which both paths pay.  Prints a table and one JSON line.  docs/measurements.md has the one run of its default shapes.

  python scripts/bench_sumcheck_batched.py                       # BN254 Fr, 2^14 and 2^20, k = 1, 3, 8, 10 repetitions
  python scripts/bench_sumcheck_batched.py --sizes 12 --ks 2 --reps 3
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


def run_shape(lg, k, reps, warm):
    import torch
    from nova_amd import fieldvec as fv
    from tests import batched_cubic_common as bc
    from tests import fv_common as fc
    from tests import spartan_common as sp
    p = fc.FIELDS[FID]
    n = 1 << lg
    src = [[torch.from_numpy(fc.rand_vec(FID, n, 100 * w + i + lg).copy()).cuda() for i in range(k)] for w in range(3)]
    taus_v, al_v = fc.rand_vec(FID, lg, 7).copy(), fc.rand_vec(FID, k, 8).copy()
    taus, al = fc.ints(taus_v), fc.ints(al_v)
    claim = 12345  # any claim gives a well-formed transcript; the verifier equation is the tests' business
    first_half = lg // 2
    # per round j (1-based): eq over taus[j:], split as EqSumCheckInstance does (sumcheck.rs:1233-1253)
    eqs = []
    for j in range(1, lg + 1):
        if j < first_half:
            left, right = taus[j:first_half], taus[first_half:]
            eqs.append((torch.from_numpy(fc.vec(bc.eq_table(p, left)).copy()).cuda(), torch.from_numpy(fc.vec(bc.eq_table(p, right)).copy()).cuda(), len(right)))
        else:
            eqs.append((None, torch.from_numpy(fc.vec(bc.eq_table(p, taus[j:])).copy()).cuda(), 0))
    inv2 = pow(2, -1, p)
    i32 = lambda b: int.from_bytes(b, "little")  # noqa: E731

    def fresh():
        out = [[t.clone() for t in row] for row in src]
        torch.cuda.synchronize()  # the copies run on torch's stream; the library's stream is not ordered behind it
        return out

    def new_path():
        A, B, C = fresh()
        tr = sp.StandInTranscript(p)
        polys, _r, _cl = fv.sumcheck_prove_batched_cubic(FID, sp.le(claim), taus_v, A, B, C, al_v, tr)
        return polys

    def composed_path():
        A, B, C = fresh()
        tr = sp.StandInTranscript(p)
        cl, left_p, polys, r = claim, 1, [], None
        for j in range(1, lg + 1):
            eqL, eqR, shift = eqs[j - 1]
            t0 = tinf = 0
            for i in range(k):
                if j == 1:
                    s = fv.sumcheck_eq_sums(FID, 3, A[i], B[i], C[i], eqR, eqL, shift)
                else:
                    A[i], B[i], C[i], s = fv.sumcheck_bind_eq_sums(FID, 3, A[i], B[i], C[i], sp.le(r), eqR, eqL, shift)
                t0, tinf = (t0 + al[i] * i32(s[0])) % p, (tinf + al[i] * i32(s[1])) % p
            tau = taus[j - 1]
            eq0, slope = (1 - tau) % p, (2 * tau - 1) % p
            s0 = eq0 * left_p * t0 % p
            t1 = (cl - s0) * pow(tau * left_p % p, -1, p) % p          # (random taus and challenges: never the fallback)
            sm1 = (eq0 - slope) * left_p * ((2 * tinf + 2 * t0 - t1) % p) % p
            lead = slope * left_p * tinf % p
            s1 = (cl - s0) % p
            c2 = ((s1 + sm1) * inv2 - s0) % p
            co = [s0, (s1 - lead - s0 - c2) % p, c2, lead]
            polys.append([sp.le(c) for c in co])
            r = i32(tr(polys[-1]))
            cl = sp.poly_at(p, co, r)
            left_p = left_p * ((1 - tau - r + 2 * r * tau) % p) % p
            if j == lg:
                for i in range(k):                                       # the last bind: no sums follow
                    A[i], B[i], C[i] = (fv.bind_poly_var_top(FID, X, sp.le(r)) for X in (A[i], B[i], C[i]))
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
    return {"log2n": lg, "k": k, "new_ms": stats(t_new), "composed_ms": stats(t_old)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="14,20")
    ap.add_argument("--ks", default="1,3,8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from nova_amd import _lib
    assert _lib.lib().nmx_init(0) == 0, _lib.lib().nmx_last_error().decode()
    rows = [run_shape(int(lg), int(k), a.reps, a.warmup) for lg in a.sizes.split(",") for k in a.ks.split(",")]
    print(f"{'log2n':>5} {'k':>3} {'new median ms':>14} {'[p10, p90]':>20} {'composed median ms':>19} {'[p10, p90]':>20}")
    for r in rows:
        n_, c_ = r["new_ms"], r["composed_ms"]
        print(f"{r['log2n']:>5} {r['k']:>3} {n_['median']:>14.3f} {'[%.3f, %.3f]' % (n_['p10'], n_['p90']):>20} {c_['median']:>19.3f} "
              f"{'[%.3f, %.3f]' % (c_['p10'], c_['p90']):>20}")
    print(json.dumps({"bench": "sumcheck_batched", "field": "BN254_FR", "rows": rows}))


if __name__ == "__main__":
    main()
