"""nmx_ppsnark_mem_oracles against the composition of existing calls it replaces, and nmx_field_gather against copies of the same bytes --
HBM operands, ONE process, the paths alternating.

  fused      nmx_ppsnark_mem_oracles, k = 2 memories of n elements
  composed   per memory  axpy(i + r, mem, gamma) and axpy(addr + r, L, gamma)        the two hashes (4 calls)
             concat([T_0, W_0, T_1, W_1])                                            one batch, as the fused call has
             batch_invert                                                            the 4 n inverses
             per memory  cross_term(inv_T, ts, 0, 0, u = 0)                          the product by ts (2 calls)
             The vectors i + r and addr + r, the zero vectors and u are built OUTSIDE the timed region (the C ABI has no way to build them in
             HBM, which is part of why the fused call exists): the composition is timed at its most favourable.
  gather     nmx_field_gather of n elements from a memory of n
  d2h + d2d  device-to-host copy of mem into pinned memory plus a device-to-device copy of the same bytes: what a host-side gather pays
             before and after it computes anything (its own work and the upload of L not counted)

Before anything is timed the two paths' eight outputs are compared byte for byte.  Times are a host clock around synchronous calls (a
call's launches and its wait included).  The repetitions run in `--blocks` blocks; within a block the paths alternate.  Reported per path:
the median over all repetitions with [p10, p90], and the median of every block.  The run-to-run spread of a path is the distance between
its lowest and its highest block median.  The condition (2^20): the fused call's median is not above the composition's by more than the
composition's own spread.  Prints a table and one JSON line.

  python scripts/bench_ppsnark_oracles.py                       # BN254 Fr, n = 2^14 and 2^20, 5 blocks of 10 repetitions
  python scripts/bench_ppsnark_oracles.py --logs 8 --reps 2 --blocks 2
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FID = 1              # BN254_FR
K = 2                # row and col


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    return {"median": statistics.median(s), "min": s[0], "max": s[-1], "p10": q(0.1), "p90": q(0.9), "n": len(s)}


def run_size(log_n, reps, blocks, warm):
    import numpy as np
    import torch
    from nova_amd import fieldvec as fv
    from tests import fv_common as fc
    p = fc.FIELDS[FID]
    n = 1 << log_n
    gpu = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
    rng = np.random.Generator(np.random.PCG64(log_n))
    gamma_i, r_i = 0x1234567890abcdef1234567890abcdef1234567890abcdef % p, 0x0fedcba987654321fedcba987654321fedcba987654321 % p
    gamma, r = fc.vec([gamma_i]).copy(), fc.vec([r_i]).copy()

    def small(vals):                         # integers below 2^63 as field elements
        out = np.zeros((len(vals), 32), np.uint8)
        out[:, :8] = np.asarray(vals, np.uint64).view(np.uint8).reshape(-1, 8)
        return out
    mems = [gpu(fc.rand_vec(FID, n, 10 + g)) for g in range(K)]
    addr_i = [rng.integers(0, n, size=n).astype(np.uint64) for g in range(K)]
    addrs = [gpu(small(a)) for a in addr_i]
    tss = [gpu(small(np.bincount(a.astype(np.int64), minlength=n))) for a in addr_i]
    Ls = [fv.gather(FID, mems[g], addrs[g]) for g in range(K)]
    # the composition's extra operands, built outside the timed region: i + r and addr + r through one axpy each (x + 1 * r_vec)
    one = fc.vec([1]).copy()
    r_vec = gpu(np.tile(r, (n, 1)))
    idx_r = fv.axpy(FID, gpu(small(np.arange(n, dtype=np.uint64))), r_vec, one)
    addr_r = [fv.axpy(FID, addrs[g], r_vec, one) for g in range(K)]
    zero_vec, zero = torch.zeros((n, 32), dtype=torch.uint8, device="cuda"), fc.vec([0]).copy()
    pinned = torch.empty((n, 32), dtype=torch.uint8).pin_memory()
    d2d_buf = torch.empty((n, 32), dtype=torch.uint8, device="cuda")

    def fused():
        return fv.ppsnark_mem_oracles(FID, mems, addrs, Ls, tss, gamma, r)

    def composed():
        T = [fv.axpy(FID, idx_r, mems[g], gamma) for g in range(K)]
        W = [fv.axpy(FID, addr_r[g], Ls[g], gamma) for g in range(K)]
        inv = fv.batch_invert(FID, fv.concat(FID, [T[0], W[0], T[1], W[1]]))
        tinv = [fv.cross_term(FID, inv[2 * g * n:(2 * g + 1) * n], tss[g], zero_vec, zero_vec, zero) for g in range(K)]
        return [(T[g], W[g], tinv[g], inv[(2 * g + 1) * n:(2 * g + 2) * n]) for g in range(K)]
    a, b = fused(), composed()
    assert all(bool((x == y).all()) for ma, mb in zip(a, b) for x, y in zip(ma, mb)), "the fused call and the composition disagree"
    del a, b
    paths = {
        "fused": fused,
        "composed": composed,
        "gather": lambda: fv.gather(FID, mems[0], addrs[0]),
        "d2h+d2d": lambda: (pinned.copy_(mems[0]), d2d_buf.copy_(mems[0]), torch.cuda.synchronize()),
    }
    for _ in range(warm):
        for fn in paths.values():
            fn()
    t = {k: [[] for _ in range(blocks)] for k in paths}
    for blk in range(blocks):
        for _ in range(reps):
            for k, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t[k][blk].append((time.perf_counter() - t0) * 1e3)
    row = {"log_n": log_n, "k": K}
    for k in paths:
        row[k] = stats([x for blk in t[k] for x in blk])
        row[k]["block_medians"] = [statistics.median(blk) for blk in t[k]]
        row[k]["spread"] = max(row[k]["block_medians"]) - min(row[k]["block_medians"])
    row["fused_minus_composed_ms"] = row["fused"]["median"] - row["composed"]["median"]
    row["condition_met"] = row["fused_minus_composed_ms"] <= row["composed"]["spread"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="14,20")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from nova_amd import _lib
    assert _lib.lib().nmx_init(0) == 0, _lib.lib().nmx_last_error().decode()
    rows = [run_size(int(x), a.reps, a.blocks, a.warmup) for x in a.logs.split(",")]
    print(f"{'n':>6} {'path':>9} {'median ms':>10} {'[p10, p90]':>20} {'block medians':>46} {'spread':>8}")
    for row in rows:
        for k in ("fused", "composed", "gather", "d2h+d2d"):
            m = row[k]
            print(f"{'2^%d' % row['log_n']:>6} {k:>9} {m['median']:>10.4f} {'[%.4f, %.4f]' % (m['p10'], m['p90']):>20} "
                  f"{' '.join('%.4f' % x for x in m['block_medians']):>46} {m['spread']:>8.4f}")
        print(f"{'2^%d' % row['log_n']:>6} fused - composed = {row['fused_minus_composed_ms']:+.4f} ms against the composition's spread of "
              f"{row['composed']['spread']:.4f} ms: condition {'met' if row['condition_met'] else 'NOT met'}")
    print(json.dumps({"bench": "ppsnark_oracles", "field": "BN254_FR", "rows": rows}))


if __name__ == "__main__":
    main()
