"""nmx_ppsnark_spark_repr against the copies a host-built key pays at the least, and nmx_masked_eq_evals against nmx_eq_evals_from_points --
ONE process, the paths alternating.

  uniform    nmx_ppsnark_spark_repr, k = 3 matrices of n / 4 rows and about n / 3.2 entries each, columns uniform over n / 2; HBM outputs
  heavy      the same matrices with the FIRST entry of every row of every matrix moved to column 0: one column holds 3 n / 4 entries
  h2d        a pinned host-to-device copy of 7 n x 32 bytes: what a caller that builds the seven vectors on the host pays after building them
  d2d        a device-to-device copy of 7 n x 32 bytes: the floor of writing seven vectors
  masked     nmx_masked_eq_evals(ell = 20, num_masked_vars = 10), HBM output         (only with --logs containing 20)
  eq         nmx_eq_evals_from_points(ell = 20), HBM output

Before anything is timed every output of both distributions is checked against numpy (row by np.repeat, ts by np.bincount).  Times are a
host clock around synchronous calls (a call's launches and its wait included).  The repetitions run in `--blocks` blocks; within a block the
paths alternate.  Reported per path: the median over all repetitions with [p10, p90], the median of every block, and the spread (highest
minus lowest block median).  Prints a table, the heavy / uniform ratio, and one JSON line.  No threshold rests on these numbers.

  python scripts/bench_ppsnark_key.py                       # BN254 Fr, n = 2^14 and 2^20, 5 blocks of 10 repetitions
  python scripts/bench_ppsnark_key.py --logs 10 --reps 2 --blocks 2
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FID = 1              # BN254_FR
K = 3                # A, B, C


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    return {"median": statistics.median(s), "min": s[0], "max": s[-1], "p10": q(0.1), "p90": q(0.9), "n": len(s)}


def low_words(t):
    import numpy as np
    a = t.cpu().numpy()
    assert not a[:, 8:].any()
    return a[:, :8].copy().view(np.uint64).reshape(-1)


def run_size(log_n, reps, blocks, warm):
    import numpy as np
    import torch
    from nova_amd import fieldvec as fv
    from tests import fv_common as fc
    n = 1 << log_n
    rows, cols = max(n // 4, 1), max(n // 2, 1)
    rng = np.random.Generator(np.random.PCG64(log_n))
    sets = {"uniform": [], "heavy": []}
    host = {"uniform": [], "heavy": []}
    for j in range(K):
        nnz = max(n // 3 - 16 * j - 5, rows)
        counts = 1 + rng.multinomial(nnz - rows, np.full(rows, 1.0 / rows))
        indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        ix = rng.integers(0, cols, size=nnz).astype(np.uint64)
        data = fc.rand_vec(FID, nnz, 30 + j).copy()
        ixh = ix.copy()
        ixh[indptr[:-1].astype(np.int64)] = 0
        for name, idx in (("uniform", ix), ("heavy", ixh)):
            sets[name].append(fv.SparseMatrix(FID, indptr, idx, data, cols))
            host[name].append((indptr, idx, data))
    # correctness first
    for name in sets:
        row, col, vals, ts_row, ts_col = fv.ppsnark_spark_repr(sets[name], n)
        w_row = np.concatenate([np.repeat(np.arange(rows, dtype=np.uint64), np.diff(ip).astype(np.int64)) for ip, _ix, _d in host[name]])
        w_col = np.concatenate([idx for _ip, idx, _d in host[name]])
        total = len(w_row)
        w_row = np.concatenate([w_row, np.zeros(n - total, np.uint64)])
        w_col = np.concatenate([w_col, np.full(n - total, n - 1, np.uint64)])
        assert (low_words(row) == w_row).all() and (low_words(col) == w_col).all(), name
        assert (low_words(ts_row) == np.bincount(w_row.astype(np.int64), minlength=n)).all(), name
        assert (low_words(ts_col) == np.bincount(w_col.astype(np.int64), minlength=n)).all(), name
        off = 0
        for j, (_ip, _ix, d) in enumerate(host[name]):
            v = vals[j].cpu().numpy()
            assert (v[off:off + len(d)] == d).all() and not v[:off].any() and not v[off + len(d):].any(), name
            off += len(d)
        del row, col, vals, ts_row, ts_col
    pinned = torch.empty((7 * n, 32), dtype=torch.uint8).pin_memory()
    dst = torch.empty((7 * n, 32), dtype=torch.uint8, device="cuda")
    src = torch.zeros((7 * n, 32), dtype=torch.uint8, device="cuda")
    paths = {
        "uniform": lambda: fv.ppsnark_spark_repr(sets["uniform"], n),
        "heavy": lambda: fv.ppsnark_spark_repr(sets["heavy"], n),
        "h2d": lambda: (dst.copy_(pinned, non_blocking=True), torch.cuda.synchronize()),
        "d2d": lambda: (dst.copy_(src), torch.cuda.synchronize()),
    }
    if log_n == 20:
        r = fc.rand_vec(FID, 20, 99).copy()
        paths["masked"] = lambda: fv.masked_eq_evals(FID, r, 10, device=True)
        paths["eq"] = lambda: fv.eq_evals_from_points(FID, r, device=True)
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
    out = {"log_n": log_n, "k": K, "total_entries": int(sum(len(h[1]) for h in host["uniform"])), "heavy_column_entries": K * rows}
    for k in paths:
        out[k] = stats([x for blk in t[k] for x in blk])
        out[k]["block_medians"] = [statistics.median(blk) for blk in t[k]]
        out[k]["spread"] = max(out[k]["block_medians"]) - min(out[k]["block_medians"])
    out["heavy_over_uniform"] = out["heavy"]["median"] / out["uniform"]["median"]
    for ms in sets.values():
        for m in ms:
            m.close()
    return out


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
        for k in ("uniform", "heavy", "h2d", "d2d", "masked", "eq"):
            if k not in row:
                continue
            m = row[k]
            print(f"{'2^%d' % row['log_n']:>6} {k:>9} {m['median']:>10.4f} {'[%.4f, %.4f]' % (m['p10'], m['p90']):>20} "
                  f"{' '.join('%.4f' % x for x in m['block_medians']):>46} {m['spread']:>8.4f}")
        print(f"{'2^%d' % row['log_n']:>6} heavy / uniform = {row['heavy_over_uniform']:.3f} ({row['heavy_column_entries']} of {row['total_entries']} entries in one column)")
    print(json.dumps({"bench": "ppsnark_key", "field": "BN254_FR", "rows": rows}))


if __name__ == "__main__":
    main()
