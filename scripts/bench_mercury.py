"""nmx_mercury_h_poly and nmx_mercury_divide_by_binomial on HBM operands against two copies of the same polynomial, in ONE process,
alternating.

  h          nmx_mercury_h_poly                      algorithmic bytes: f once
  div        nmx_mercury_divide_by_binomial          algorithmic bytes: f once + q once (the kernels read f twice: DESIGN.md)
  d2d        device-to-device copy of f into a q-sized buffer: the same mandatory bytes as the division, its yardstick
  d2h        device-to-host copy of f into pinned memory: what any host path pays first, and what the feature removes

Times are a host clock around synchronous calls (a call's launch and its wait included).  Each is reported as a median with its spread,
and each call's share of the HBM peak by algorithmic bytes.  Prints a table and one JSON line.

  python scripts/bench_mercury.py                       # BN254 Fr, 1024 x 1024 (2^20) and 512 x 1024 (2^19), 20 repetitions
  python scripts/bench_mercury.py --shapes 64x64 --reps 3
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FID = 1              # BN254_FR
HBM_PEAK_GBS = 8000  # MI355X datasheet peak, GB/s


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    return {"median": statistics.median(s), "min": s[0], "max": s[-1], "p10": q(0.1), "p90": q(0.9), "n": len(s)}


def run_shape(n_rows, n_cols, reps, warm):
    import torch
    from nova_amd import fieldvec as fv
    from tests import fv_common as fc
    n = n_rows * n_cols
    f = torch.from_numpy(fc.rand_vec(FID, n, 1).copy()).cuda()
    eq = torch.from_numpy(fc.rand_vec(FID, n_cols, 2).copy()).cuda()
    alpha = fc.rand_vec(FID, 1, 3).copy()
    qbuf = torch.empty(((n_rows - 1) * n_cols, 32), dtype=torch.uint8, device="cuda")
    pinned = torch.empty((n, 32), dtype=torch.uint8).pin_memory()
    paths = {
        "h": lambda: fv.mercury_h_poly(FID, f, n_rows, n_cols, eq),
        "div": lambda: fv.mercury_divide_by_binomial(FID, f, n_rows, n_cols, alpha),
        "d2d": lambda: (qbuf.copy_(f[:qbuf.shape[0]]), torch.cuda.synchronize()),
        "d2h": lambda: (pinned.copy_(f), torch.cuda.synchronize()),
    }
    for _ in range(warm):
        for fn in paths.values():
            fn()
    t = {k: [] for k in paths}
    for _ in range(reps):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t[k].append((time.perf_counter() - t0) * 1e3)
    row = {"n_rows": n_rows, "n_cols": n_cols}
    bytes_of = {"h": 32 * n, "div": 32 * (2 * n - n_cols), "d2d": 64 * (n - n_cols), "d2h": 32 * n}
    for k in paths:
        row[k + "_ms"] = stats(t[k])
        row[k + "_gbs"] = bytes_of[k] / row[k + "_ms"]["median"] / 1e6
        row[k + "_share_of_peak"] = row[k + "_gbs"] / HBM_PEAK_GBS
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x1024,512x1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from nova_amd import _lib
    assert _lib.lib().nmx_init(0) == 0, _lib.lib().nmx_last_error().decode()
    rows = [run_shape(*[int(x) for x in s.split("x")], a.reps, a.warmup) for s in a.shapes.split(",")]
    print(f"{'shape':>11} {'path':>4} {'median ms':>10} {'[p10, p90]':>18} {'GB/s (algorithmic)':>19} {'of HBM peak':>12}")
    for r in rows:
        for k in ("h", "div", "d2d", "d2h"):
            m = r[k + "_ms"]
            print(f"{'%dx%d' % (r['n_rows'], r['n_cols']):>11} {k:>4} {m['median']:>10.4f} {'[%.4f, %.4f]' % (m['p10'], m['p90']):>18} {r[k + '_gbs']:>19.0f} "
                  f"{100 * r[k + '_share_of_peak']:>11.1f}%")
    print(json.dumps({"bench": "mercury", "field": "BN254_FR", "hbm_peak_gbs": HBM_PEAK_GBS, "rows": rows}))


if __name__ == "__main__":
    main()
