"""nmx_neutron_fold_sums and nmx_neutron_fold_witness on HBM operands against two copies of the same bytes, in ONE process, alternating.

  sums       nmx_neutron_fold_sums                   algorithmic bytes: the six product vectors once, 6 x 32 x N
  fold       nmx_neutron_fold_witness                algorithmic bytes: w1, w2 read and w written, 3 x 32 x n (n = N + left + right here)
  d2d        device-to-device copy moving the fold's bytes (1.5 n elements copied: 3 x 32 x n bytes read + written): its yardstick
  d2h        device-to-host copy of the six product vectors into pinned memory: what a host-side prove_helper pays first, and what the
             sums call removes

Times are a host clock around synchronous calls (a call's launch and its wait included).  Each is reported as a median with its spread,
and each call's share of the HBM peak by algorithmic bytes.  The one condition this script checks ("sums_below_d2h"): the sums' median lies
below the d2h copy's median by more than that copy's own p90 - p10 spread.  Prints a table and one JSON line.

  python scripts/bench_neutron_fold.py                       # BN254 Fr, (1024, 1024) and (128, 128), 20 repetitions
  python scripts/bench_neutron_fold.py --shapes 64x64 --reps 3
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
PATHS = ("sums", "fold", "d2d", "d2h")


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    return {"median": statistics.median(s), "min": s[0], "max": s[-1], "p10": q(0.1), "p90": q(0.9), "n": len(s)}


def run_shape(left, right, reps, warm):
    import torch
    from nova_amd import fieldvec as fv
    from tests import fv_common as fc
    n, n_e = left * right, left + right
    dev = lambda m, seed: torch.from_numpy(fc.rand_vec(FID, m, seed).copy()).cuda()  # noqa: E731
    E1, E2 = dev(n_e, 1), dev(n_e, 2)
    six = torch.cat([dev(n, 3 + j) for j in range(6)])             # Az1, Bz1, Cz1, Az2, Bz2, Cz2, contiguous: one copy brings all six to the host
    A1, B1, C1, A2, B2, C2 = (six[j * n:(j + 1) * n] for j in range(6))
    rho, r_b = fc.rand_vec(FID, 1, 11).copy(), fc.rand_vec(FID, 1, 12).copy()
    w_out = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    e_out = torch.empty((n_e, 32), dtype=torch.uint8, device="cuda")
    n_f = n + n_e                                                   # elements the fold writes
    d2d_src, d2d_dst = six[:n_f + n_f // 2], torch.empty((n_f + n_f // 2, 32), dtype=torch.uint8, device="cuda")
    pinned = torch.empty((6 * n, 32), dtype=torch.uint8).pin_memory()
    from nova_amd import _lib
    lib, flags = _lib.lib(), _lib.SCALARS_DEVICE

    def fold():                                                     # the raw call: the outputs are allocated once, outside the clock
        rc = lib.nmx_neutron_fold_witness(FID, A1.data_ptr(), A2.data_ptr(), n, E1.data_ptr(), E2.data_ptr(), n_e, r_b.ctypes.data, flags,
                                          w_out.data_ptr(), e_out.data_ptr())
        assert rc == 0, lib.nmx_last_error().decode()
    paths = {
        "sums": lambda: fv.neutron_fold_sums(FID, left, right, E1, A1, B1, C1, E2, A2, B2, C2, rho),
        "fold": fold,
        "d2d": lambda: (d2d_dst.copy_(d2d_src), torch.cuda.synchronize()),
        "d2h": lambda: (pinned.copy_(six), torch.cuda.synchronize()),
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
    row = {"left": left, "right": right}
    bytes_of = {"sums": 6 * 32 * n, "fold": 3 * 32 * n_f, "d2d": 2 * 32 * (n_f + n_f // 2), "d2h": 6 * 32 * n}
    for k in paths:
        row[k + "_ms"] = stats(t[k])
        row[k + "_gbs"] = bytes_of[k] / row[k + "_ms"]["median"] / 1e6
        row[k + "_share_of_peak"] = row[k + "_gbs"] / HBM_PEAK_GBS
    d2h = row["d2h_ms"]
    row["sums_below_d2h"] = bool(row["sums_ms"]["median"] < d2h["median"] - (d2h["p90"] - d2h["p10"]))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x1024,128x128")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from nova_amd import _lib
    assert _lib.lib().nmx_init(0) == 0, _lib.lib().nmx_last_error().decode()
    rows = [run_shape(*[int(x) for x in s.split("x")], a.reps, a.warmup) for s in a.shapes.split(",")]
    print(f"{'shape':>11} {'path':>4} {'median ms':>10} {'[p10, p90]':>18} {'GB/s (algorithmic)':>19} {'of HBM peak':>12}")
    for r in rows:
        for k in PATHS:
            m = r[k + "_ms"]
            print(f"{'%dx%d' % (r['left'], r['right']):>11} {k:>4} {m['median']:>10.4f} {'[%.4f, %.4f]' % (m['p10'], m['p90']):>18} {r[k + '_gbs']:>19.0f} "
                  f"{100 * r[k + '_share_of_peak']:>11.1f}%")
        print(f"{'%dx%d' % (r['left'], r['right']):>11} sums below d2h by more than d2h's p90 - p10: {r['sums_below_d2h']}")
    print(json.dumps({"bench": "neutron_fold", "field": "BN254_FR", "hbm_peak_gbs": HBM_PEAK_GBS, "rows": rows}))


if __name__ == "__main__":
    main()
