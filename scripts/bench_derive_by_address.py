"""nmx_bases_derive_by_address against the two things it can be set beside -- ONE process, the paths alternating.

  derive_host / derive_hbm   nmx_bases_derive_by_address(ck, addresses, n, table_size) with host and with HBM addresses, no window tables
                             for the derived key: keys, pair sort, bounds, plan, accumulate, folds, normalisation, the wait, unregister
  transfers                  nmx_bases_read of the n source points plus nmx_bases_register of table_size points: what a host-side derivation
                             pays to move the key, WITHOUT its n point additions (the reference's serial loop)
  sparse_sum                 nmx_msm_sparse_handle with NULL scalars over the same n indices: the same gathers and additions into ONE sum

BN254 G1, a generated source key; two address distributions: uniform, and three quarters of the addresses on index 0 (padding).  Before
anything is timed the two address forms are compared byte for byte, and sum_j derived[j] with the sparse sum of all n points.  Times are a
host clock around synchronous calls.  The repetitions run in `--blocks` blocks; within a block the paths alternate.  Reported per path: the
median over all repetitions with [p10, p90], the median of every block, and the spread (highest minus lowest block median).  Prints a table
and one JSON line.  No threshold rests on these numbers.  NOT done here: no kernel trace, nothing tuned (derive_lmax stays at its rule), the
rocPRIM pair sort not compared with a counting scatter.

  python scripts/bench_derive_by_address.py                       # n = 2^20, table_size = 2^16, 5 blocks of 6 repetitions
  python scripts/bench_derive_by_address.py --log-n 12 --log-table 8 --reps 2 --blocks 2
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CID = 0              # BN254 G1


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    return {"median": statistics.median(s), "min": s[0], "max": s[-1], "p10": q(0.1), "p90": q(0.9), "n": len(s)}


def run_case(name, log_n, log_t, reps, blocks, warm):
    import numpy as np
    import torch
    from nova_amd import _lib
    L = _lib.lib()
    n, T = 1 << log_n, 1 << log_t
    rng = np.random.default_rng(log_n * 100 + log_t)
    addr = rng.integers(0, T, n, dtype=np.uint64)
    if name == "skewed":
        addr[np.arange(n) % 4 != 0] = 0
    idx = np.arange(n, dtype=np.uint64)
    addr_dev = torch.from_numpy(addr.view(np.int64).copy()).cuda()

    def check(rc):
        assert rc == 0, L.nmx_last_error().decode()
    src = ctypes.c_uint64(0)
    check(L.nmx_bases_generate(CID, 1, n, _lib.BASES_PRECOMPUTE, ctypes.byref(src)))
    host_rows = np.zeros((n, 64), np.uint8)
    table_rows = np.zeros((T, 64), np.uint8)

    def derive(dev, keep=False):
        h = ctypes.c_uint64(0)
        check(L.nmx_bases_derive_by_address(src.value, addr_dev.data_ptr() if dev else addr.ctypes.data, n, T, _lib.SCALARS_DEVICE if dev else 0,
                                            ctypes.byref(h)))
        if keep:
            return h.value
        check(L.nmx_bases_unregister(h.value))

    def transfers():
        h = ctypes.c_uint64(0)
        check(L.nmx_bases_read(src.value, 0, n, host_rows.ctypes.data))
        check(L.nmx_bases_register(CID, table_rows.ctypes.data, T, 0, ctypes.byref(h)))
        check(L.nmx_bases_unregister(h.value))

    def sparse_sum(handle=None, count=None, out=None):
        o = np.zeros(64, np.uint8) if out is None else out
        inf = np.zeros(1, np.uint8)
        check(L.nmx_msm_sparse_handle(src.value if handle is None else handle, idx.ctypes.data, None, n if count is None else count, 0, o.ctypes.data,
                                      inf.ctypes.data))
        return o
    # correctness first: both address forms give the same key, and the derived key's points sum to the sum of the n source points
    hh, hd = derive(False, keep=True), derive(True, keep=True)
    a, b = np.zeros((T, 64), np.uint8), np.zeros((T, 64), np.uint8)
    check(L.nmx_bases_read(hh, 0, T, a.ctypes.data))
    check(L.nmx_bases_read(hd, 0, T, b.ctypes.data))
    assert (a == b).all(), "host and HBM addresses disagree"
    table_rows[:] = a          # what `transfers` registers: valid points
    assert (sparse_sum(hh, T) == sparse_sum()).all(), "the derived key's points do not sum to the source's"
    check(L.nmx_bases_unregister(hh))
    check(L.nmx_bases_unregister(hd))

    paths = {"derive_host": lambda: derive(False), "derive_hbm": lambda: derive(True), "transfers": transfers, "sparse_sum": sparse_sum}
    for _ in range(warm):
        for fn in paths.values():
            fn()
    t = {k: [[] for _ in range(blocks)] for k in paths}
    for blk in range(blocks):
        for _ in range(reps):
            for k, fn in paths.items():
                t0 = time.perf_counter()
                fn()
                t[k][blk].append((time.perf_counter() - t0) * 1e3)
    check(L.nmx_bases_unregister(src.value))
    out = {"case": name, "log_n": log_n, "log_table": log_t}
    for k in paths:
        out[k] = stats([x for blk in t[k] for x in blk])
        out[k]["block_medians"] = [statistics.median(blk) for blk in t[k]]
        out[k]["spread"] = max(out[k]["block_medians"]) - min(out[k]["block_medians"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--log-table", type=int, default=16)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from nova_amd import _lib
    assert _lib.lib().nmx_init(0) == 0, _lib.lib().nmx_last_error().decode()
    rows = [run_case(name, a.log_n, a.log_table, a.reps, a.blocks, a.warmup) for name in ("uniform", "skewed")]
    print(f"{'case':>8} {'path':>12} {'median ms':>10} {'[p10, p90]':>20} {'block medians':>46} {'spread':>8}")
    for row in rows:
        for k, m in row.items():
            if not isinstance(m, dict):
                continue
            print(f"{row['case']:>8} {k:>12} {m['median']:>10.4f} {'[%.4f, %.4f]' % (m['p10'], m['p90']):>20} "
                  f"{' '.join('%.4f' % x for x in m['block_medians']):>46} {m['spread']:>8.4f}")
    print(json.dumps({"bench": "derive_by_address", "curve": "BN254_G1", "rows": rows}))


if __name__ == "__main__":
    main()
