"""nmx_bases_setup_from_tau at window widths c = 8, 12 and 16 against the two ways a key of the same size could be had before -- ONE process,
the paths alternating.

  tau_c8 / tau_c12 / tau_c16   nmx_bases_setup_from_tau(n) with nmx_set_option("fixed_base_c", c): host window bases and squarings, the
                               table, the multiplication with its block normalisation, the wait
  generate                     nmx_bases_generate(n): (k0 + i) G, one 64-bit double-and-add and one inversion per lane (not a KZG key)
  register                     nmx_bases_register(NMX_BASES_VALIDATE) of a pageable host array of n points: what a host-made key still pays
                               after its CPU generation (upload, validation, conversion)

No window tables for MSMs are built in any path (no NMX_BASES_PRECOMPUTE): that step is the same for all of them.  Before anything is
timed the tau key of every width is compared byte for byte with the others, and its first points with the oracle.  Times are a host clock
around synchronous calls; every call also unregisters its key (freeing n x 64 bytes), in all paths alike.  The repetitions run in
`--blocks` blocks; within a block the paths alternate.  Reported per path: the median over all repetitions with [p10, p90], the median
of every block, and the spread (highest minus lowest block median).  Prints a table and one JSON line.  No threshold rests on these numbers.

  python scripts/bench_fixed_base.py                       # BN254 G1, n = 2^16 and 2^20, 5 blocks of 6 repetitions
  python scripts/bench_fixed_base.py --logs 10 --reps 2 --blocks 2
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
WIDTHS = (8, 12, 16)


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    return {"median": statistics.median(s), "min": s[0], "max": s[-1], "p10": q(0.1), "p90": q(0.9), "n": len(s)}


def run_size(log_n, reps, blocks, warm):
    import numpy as np
    from nova_amd import _lib
    from oracle import pyref as R
    from tests import fixed_base_common as fb
    L = _lib.lib()
    c = R.CURVES_BY_ID[CID]
    n = 1 << log_n
    tau = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % c.r
    t32 = fb.scalar_rows(c, [tau])

    def check(rc):
        assert rc == 0, L.nmx_last_error().decode()

    def tau_key(cw, keep=False):
        h = ctypes.c_uint64(0)
        check(L.nmx_set_option(b"fixed_base_c", cw))
        check(L.nmx_bases_setup_from_tau(CID, t32.ctypes.data, n, 0, ctypes.byref(h)))
        if keep:
            return h.value
        check(L.nmx_bases_unregister(h.value))

    def read(handle):
        out = np.zeros((n, 64), np.uint8)
        check(L.nmx_bases_read(handle, 0, n, out.ctypes.data))
        check(L.nmx_bases_unregister(handle))
        return out
    # correctness first: the widths agree, and the first points are tau^i G
    keys = [read(tau_key(cw, keep=True)) for cw in WIDTHS]
    assert all((k == keys[0]).all() for k in keys[1:]), "the window widths disagree"
    m = min(n, 40)
    assert (keys[0][:m] == fb.xy64_rows(fb.expect_points(c, fb.tau_powers(c, tau, m)))).all()
    host_key = keys[0].copy()      # a pageable host array of n valid points
    del keys

    def generate():
        h = ctypes.c_uint64(0)
        check(L.nmx_bases_generate(CID, 1, n, 0, ctypes.byref(h)))
        check(L.nmx_bases_unregister(h.value))

    def register():
        h = ctypes.c_uint64(0)
        check(L.nmx_bases_register(CID, host_key.ctypes.data, n, _lib.BASES_VALIDATE, ctypes.byref(h)))
        check(L.nmx_bases_unregister(h.value))
    paths = {"tau_c%d" % cw: (lambda cw=cw: tau_key(cw)) for cw in WIDTHS}
    paths["generate"] = generate
    paths["register"] = register
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
    check(L.nmx_set_option(b"fixed_base_c", 8))
    out = {"log_n": log_n}
    for k in paths:
        out[k] = stats([x for blk in t[k] for x in blk])
        out[k]["block_medians"] = [statistics.median(blk) for blk in t[k]]
        out[k]["spread"] = max(out[k]["block_medians"]) - min(out[k]["block_medians"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,20")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from nova_amd import _lib
    assert _lib.lib().nmx_init(0) == 0, _lib.lib().nmx_last_error().decode()
    rows = [run_size(int(x), a.reps, a.blocks, a.warmup) for x in a.logs.split(",")]
    print(f"{'n':>6} {'path':>9} {'median ms':>10} {'[p10, p90]':>20} {'block medians':>46} {'spread':>8}")
    for row in rows:
        for k, m in row.items():
            if k == "log_n":
                continue
            print(f"{'2^%d' % row['log_n']:>6} {k:>9} {m['median']:>10.4f} {'[%.4f, %.4f]' % (m['p10'], m['p90']):>20} "
                  f"{' '.join('%.4f' % x for x in m['block_medians']):>46} {m['spread']:>8.4f}")
    print(json.dumps({"bench": "fixed_base", "curve": "BN254_G1", "rows": rows}))


if __name__ == "__main__":
    main()
