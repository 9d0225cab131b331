"""nmx_bases_fold / nmx_bases_scale / nmx_bases_concat against the paths they replace -- ONE process, the paths alternating.

  fold_hbm / scale_hbm   nmx_bases_fold / nmx_bases_scale over the whole key, no window tables for the result: the launch, the wait, unregister
  fold_host / scale_host what a caller pays without them: nmx_bases_read of the source, the oracle's two-point / one-point multiplication per
                         output (oracle/cref.py ref_msm with n = 2 / n = 1, what the reference runs inside par_iter) on `--threads` host
                         threads, nmx_bases_register of the result (no window tables), unregister.  The three parts are also timed apart
  concat_hbm             nmx_bases_concat of the whole key (k = 1), no window tables, unregister
  d2d_copy               hipMemcpy device to device of the same bytes between two torch buffers, and the wait

BN254 G1, a key made by nmx_bases_generate, random weights.  Before anything is timed the HBM results are compared byte for byte with the host
path's.  Times are a host clock around synchronous calls.  The repetitions run in `--blocks` blocks; within a block the paths alternate; a
path whose block has used `--step-seconds` stops repeating in that block (at least one repetition), and a step that does not return within
`--hang-seconds` ends the process.  Reported per path: the median over all repetitions with [p10, p90], the median of every block, and the
spread (highest minus lowest block median).  For the two kernels also the modular products per second, from the operation counts of the
digit stream (doublings 9 products, mixed additions 10, a block normalisation 8 per lane; nova_amd/csrc/key_ext.hpp).  Prints a table and one
JSON line.  No threshold rests on these numbers.  NOT done here: no kernel trace, nothing tuned.

  python scripts/bench_key_ext.py                         # keys of 2^14 and 2^20 points, 3 blocks of 4 repetitions
  python scripts/bench_key_ext.py --log-n 10 --reps 2 --blocks 2
"""
import argparse
import ctypes
import faulthandler
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CID = 0              # BN254 G1
R_BN254 = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    return {"median": statistics.median(s), "min": s[0], "max": s[-1], "p10": q(0.1), "p90": q(0.9), "n": len(s)}


def jsf_counts(a, b):
    """(positions, non-zero positions) of Solinas' joint sparse form of (a, b): what ke_recode (key_ext.hpp) produces"""
    d, pos, nz = [0, 0], 0, 0
    k = [a, b]
    while k[0] + d[0] or k[1] + d[1]:
        ell = [(k[i] + d[i]) & 7 for i in range(2)]
        u = [0, 0]
        for i in range(2):
            if ell[i] & 1:
                u[i] = 2 - (ell[i] & 3)
                if ell[i] in (3, 5) and (ell[1 - i] & 3) == 2:
                    u[i] = -u[i]
        for i in range(2):
            if 2 * d[i] == 1 + u[i]:
                d[i] = 1 - d[i]
            k[i] >>= 1
        pos += 1
        nz += 1 if (u[0] or u[1]) else 0
    return pos, nz


def run_case(log_n, reps, blocks, warm, threads, step_seconds, hang_seconds):
    import numpy as np
    import torch
    from nova_amd import _lib
    from oracle import cref
    L, C = _lib.lib(), cref.lib()
    cref.set_threads(1)       # every oracle call serial inside: the parallelism is the pool's, one output per call, as par_iter's is
    n, h = 1 << log_n, 1 << (log_n - 1)
    rng = np.random.default_rng(log_n)
    w1, w2, r = (int.from_bytes(rng.bytes(40), "little") % R_BN254 for _ in range(3))
    wb = {k: np.frombuffer(int(v).to_bytes(32, "little"), np.uint8).copy() for k, v in (("w1", w1), ("w2", w2), ("r", r))}

    def check(rc):
        assert rc == 0, L.nmx_last_error().decode()
    src = ctypes.c_uint64(0)
    check(L.nmx_bases_generate(CID, 1, n, 0, ctypes.byref(src)))
    rows = np.zeros((n, 64), np.uint8)
    pool = ThreadPoolExecutor(threads)
    parts = {}

    def hbm(kind, keep=False):
        hd = ctypes.c_uint64(0)
        if kind == "fold":
            check(L.nmx_bases_fold(src.value, 0, n, wb["w1"].ctypes.data, wb["w2"].ctypes.data, 0, ctypes.byref(hd)))
        elif kind == "scale":
            check(L.nmx_bases_scale(src.value, 0, n, wb["r"].ctypes.data, 0, ctypes.byref(hd)))
        else:
            hs, ln = (ctypes.c_uint64 * 1)(src.value), (ctypes.c_size_t * 1)(n)
            check(L.nmx_bases_concat(hs, None, ln, 1, 0, ctypes.byref(hd)))
        if keep:
            return hd.value
        check(L.nmx_bases_unregister(hd.value))

    def host(kind, keep=False):
        t0 = time.perf_counter()
        check(L.nmx_bases_read(src.value, 0, n, rows.ctypes.data))
        t1 = time.perf_counter()
        if kind == "fold":
            m, k = h, 2
            pairs = np.ascontiguousarray(np.stack([rows[:h], rows[h:2 * h]], axis=1))     # (h, 2, 64): L[i] next to R[i]
            sc = np.concatenate([wb["w1"], wb["w2"]])
        else:
            m, k, pairs, sc = n, 1, rows, wb["r"]
        out, inf = np.zeros((m, 64), np.uint8), np.zeros(m, np.uint8)
        bp, op, ip, sp, f = pairs.ctypes.data, out.ctypes.data, inf.ctypes.data, sc.ctypes.data, C.ref_msm

        def chunk(lo, hi):
            for i in range(lo, hi):
                f(CID, sp, bp + 64 * k * i, k, op + 64 * i, ip + i)
        step = (m + threads - 1) // threads
        list(pool.map(lambda t: chunk(t * step, min(m, (t + 1) * step)), range(threads)))
        t2 = time.perf_counter()
        hd = ctypes.c_uint64(0)
        check(L.nmx_bases_register(CID, out.ctypes.data, m, 0, ctypes.byref(hd)))
        t3 = time.perf_counter()
        for name, dt in (("read", t1 - t0), ("mul", t2 - t1), ("register", t3 - t2)):
            parts.setdefault(kind + "_host_" + name, []).append(dt * 1e3)
        if keep:
            return hd.value, out
        check(L.nmx_bases_unregister(hd.value))

    a_dev = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    b_dev = torch.empty(n * 64, dtype=torch.uint8, device="cuda")

    def d2d():
        b_dev.copy_(a_dev)
        torch.cuda.synchronize()

    # correctness first: the HBM results are the host path's, byte for byte
    faulthandler.dump_traceback_later(hang_seconds, exit=True)
    for kind, m in (("fold", h), ("scale", n)):
        hh, want = host(kind, keep=True)
        hd = hbm(kind, keep=True)
        got = np.zeros((m, 64), np.uint8)
        check(L.nmx_bases_read(hd, 0, m, got.ctypes.data))
        assert (got == want).all(), kind + ": the HBM result differs from the host path's"
        check(L.nmx_bases_unregister(hh))
        check(L.nmx_bases_unregister(hd))
    hd = hbm("concat", keep=True)
    got = np.zeros((n, 64), np.uint8)
    check(L.nmx_bases_read(hd, 0, n, got.ctypes.data))
    assert (got == rows).all(), "concat: the copy differs from the source"
    check(L.nmx_bases_unregister(hd))
    parts.clear()

    paths = {"fold_hbm": lambda: hbm("fold"), "fold_host": lambda: host("fold"), "scale_hbm": lambda: hbm("scale"), "scale_host": lambda: host("scale"),
             "concat_hbm": lambda: hbm("concat"), "d2d_copy": d2d}
    for _ in range(warm):
        for name, fn in paths.items():
            if not name.endswith("_host"):          # (the host paths ran once above)
                faulthandler.dump_traceback_later(hang_seconds, exit=True)
                fn()
    t = {k: [[] for _ in range(blocks)] for k in paths}
    for blk in range(blocks):
        for _ in range(reps):
            for k, fn in paths.items():
                if t[k][blk] and sum(t[k][blk]) > step_seconds * 1e3:
                    continue
                faulthandler.dump_traceback_later(hang_seconds, exit=True)
                t0 = time.perf_counter()
                fn()
                t[k][blk].append((time.perf_counter() - t0) * 1e3)
    faulthandler.cancel_dump_traceback_later()
    check(L.nmx_bases_unregister(src.value))
    pool.shutdown()
    out = {"log_n": log_n, "threads": threads}
    for k in paths:
        out[k] = stats([x for blk in t[k] for x in blk])
        out[k]["block_medians"] = [statistics.median(blk) for blk in t[k]]
        out[k]["spread"] = max(out[k]["block_medians"]) - min(out[k]["block_medians"])
    for k, v in parts.items():
        out[k] = {"median": statistics.median(v), "n": len(v)}
    # modular products: (positions - 1) doublings of 9, one mixed addition of 10 per non-zero position, and per lane of a block
    # normalisation 8; a pair also forms S and D (2 additions) and normalises them (2 more normalisations)
    pf, jf = jsf_counts(w1, w2)
    ps, js = jsf_counts(r, 0)
    out["fold_products_per_output"] = 9 * (pf - 1) + 10 * (jf + 2) + 8 * 3
    out["scale_products_per_output"] = 9 * (ps - 1) + 10 * js + 8
    out["fold_digits"], out["scale_digits"] = [pf, jf], [ps, js]
    out["fold_gmodmul_per_s"] = out["fold_products_per_output"] * h / (out["fold_hbm"]["median"] * 1e-3) / 1e9
    out["scale_gmodmul_per_s"] = out["scale_products_per_output"] * n / (out["scale_hbm"]["median"] * 1e-3) / 1e9
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="*", default=[14, 20])
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    ap.add_argument("--step-seconds", type=float, default=8.0, help="a path stops repeating inside a block once it has used this much")
    ap.add_argument("--hang-seconds", type=float, default=150.0, help="a single step that takes longer ends the process")
    a = ap.parse_args()
    from nova_amd import _lib
    assert _lib.lib().nmx_init(0) == 0, _lib.lib().nmx_last_error().decode()
    rows = [run_case(ln, a.reps, a.blocks, a.warmup, a.threads, a.step_seconds, a.hang_seconds) for ln in a.log_n]
    print(f"{'log n':>6} {'path':>20} {'median ms':>11} {'[p10, p90]':>24} {'block medians':>36} {'spread':>9} {'reps':>5}")
    for row in rows:
        for k, m in row.items():
            if isinstance(m, dict) and "block_medians" in m:
                print(f"{row['log_n']:>6} {k:>20} {m['median']:>11.4f} {'[%.4f, %.4f]' % (m['p10'], m['p90']):>24} "
                      f"{' '.join('%.3f' % x for x in m['block_medians']):>36} {m['spread']:>9.4f} {m['n']:>5}")
            elif isinstance(m, dict):
                print(f"{row['log_n']:>6} {k:>20} {m['median']:>11.4f} {'(part of the host path)':>24}")
        print(f"{row['log_n']:>6} fold: {row['fold_products_per_output']} products per output ({row['fold_digits'][0]} positions, {row['fold_digits'][1]} non-zero), "
              f"{row['fold_gmodmul_per_s']:.1f} G modmul/s; scale: {row['scale_products_per_output']} ({row['scale_digits'][0]}, {row['scale_digits'][1]}), "
              f"{row['scale_gmodmul_per_s']:.1f} G modmul/s; host multiplications on {row['threads']} threads")
    print(json.dumps({"bench": "key_ext", "curve": "BN254_G1", "rows": rows}))


if __name__ == "__main__":
    main()
