"""nmx_r1cs_evaluate against the path a caller had to compose before it existed, in ONE process, alternating.

  new        nmx_r1cs_evaluate over the three resident matrices (RelaxedR1CSSNARK::verify's multi_evaluate, spartan/snark.rs:325-353)
  composed   nmx_eq_evals_from_points(r_x) into HBM -> nmx_spmv_apply_many(transposed = 1) -> nmx_mle_multi_evaluate(.., r_y), every
             entry point as it is without the new call.  The transposed forms are built by a first call that is timed on its own
             ("composed_first_call_ms") and is not part of the mean.

Shapes: bench.py's spartan_like_matrices (num_cons = num_vars = n, columns [0, n + 2) of 2 n, the constant column in one row in
eight of A), three matrices, ell_x = log2 n, ell_y = log2 n + 1.  Both paths must give the same three values in every repetition.
Times are a host clock around synchronous calls after a warm-up; the new call's device time (tables + pass + finish) comes from
nmx_set_profiling's events.  Algorithmic bytes of the new path: indptr, the index words, the coefficients that are read (every entry
that is not +-1 .. +-7), one 32-byte T_y gather per entry, the two T_x halves per row.

  python scripts/bench_r1cs_evaluate.py                       # BN254 Fr and Grumpkin's scalar field at 2^14 and 2^20, 20 alternations
  python scripts/bench_r1cs_evaluate.py --sizes 1:12 --reps 5
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_r1cs_evaluate.py --new-only
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E, spec


def full_width_coefficients(data, p):
    """entries whose 32-byte coefficient is read: everything but +-1 .. +-7 (those ride in the index word)"""
    d = np.ascontiguousarray(data).reshape(-1, 32)
    small = (~d[:, 1:].any(axis=1)) & (d[:, 0] >= 1) & (d[:, 0] <= 7)
    neg = np.zeros(len(d), bool)
    for k in range(1, 8):
        neg |= (d == np.frombuffer((p - k).to_bytes(32, "little"), np.uint8)).all(axis=1)
    return int(len(d) - small.sum() - neg.sum())


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    return {"median": statistics.median(s), "min": s[0], "max": s[-1], "p10": q(0.1), "p90": q(0.9), "n": len(s)}


def run_size(fid, lg, reps, warm, new_only):
    import bench
    from nova_amd import _lib, fieldvec as fv
    from tests import fv_common as C
    L = _lib.lib()
    p = C.FIELDS[fid]
    n = 1 << lg
    csr = bench.spartan_like_matrices(fid, n, seed=700 + lg)
    mats = [fv.SparseMatrix(fid, ip, ix, dt, 2 * n) for ip, ix, dt in csr]
    nnz = sum(int(ip[-1]) for ip, _ix, _dt in csr)
    full = sum(full_width_coefficients(dt, p) for _ip, _ix, dt in csr)
    alg_bytes = 3 * 4 * (n + 1) + 4 * nnz + 32 * full + 32 * nnz + 3 * 64 * n
    r_x, r_y = C.rand_vec(fid, lg, 5 + lg).copy(), C.rand_vec(fid, lg + 1, 6 + lg).copy()

    def new():
        return fv.r1cs_evaluate(mats, r_x, r_y)

    def composed():
        T_x = fv.eq_evals_from_points(fid, r_x, device=True)
        return fv.mle_multi_evaluate(fid, fv.multiply_vec_many(mats, T_x, transposed=True), r_y)

    want = new()
    first = None
    variants = [("new", new)]
    if not new_only:
        t = time.perf_counter()
        assert composed() == want
        first = (time.perf_counter() - t) * 1e3  # builds the three transposed forms
        variants.append(("composed", composed))
    for _ in range(warm):
        for _name, fn in variants:
            fn()
    times = {name: [] for name, _ in variants}
    for _ in range(reps):  # alternating
        for name, fn in variants:
            t = time.perf_counter()
            got = fn()
            times[name].append((time.perf_counter() - t) * 1e3)
            assert got == want, name
    L.nmx_set_profiling(1)
    dev = []
    buf = (ctypes.c_float * 4)()
    for _ in range(reps):
        new()
        assert L.nmx_profile_last(buf, 4) >= 1
        dev.append(buf[0])
    L.nmx_set_profiling(0)
    out = {"field": fid, "log2_rows": lg, "rows": n, "cols": 2 * n, "nnz": nnz, "full_width_coefficients": full, "algorithmic_bytes": alg_bytes,
           "call_ms": {k: stats(v) for k, v in times.items()}, "new_device_ms": stats(dev), "composed_first_call_ms": first}
    d_med = out["new_device_ms"]["median"]
    out["new_GBs"] = alg_bytes / (d_med * 1e-3) / 1e9
    out["new_share_of_hbm_peak"] = out["new_GBs"] / HBM_PEAK_GBS
    if not new_only:
        spread = max(out["call_ms"][k]["p90"] - out["call_ms"][k]["p10"] for k in ("new", "composed"))
        out["acceptance"] = {"spread_ms": spread, "ok": out["call_ms"]["new"]["median"] <= out["call_ms"]["composed"]["median"] + spread}
    for m in mats:
        m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1:14,0:14,1:20,0:20", help="field:log2(num_cons) pairs; field 1 = BN254 Fr, 0 = BN254 Fq = Grumpkin's scalar field")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--new-only", action="store_true", help="the new call alone: the run to put under rocprofv3 --kernel-trace --stats")
    args = ap.parse_args()
    from nova_amd import _lib
    L = _lib.lib()
    rc = L.nmx_init(0)
    assert rc == 0, L.nmx_last_error().decode()  # (no device: this is a measurement, it does not fall back)
    results = []
    for item in args.sizes.split(","):
        fid, lg = (int(x) for x in item.split(":"))
        r = run_size(fid, lg, args.reps, args.warmup, args.new_only)
        results.append(r)
        print(f"field {fid} num_cons = num_vars = 2^{lg}  nnz {r['nnz']}  full-width coefficients {r['full_width_coefficients']}  "
              f"algorithmic bytes {r['algorithmic_bytes']}", flush=True)
        for k, v in list(r["call_ms"].items()) + [("new, device events", r["new_device_ms"])]:
            print(f"  {k:20s} median {v['median']:8.4f} ms   min {v['min']:8.4f}   p10 {v['p10']:8.4f}   p90 {v['p90']:8.4f}   max {v['max']:8.4f}   (n = {v['n']})", flush=True)
        if r["composed_first_call_ms"] is not None:
            print(f"  composed, first call (builds the transposed forms): {r['composed_first_call_ms']:.3f} ms")
        print(f"  new: {r['new_GBs']:.1f} GB/s of algorithmic bytes = {100 * r['new_share_of_hbm_peak']:.2f} % of the HBM peak")
        if "acceptance" in r:
            print(f"  acceptance: {json.dumps(r['acceptance'])}", flush=True)
    print(json.dumps({"bench": "r1cs_evaluate", "reps": args.reps, "results": results}))


if __name__ == "__main__":
    main()
