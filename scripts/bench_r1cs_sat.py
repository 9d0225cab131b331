"""nmx_r1cs_is_sat against the path a caller had to compose before it existed, in ONE process, alternating.

  new        nmx_r1cs_is_sat, relaxed, HBM operands (W, E resident): the full call, and the equation-only form (ck_handle = 0)
  composed   nmx_field_concat -> nmx_r1cs_cross_term with E -> D2H of T -> numpy.any on the host -> nmx_commit twice in sequence
             (every call of it exists without nmx_r1cs_is_sat); its equation half alone is the yardstick of the equation-only form
  kernels    k_r1cs_sat against k_launch<SpmvCrossFn> on the same matrices: device events (nmx_set_profiling) here, and the kernel
             trace of `--kernels-only` under `rocprofv3 --kernel-trace --stats` in a run of its own

Instances: tests/fv_common.random_csr matrices (<= 8 entries a row, one 40-entry row), random W, X, u, E := Az o Bz - u Cz computed on
the device (as bench.py's Spartan replay does), expected commitments from nmx_commit; every timed call must answer "satisfied".
Every shape is warmed up first; times are a host clock around synchronous calls.  Prints a table and one JSON line.

  python scripts/bench_r1cs_sat.py                      # BN254 2^20 and Grumpkin 2^14, 20 repetitions
  python scripts/bench_r1cs_sat.py --sizes 0:12 --reps 5
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_r1cs_sat.py --kernels-only
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
    """entries whose 32-byte coefficient is read: everything but +-1 .. +-7 (fieldvec.hip: those ride in the index word)"""
    d = np.ascontiguousarray(data).reshape(-1, 32)
    small = (~d[:, 1:].any(axis=1)) & (d[:, 0] >= 1) & (d[:, 0] <= 7)
    neg = np.zeros(len(d), bool)
    for k in range(1, 8):
        neg |= (d == np.frombuffer((p - k).to_bytes(32, "little"), np.uint8)).all(axis=1)
    return int(len(d) - small.sum() - neg.sum())


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]
    return {"median": statistics.median(s), "min": s[0], "max": s[-1], "p10": q(0.1), "p90": q(0.9), "n": len(s)}


def run_size(cid, lg, reps, warm, kernels_only):
    import torch
    import nova_amd
    from nova_amd import _lib, fieldvec as fv
    from tests import fv_common as C
    from tests import util
    L = _lib.lib()
    fid = fv.SCALAR_FIELD_OF_CURVE[cid]
    p = C.FIELDS[fid]
    n = 1 << lg
    rows = cols = n
    n_io = 2
    n_w = cols - 1 - n_io
    csr = [C.random_csr(fid, rows, cols, 1000 + 10 * j + lg) for j in range(3)]
    mats = [fv.SparseMatrix(fid, ip, ix, dt, cols) for ip, ix, dt in csr]
    nnz = sum(int(ip[-1]) for ip, _ix, _dt in csr)
    full = sum(full_width_coefficients(dt, p) for _ip, _ix, dt in csr)
    alg_bytes = 4 * nnz + 32 * full + 32 * nnz + 32 * rows
    hW, X, u = C.rand_vec(fid, n_w, 7 + lg).copy(), C.rand_vec(fid, n_io, 8 + lg).copy(), C.rand_vec(fid, 1, 9 + lg).copy()
    rW, rE = C.rand_vec(fid, 1, 10 + lg).copy(), C.rand_vec(fid, 1, 11 + lg).copy()
    dW = torch.from_numpy(hW).cuda()
    torch.cuda.synchronize()
    z = fv.concat(fid, [dW, u, X])
    dE = fv.r1cs_cross_term(mats[0], mats[1], mats[2], z, None, torch.zeros((rows, 32), dtype=torch.uint8, device="cuda"), u)
    ck = None if kernels_only else nova_amd.CommitmentKey.generate(cid, n, k0=1)  # with window tables
    ce = nova_amd.CommitmentEngine(cid)
    if ck is not None:
        cw, cE = ce.commit(ck, dW, rW), ce.commit(ck, dE, rE)

    def new(with_ck):
        r = fv.r1cs_is_sat_relaxed(mats[0], mats[1], mats[2], ck if with_ck else None, dW, dE, u, X, cw if with_ck else None,
                                   cE if with_ck else None, rW, rE)
        assert r.ok and r.bad_rows == 0, repr(r)

    def composed(with_ck):
        zz = fv.concat(fid, [dW, u, X])
        T = fv.r1cs_cross_term(mats[0], mats[1], mats[2], zz, None, dE, u)
        assert not T.cpu().numpy().any()
        if with_ck:
            a, b = ce.commit(ck, dW, rW), ce.commit(ck, dE, rE)
            assert (a.xy, a.is_inf, b.xy, b.is_inf) == (cw.xy, cw.is_inf, cE.xy, cE.is_inf)

    def kernel_ms(fn):
        buf = (ctypes.c_float * 4)()
        fn()
        assert L.nmx_profile_last(buf, 4) >= 1
        return buf[0]

    variants = [("new_eq_only", lambda: new(False)), ("composed_eq_only", lambda: composed(False))]
    if not kernels_only:
        variants = [("new", lambda: new(True)), ("composed", lambda: composed(True))] + variants
    for _ in range(warm):
        for _name, fn in variants:
            fn()
    times = {name: [] for name, _ in variants}
    for _ in range(reps):  # alternating
        for name, fn in variants:
            t = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t) * 1e3)
    # the kernel pair by device events, alternating as well
    L.nmx_set_profiling(1)
    kt = {"k_r1cs_sat": [], "SpmvCrossFn": []}
    for _ in range(reps):
        kt["k_r1cs_sat"].append(kernel_ms(lambda: new(False)))
        kt["SpmvCrossFn"].append(kernel_ms(lambda: fv.r1cs_cross_term(mats[0], mats[1], mats[2], z, None, dE, u)))
    L.nmx_set_profiling(0)
    out = {"curve": nova_amd.CURVE_NAMES[cid] if hasattr(nova_amd, "CURVE_NAMES") else cid, "log2_rows": lg, "rows": rows, "cols": cols, "nnz": nnz,
           "full_width_coefficients": full, "algorithmic_bytes": alg_bytes,
           "call_ms": {k: stats(v) for k, v in times.items()}, "kernel_ms": {k: stats(v) for k, v in kt.items()}}
    k_med = out["kernel_ms"]["k_r1cs_sat"]["median"]
    out["k_r1cs_sat_GBs"] = alg_bytes / (k_med * 1e-3) / 1e9
    out["k_r1cs_sat_share_of_hbm_peak"] = out["k_r1cs_sat_GBs"] / HBM_PEAK_GBS  # a latency-bound gather: algorithmic bytes over kernel time
    acc = {}
    for a, b in (("new", "composed"), ("new_eq_only", "composed_eq_only")):
        if a in times:
            spread = out["call_ms"][b]["p90"] - out["call_ms"][b]["p10"]
            acc[a] = {"spread_of_composed_ms": spread, "ok": out["call_ms"][a]["median"] <= out["call_ms"][b]["median"] + spread}
    ks = out["kernel_ms"]["SpmvCrossFn"]["p90"] - out["kernel_ms"]["SpmvCrossFn"]["p10"]
    acc["kernel"] = {"spread_of_SpmvCrossFn_ms": ks, "ok": k_med <= out["kernel_ms"]["SpmvCrossFn"]["median"] + ks}
    out["acceptance"] = acc
    for m in mats:
        m.close()
    if ck is not None:
        ck.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="0:20,1:14", help="curve:log2(rows) pairs; curve 0 = BN254, 1 = Grumpkin, 2 = Pallas, 3 = Vesta")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true", help="no key, no commitments: the run to put under rocprofv3 --kernel-trace --stats")
    args = ap.parse_args()
    from nova_amd import _lib
    L = _lib.lib()
    rc = L.nmx_init(0)
    assert rc == 0, L.nmx_last_error().decode()  # (no device: this is a measurement, it does not fall back)
    results = []
    for item in args.sizes.split(","):
        cid, lg = (int(x) for x in item.split(":"))
        r = run_size(cid, lg, args.reps, args.warmup, args.kernels_only)
        results.append(r)
        print(f"{r['curve']} rows = cols = 2^{lg}  nnz {r['nnz']}  algorithmic bytes {r['algorithmic_bytes']}", flush=True)
        for k, v in list(r["call_ms"].items()) + [("kernel " + k, v) for k, v in r["kernel_ms"].items()]:
            print(f"  {k:24s} median {v['median']:8.4f} ms   min {v['min']:8.4f}   p10 {v['p10']:8.4f}   p90 {v['p90']:8.4f}   max {v['max']:8.4f}   (n = {v['n']})", flush=True)
        print(f"  k_r1cs_sat: {r['k_r1cs_sat_GBs']:.1f} GB/s of algorithmic bytes = {100 * r['k_r1cs_sat_share_of_hbm_peak']:.2f} % of the HBM peak (latency-bound gather)")
        print(f"  acceptance: {json.dumps(r['acceptance'])}", flush=True)
    print(json.dumps({"bench": "r1cs_sat", "reps": args.reps, "results": results}))


if __name__ == "__main__":
    main()
