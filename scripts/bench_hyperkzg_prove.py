"""nmx_hyperkzg_prove against the composed sequence of the calls that existed before it, and the fused quotient pass against
lincomb_powers + 3 x suffix Horner, on BN254 (scalar field Fr), HBM operands, in ONE process, alternating.

  (a) prove      nmx_hyperkzg_prove                                              one call
      composed   nmx_poly_fold_chain, nmx_msm_batch_handle, nmx_poly_eval_multi, nmx_field_lincomb_powers, 3 x nmx_poly_suffix_horner,
                 nmx_msm_batch_handle with the same SHA3 transcript squeezed in between, raw C calls over buffers allocated once
  (b) fused      nmx_poly_lincomb_quotients on prove's shape (n, n/2, ..., 2; three points), under every value of its two options
      division   nmx_field_lincomb_powers + 3 x nmx_poly_suffix_horner
      d2d        a device-to-device copy moving the pass's algorithmic bytes (2n elements read on average, 3n written: 2.5n copied)

Times are a host clock around synchronous calls.  Each is a median with its p10 / p90.  Two conditions are checked and printed:
"prove_not_slower": prove's median is not above composed's by more than composed's own p90 - p10; "fused_not_slower": likewise for (b), for the default options (4 coefficients per lane, B stored).
Prints a table and one JSON line.  No kernel trace is taken here.

  python scripts/bench_hyperkzg_prove.py                    # ell = 14 and 20, 7 repetitions
  python scripts/bench_hyperkzg_prove.py --ells 10 --reps 3
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CID, FID = 0, 1      # BN254 G1, BN254_FR
HBM_PEAK_GBS = 8000  # MI355X datasheet peak, GB/s


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    return {"median": statistics.median(s), "min": s[0], "max": s[-1], "p10": q(0.1), "p90": q(0.9), "n": len(s)}


def run_ell(ell, reps, warm):
    import numpy as np
    import torch
    import nova_amd
    from nova_amd import _lib
    from tests import fv_common as fc
    from tests import hyperkzg_common as hk
    lib = _lib.lib()
    n, p = 1 << ell, fc.FIELDS[FID]
    ck = nova_amd.CommitmentKey.generate(CID, n, k0=7)
    dev = lambda m, seed: torch.from_numpy(fc.rand_vec(FID, m, seed).copy()).cuda()  # noqa: E731
    empty = lambda m: torch.empty((max(m, 1), 32), dtype=torch.uint8, device="cuda")  # noqa: E731
    hat_P, point = dev(n, 1), fc.rand_vec(FID, ell, 2).copy()
    xs = np.ascontiguousarray(point[::-1][:ell - 1])
    folds = [empty(n >> i) for i in range(1, ell)]
    polys = [hat_P] + folds
    B, quot = empty(n), [empty(n) for _ in range(3)]
    DEV = _lib.SCALARS_DEVICE
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    p_polys, p_lens = (vp * ell)(*[t.data_ptr() for t in polys]), (sz * ell)(*[n >> i for i in range(ell)])
    p_folds = (vp * max(ell - 1, 1))(*[t.data_ptr() for t in folds])
    p_quot = (vp * 3)(*[t.data_ptr() for t in quot])
    p_hs, l_hs = (vp * 3)(*[t.data_ptr() + 32 for t in quot]), (sz * 3)(n - 1, n - 1, n - 1)
    com, com_inf, v, w, w_inf = (np.zeros(k, np.uint8) for k in (64 * ell, ell, 96 * ell, 192, 3))
    ok = lambda rc: rc == 0 or (_ for _ in ()).throw(RuntimeError(lib.nmx_last_error().decode()))  # noqa: E731

    def callback(tr):
        def cb(_ctx, stage, data, count, is_inf, out):
            ch = tr.stage(stage, bytes(data[:(32 if stage == 1 else 64) * count]), count, bytes(is_inf[:count]) if is_inf else None)
            ctypes.memmove(out, ch, 32)
            return 0
        return _lib.KZG_TRANSCRIPT_FN(cb)

    def prove():
        cb = callback(hk.Sha3Transcript(p))
        ok(lib.nmx_hyperkzg_prove(ck.handle, hat_P.data_ptr(), n, point.ctypes.data, DEV, cb, None, com.ctypes.data, com_inf.ctypes.data,
                                  v.ctypes.data, w.ctypes.data, w_inf.ctypes.data))
        return com[:64 * (ell - 1)].tobytes(), v.tobytes(), w.tobytes()

    def quotients_composed(q, us):
        ok(lib.nmx_field_lincomb_powers(FID, p_polys, p_lens, ell, q, n, DEV, B.data_ptr()))
        for j in range(3):
            ok(lib.nmx_poly_suffix_horner(FID, B.data_ptr(), n, us + 32 * j, DEV, quot[j].data_ptr()))

    def composed():
        tr = hk.Sha3Transcript(p)
        if ell > 1:
            ok(lib.nmx_poly_fold_chain(FID, hat_P.data_ptr(), n, xs.ctypes.data, ell - 1, DEV | _lib.ASYNC, p_folds))
            ok(lib.nmx_msm_batch_handle(ck.handle, p_folds, (sz * (ell - 1))(*[n >> i for i in range(1, ell)]), ell - 1, DEV, com.ctypes.data, com_inf.ctypes.data))
        r = tr.decode(tr.stage(0, com[:64 * (ell - 1)].tobytes(), ell - 1, com_inf[:ell - 1].tobytes()))
        us = fc.vec([r, (-r) % p, r * r % p]).copy()
        ok(lib.nmx_poly_eval_multi(FID, p_polys, p_lens, ell, us.ctypes.data, 3, DEV, v.ctypes.data))
        q = np.frombuffer(tr.stage(1, v.tobytes(), 3 * ell, None), np.uint8).copy()
        quotients_composed(q.ctypes.data, us.ctypes.data)
        ok(lib.nmx_msm_batch_handle(ck.handle, p_hs, l_hs, 3, DEV, w.ctypes.data, w_inf.ctypes.data))
        tr.stage(2, w.tobytes(), 3, w_inf.tobytes())
        return com[:64 * (ell - 1)].tobytes(), v.tobytes(), w.tobytes()

    assert prove() == composed(), "the one call and the composed sequence disagree"
    qv, uv = fc.rand_vec(FID, 1, 3).copy(), fc.rand_vec(FID, 3, 4).copy()

    def fused(chunk, scratch):
        def run():
            ok(lib.nmx_poly_lincomb_quotients(FID, p_polys, p_lens, ell, qv.ctypes.data, uv.ctypes.data, 3, DEV, p_quot))
        return chunk, scratch, run
    n_copy = (5 * n) // 2
    src, dst = empty(n_copy), empty(n_copy)
    paths = {"prove": prove, "composed": composed, "division": lambda: quotients_composed(qv.ctypes.data, uv.ctypes.data),
             "d2d": lambda: (dst.copy_(src), torch.cuda.synchronize())}
    variants = {"fused_c%d_s%d" % (c, s): fused(c, s) for c in (4, 8) for s in (1, 0)}
    t = {k: [] for k in list(paths) + list(variants)}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3
    for it in range(warm + reps):
        for k, fn in paths.items():
            ms = timed(fn)
            if it >= warm:
                t[k].append(ms)
        for k, (chunk, scratch, fn) in variants.items():
            ok(lib.nmx_set_option(b"kzg_quot_chunk", chunk)), ok(lib.nmx_set_option(b"kzg_quot_scratch", scratch))
            ms = timed(fn)
            if it >= warm:
                t[k].append(ms)
        ok(lib.nmx_set_option(b"kzg_quot_chunk", 0)), ok(lib.nmx_set_option(b"kzg_quot_scratch", 1))
    row = {"ell": ell, "ms": {k: stats(x) for k, x in t.items()}}
    row["gbs"] = {k: 5 * 32 * n / row["ms"][k]["median"] / 1e6 for k in list(variants) + ["division", "d2d"]}
    spread = lambda k: row["ms"][k]["p90"] - row["ms"][k]["p10"]  # noqa: E731
    row["prove_not_slower"] = bool(row["ms"]["prove"]["median"] <= row["ms"]["composed"]["median"] + spread("composed"))
    row["fused_not_slower"] = bool(row["ms"]["fused_c4_s1"]["median"] <= row["ms"]["division"]["median"] + spread("division"))
    ck.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ells", default="14,20")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from nova_amd import _lib
    assert _lib.lib().nmx_init(0) == 0, _lib.lib().nmx_last_error().decode()
    rows = [run_ell(int(e), a.reps, a.warmup) for e in a.ells.split(",")]
    print(f"{'ell':>4} {'path':>14} {'median ms':>10} {'[p10, p90]':>20} {'GB/s (5n x 32 B)':>17}")
    for r in rows:
        for k, m in r["ms"].items():
            g = r["gbs"].get(k)
            print(f"{r['ell']:>4} {k:>14} {m['median']:>10.4f} {'[%.4f, %.4f]' % (m['p10'], m['p90']):>20} {('%.0f' % g) if g else '':>17}")
        print(f"{r['ell']:>4} prove not slower than composed: {r['prove_not_slower']}; fused pass not slower than the composed division: {r['fused_not_slower']}")
    print(json.dumps({"bench": "hyperkzg_prove", "curve": "bn254_g1", "hbm_peak_gbs": HBM_PEAK_GBS, "rows": rows}))


if __name__ == "__main__":
    main()
