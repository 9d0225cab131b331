"""nmx_mercury_prove against the composed sequence of public calls, nmx_mercury_s_poly alone, and nmx_hyperkzg_prove at the same sizes as
context, on BN254 (scalar field Fr), HBM operands, in ONE process, alternating.

  prove      nmx_mercury_prove                                               one call; inside the timed region: everything, the SHA3
             transcript callback (Python) and the O(b) host algebra of the batch opening included
  composed   2 x nmx_eq_evals_from_points, nmx_mercury_h_poly, nmx_mercury_divide_by_binomial, nmx_mercury_s_poly, a device-side reversal of
             g, nmx_poly_eval_multi, nmx_field_lincomb_powers + nmx_poly_suffix_horner (quot_f), six nmx_msm_batch_handle calls with the same
             SHA3 transcript squeezed in between, the read-back of g, h, s and the upload of W and W'; raw C calls over buffers allocated
             once.  NOT inside its timed region: the O(b) algebra that makes W and W' -- they are taken from the one call's own first run
             (the transcript is deterministic, so they are the same polynomials), which favours `composed` by that host work
  s_poly     nmx_mercury_s_poly alone on the proof's (eq_col, g, eq_row, h) shape: b = 2^(ell / 2); 4 b (b - 1) / 2 products per call
  hyperkzg   nmx_hyperkzg_prove on the same polynomial, point and key

Times are a host clock around synchronous calls.  Each is a median with its p10 / p90.  "prove_not_slower": prove's median is not above
composed's by more than composed's own p90 - p10.  Prints a table and one JSON line.  No kernel trace is taken here.

  python scripts/bench_mercury_prove.py                    # ell = 14 and 20, 7 repetitions
  python scripts/bench_mercury_prove.py --ells 10 --reps 3
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
    from tests import mercury_common as MC
    from tests import mercury_prove_common as MP
    lib = _lib.lib()
    n, p = 1 << ell, fc.FIELDS[FID]
    log_b = (ell + 1) // 2
    b = 1 << log_b
    n_rows = n // b
    nq = (n_rows - 1) * b
    ck = nova_amd.CommitmentKey.generate(CID, n, k0=7)
    dev = lambda m, seed: torch.from_numpy(fc.rand_vec(FID, m, seed).copy()).cuda()  # noqa: E731
    empty = lambda m: torch.empty((max(m, 1), 32), dtype=torch.uint8, device="cuda")  # noqa: E731
    poly, point = dev(n, 1), fc.rand_vec(FID, ell, 2).copy()
    pt = np.concatenate([np.zeros((2 * log_b - ell, 32), np.uint8), point.reshape(-1, 32)])
    u_row, u_col = np.ascontiguousarray(pt[:log_b]), np.ascontiguousarray(pt[log_b:])
    eq_row, eq_col, h, g, s, d, q, B, quot, Wd, Wpd = (empty(m) for m in (b, b, b, b, b, b, nq, n, n, b, b))
    h.zero_()
    DEV = _lib.SCALARS_DEVICE
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    comms, infs, evals = np.zeros(512, np.uint8), np.zeros(8, np.uint8), np.zeros(192, np.uint8)
    ok = lambda rc: rc == 0 or (_ for _ in ()).throw(RuntimeError(lib.nmx_last_error().decode()))  # noqa: E731
    W_host = {}

    def callback(tr, scalars_at):
        def cb(_ctx, stage, data, count, is_inf, out):
            ch = tr.stage(stage, bytes(data[:(32 if stage == scalars_at else 64) * count]), count, bytes(is_inf[:count]) if is_inf else None)
            ctypes.memmove(out, ch, 32)
            return 0
        return _lib.KZG_TRANSCRIPT_FN(cb)

    def prove():
        cb = callback(hk.Sha3Transcript(p), 3)
        ok(lib.nmx_mercury_prove(ck.handle, poly.data_ptr(), n, point.ctypes.data, DEV, cb, None, comms.ctypes.data, infs.ctypes.data, evals.ctypes.data))
        return comms.tobytes(), evals.tobytes()

    def commit(vecs_lens):
        k = len(vecs_lens)
        out, oi = np.zeros(64 * k, np.uint8), np.zeros(k, np.uint8)
        ok(lib.nmx_msm_batch_handle(ck.handle, (vp * k)(*[t.data_ptr() + 32 * off for t, off, _m in vecs_lens]), (sz * k)(*[m for _t, _o, m in vecs_lens]), k, DEV,
                                    out.ctypes.data, oi.ctypes.data))
        return out.tobytes(), oi.tobytes()

    def composed():
        tr = hk.Sha3Transcript(p)
        out = [None] * 8
        ok(lib.nmx_eq_evals_from_points(FID, u_row.ctypes.data, log_b, DEV, eq_row.data_ptr()))
        ok(lib.nmx_eq_evals_from_points(FID, u_col.ctypes.data, log_b, DEV, eq_col.data_ptr()))
        ok(lib.nmx_mercury_h_poly(FID, poly.data_ptr(), n_rows, b, eq_col.data_ptr(), DEV | _lib.ASYNC, h.data_ptr()))
        out[0], i0 = commit([(h, 0, n_rows)])
        alpha = np.frombuffer(tr.stage(0, out[0], 1, i0), np.uint8).copy()
        ok(lib.nmx_mercury_divide_by_binomial(FID, poly.data_ptr(), n_rows, b, alpha.ctypes.data, DEV | _lib.ASYNC, q.data_ptr(), g.data_ptr()))
        c2, i2 = commit([(q, 0, nq), (g, 0, b)])
        out[2], out[1] = c2[:64], c2[64:]
        gamma = np.frombuffer(tr.stage(1, c2, 2, i2), np.uint8).copy()
        ok(lib.nmx_mercury_s_poly(FID, eq_col.data_ptr(), g.data_ptr(), eq_row.data_ptr(), h.data_ptr(), b, gamma.ctypes.data, DEV | _lib.ASYNC, s.data_ptr()))
        ok(lib.nmx_sync())
        d.copy_(torch.flip(g, dims=[0]))
        torch.cuda.synchronize()
        c3, i3 = commit([(s, 0, b - 1), (d, 0, b)])
        out[3], out[4] = c3[:64], c3[64:]
        zeta_b = tr.stage(2, c3, 2, i3)
        ze, al = tr.decode(zeta_b), tr.decode(alpha.tobytes())
        pts = fc.vec([ze, pow(ze, -1, p), al]).copy()
        ev = np.zeros(12 * 32, np.uint8)
        ok(lib.nmx_poly_eval_multi(FID, (vp * 4)(g.data_ptr(), h.data_ptr(), s.data_ptr(), d.data_ptr()), (sz * 4)(b, b, b - 1, b), 4, pts.ctypes.data, 3, DEV,
                                   ev.ctypes.data))
        e = ev.reshape(12, 32)
        six = b"".join(e[i].tobytes() for i in (0, 1, 3, 4, 6, 7))
        tr.stage(3, six, 6, None)
        ghs = [t.cpu() for t in (g, h, s)]                                     # what the batch opening reads back
        wq = fc.vec([(al - pow(ze, b, p)) % p]).copy()
        ok(lib.nmx_field_lincomb_powers(FID, (vp * 2)(poly.data_ptr(), q.data_ptr()), (sz * 2)(n, nq), 2, wq.ctypes.data, n, DEV, B.data_ptr()))
        ok(lib.nmx_poly_suffix_horner(FID, B.data_ptr(), n, pts.ctypes.data, DEV, quot.data_ptr()))
        out[5], i5 = commit([(quot, 1, n - 1)])
        tr.stage(4, out[5], 1, i5)
        Wd[:b - 1].copy_(W_host["W"], non_blocking=False)
        out[6], i6 = commit([(Wd, 0, b - 1)])
        tr.stage(5, out[6], 1, i6)
        Wpd[:b - 1].copy_(W_host["Wp"], non_blocking=False)
        out[7], i7 = commit([(Wpd, 0, b - 1)])
        tr.stage(6, out[7], 1, i7)
        del ghs
        return b"".join(out), six

    # W and W' for `composed`: the restated batch opening on the one call's own g, h, s and challenges (once, outside every timed region)
    first = prove()
    tr0 = hk.Sha3Transcript(p)
    W_host["W"] = W_host["Wp"] = torch.zeros((b - 1, 32), dtype=torch.uint8)
    composed()                                                                 # fills g, h, s, d with the proof's polynomials
    ints = lambda t: fc.ints(t.cpu().numpy())  # noqa: E731
    ch = {}
    for stage, idx in ((0, [0]), (1, [2, 1]), (2, [3, 4])):                     # the absorb order: comm_h; comm_q, comm_g; comm_s, comm_d
        ch[stage] = tr0.decode(tr0.stage(stage, b"".join(first[0][64 * i: 64 * i + 64] for i in idx), len(idx), bytes(len(idx))))
    tr0.stage(3, first[1], 6, None)
    beta = tr0.decode(tr0.stage(4, first[0][320:384], 1, bytes(1)))
    z = tr0.decode(tr0.stage(5, first[0][384:448], 1, bytes(1)))
    ze, al = ch[2], ch[0]
    gi, hi_, si = ints(g), ints(h), ints(s)[:b - 1]
    di = gi[::-1]
    E = lambda f, x: MC.UniPoly(f, p).evaluate(x)  # noqa: E731
    zi = pow(ze, -1, p)
    evd = {"g_zeta": E(gi, ze), "g_zeta_inv": E(gi, zi), "h_zeta": E(hi_, ze), "h_zeta_inv": E(hi_, zi), "h_alpha": E(hi_, al), "s_zeta": E(si, ze),
           "s_zeta_inv": E(si, zi), "d_zeta": E(di, ze), "zeta": ze, "zeta_inv": zi, "alpha": al}
    _, _, W, Wp = MP.generate_batch_evaluate_arg(p, lambda f: None, evd, (gi, hi_, si, di), beta, lambda cw: z)
    W_host["W"], W_host["Wp"] = torch.from_numpy(fc.vec(W).copy()), torch.from_numpy(fc.vec(Wp).copy())
    assert prove() == composed(), "the one call and the composed sequence disagree"

    gam = fc.rand_vec(FID, 1, 3).copy()

    def s_alone():
        ok(lib.nmx_mercury_s_poly(FID, eq_col.data_ptr(), g.data_ptr(), eq_row.data_ptr(), h.data_ptr(), b, gam.ctypes.data, DEV, s.data_ptr()))

    hcom, hinf, hv, hw, hwi = (np.zeros(k, np.uint8) for k in (64 * ell, ell, 96 * ell, 192, 3))

    def hyperkzg():
        cb = callback(hk.Sha3Transcript(p), 1)
        ok(lib.nmx_hyperkzg_prove(ck.handle, poly.data_ptr(), n, point.ctypes.data, DEV, cb, None, hcom.ctypes.data, hinf.ctypes.data, hv.ctypes.data,
                                  hw.ctypes.data, hwi.ctypes.data))

    paths = {"prove": prove, "composed": composed, "s_poly": s_alone, "hyperkzg": hyperkzg}
    t = {k: [] for k in paths}

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
    row = {"ell": ell, "b": b, "ms": {k: stats(x) for k, x in t.items()}}
    products = 4 * b * (b - 1) // 2
    row["s_poly_products"] = products
    row["s_poly_gproducts_per_s"] = products / row["ms"]["s_poly"]["median"] / 1e6
    row["s_poly_share_of_prove"] = row["ms"]["s_poly"]["median"] / row["ms"]["prove"]["median"]
    spread = row["ms"]["composed"]["p90"] - row["ms"]["composed"]["p10"]
    row["prove_not_slower"] = bool(row["ms"]["prove"]["median"] <= row["ms"]["composed"]["median"] + spread)
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
    print(f"{'ell':>4} {'path':>10} {'median ms':>10} {'[p10, p90]':>20}")
    for r in rows:
        for k, m in r["ms"].items():
            print(f"{r['ell']:>4} {k:>10} {m['median']:>10.4f} {'[%.4f, %.4f]' % (m['p10'], m['p90']):>20}")
        print(f"{r['ell']:>4} s_poly: b = {r['b']}, {r['s_poly_products']} products, {r['s_poly_gproducts_per_s']:.2f} G products/s, "
              f"{100 * r['s_poly_share_of_prove']:.1f} % of prove; prove not slower than composed: {r['prove_not_slower']}")
    print(json.dumps({"bench": "mercury_prove", "curve": "bn254_g1", "rows": rows}))


if __name__ == "__main__":
    main()
