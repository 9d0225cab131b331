"""When do the waves of one SIMD finish the segment accumulate?  Needs the measuring build of the library (NMX_HIPCC_FLAGS=-DNMX_ACCUM_TRACE
for __graft_entry__.build(), or capi.hip and the BN254 unit compiled with it and linked with the other objects; loaded through NMX_SO): lane 0 of every wave of k_launch<AccumSegFn> then stores four
64-bit words -- block, wave of the block | HW_ID << 8 | XCC_ID << 40, wall_clock64() at entry and after the wave's last flush
(msm_seg.hpp AccumTrace) -- into the buffer handed over with nmx_accum_trace_buffer.

Per configuration (rounds of resident lanes x option accum_prio) the script runs a few BN254 MSMs of 2^log2n pairs on the key's
tables, keeps the trace of the last one, groups the waves by (XCC, SE, SH, CU, SIMD) read from HW_ID / XCC_ID, and reports per SIMD
  spread     last finish - first finish among the waves that were resident at the end (the last three)
  two_left   time the SIMD ran with exactly two waves, one_left with exactly one, idle_end from its last finish to the kernel's end
as shares of the kernel's duration (first entry to last finish over all waves): median / mean / 90th percentile / maximum over
the SIMDs.  wall_clock64 ticks at 100 MHz: 10 ns, 1e-5 of a 1 ms kernel.

usage: NMX_SO=<trace build> accum_wave_trace.py [--log2n 20] [--rounds 1 2] [--prio 1] [--runs 3] [--out FILE]"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import nova_amd  # noqa: E402
from nova_amd import _lib  # noqa: E402
from tests import util  # noqa: E402

WAVES_PER_SIMD = 3  # k_launch<AccumSegFn>: three 256-thread blocks per CU, one wave of each on every SIMD


def decode(words):
    """(n, 4) uint64 -> dict of arrays; waves that never ran (all-zero rows) dropped."""
    w = words[(words[:, 2] != 0) | (words[:, 3] != 0)]
    hw = (w[:, 1] >> np.uint64(8)) & np.uint64(0xFFFFFFFF)
    return {"block": w[:, 0].astype(np.int64), "wave": (w[:, 1] & np.uint64(0xFF)).astype(np.int64),
            "simd": ((hw >> np.uint64(4)) & np.uint64(3)).astype(np.int64), "cu": ((hw >> np.uint64(8)) & np.uint64(15)).astype(np.int64),
            "sh": ((hw >> np.uint64(12)) & np.uint64(1)).astype(np.int64), "se": ((hw >> np.uint64(13)) & np.uint64(7)).astype(np.int64),
            "xcc": ((w[:, 1] >> np.uint64(40)) & np.uint64(15)).astype(np.int64),
            "t0": w[:, 2].astype(np.int64), "t1": w[:, 3].astype(np.int64)}


def occupancy(t0, t1):
    """Time a SIMD spent with exactly k waves, k = 1, 2, from the waves' [t0, t1) intervals."""
    ev = sorted([(t, 1) for t in t0] + [(t, -1) for t in t1])
    at = {1: 0, 2: 0}
    live, prev = 0, ev[0][0]
    for t, d in ev:
        if live in at:
            at[live] += t - prev
        live += d
        prev = t
    return at[1], at[2]


def analyse(tr):
    key = (((tr["xcc"] * 8 + tr["se"]) * 2 + tr["sh"]) * 16 + tr["cu"]) * 4 + tr["simd"]
    start, end = tr["t0"].min(), tr["t1"].max()
    dur = float(end - start)
    rows = []
    counts = {}
    for k in np.unique(key):
        m = key == k
        t0, t1 = tr["t0"][m], tr["t1"][m]
        counts[int(m.sum())] = counts.get(int(m.sum()), 0) + 1
        fin = np.sort(t1)[-WAVES_PER_SIMD:]
        one, two = occupancy(t0.tolist(), t1.tolist())
        rows.append(((fin[-1] - fin[0]) / dur, two / dur, one / dur, (end - fin[-1]) / dur))
    return np.array(rows), counts, dur


def line(name, v):
    return f"    {name:9s} median {np.median(v):.4f}  mean {v.mean():.4f}  p90 {np.percentile(v, 90):.4f}  max {v.max():.4f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--rounds", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--prio", type=int, nargs="*", default=[1])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    if not hasattr(L, "nmx_accum_trace_buffer"):
        sys.exit("this library was not built with -DNMX_ACCUM_TRACE (load the measuring build through NMX_SO)")
    L.nmx_accum_trace_buffer.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    assert L.nmx_init(0) == 0
    resident = torch.cuda.get_device_properties(0).multi_processor_count * 256 * WAVES_PER_SIMD
    n = 1 << a.log2n
    g = nova_amd.DlogGroup(0)
    ck = nova_amd.CommitmentKey.generate(0, n, k0=3)
    d = torch.from_numpy(util.random_scalars(0, n, seed=a.log2n)).cuda()
    out = [f"segment accumulate, BN254 G1, 2^{a.log2n} pairs on the key's tables; {resident} lanes resident; shares of the kernel's duration over the SIMDs"]
    try:
        for rounds in a.rounds:
            for prio in a.prio:
                lanes = rounds * resident
                assert L.nmx_set_option(b"seg_lanes", lanes) == 0 and L.nmx_set_option(b"accum_prio", prio) == 0
                buf = torch.zeros((lanes // 64, 4), dtype=torch.int64, device="cuda")
                for _ in range(a.runs):
                    buf.zero_()
                    torch.cuda.synchronize()
                    assert L.nmx_accum_trace_buffer(buf.data_ptr(), buf.numel()) == 0
                    g.vartime_multiscalar_mul(d, ck)
                    torch.cuda.synchronize()
                assert L.nmx_accum_trace_buffer(None, 0) == 0
                tr = decode(buf.cpu().numpy().view(np.uint64))
                rows, counts, dur = analyse(tr)
                note = "grouped by XCC / SE / SH / CU / SIMD from HW_ID"
                if set(counts) != {WAVES_PER_SIMD * rounds}:
                    note += f" (waves per SIMD seen: {dict(sorted(counts.items()))})"
                out.append(f"rounds {rounds}  accum_prio {prio}  waves {len(tr['t0'])}  SIMDs {len(rows)}  kernel {dur / 100:.1f} us  -- {note}")
                for i, name in enumerate(("spread", "two_left", "one_left", "idle_end")):
                    out.append(line(name, rows[:, i]))
                fin_all = (tr["t1"] - tr["t0"].min()) / dur  # when waves finish, chip-wide
                out.append("    finish times of all waves, share of the kernel: " + "  ".join(f"p{p} {np.percentile(fin_all, p):.3f}" for p in (1, 10, 25, 50, 75, 90, 99)))
    finally:
        L.nmx_accum_trace_buffer(None, 0)
        L.nmx_set_option(b"seg_lanes", 0)
        L.nmx_set_option(b"accum_prio", 0)
        ck.close()
    text = "\n".join(out) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
