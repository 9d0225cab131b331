"""A/B of the segment accumulate's progress-keyed wave priority (option accum_prio) and of the rounds of resident lanes (option
seg_lanes) in ONE process: configurations alternating with the order reversed every repetition, one discarded repetition first (the
form of scripts/host_combine_ab.py).  Per repetition and configuration `steps` driver-timed MSMs (wall clock around the call,
profiling off), then five more with profiling on for the stage means.  One JSON line per (shape, configuration, repetition).
BN254 G1, 2^log2n pairs on the key's tables, scalars in HBM.

  configurations  r<rounds>p<accum_prio>, e.g. r2p1 = two rounds of resident lanes, priority off; r0 = rounds by the library's rule,
                  p0 = priority by the library's rule (r0p0 is the build's default)

usage: accum_prio_ab.py [--log2n 20 22] [--configs r0p0 r1p1 r1p2 ...] [--reps 10] [--steps 20]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import nova_amd  # noqa: E402
from nova_amd import _lib  # noqa: E402
from tests import util  # noqa: E402

STAGES = ["digits", "sort", "bounds_plan", "accum", "fold", "reduce", "tail"]
L = _lib.lib()
assert L.nmx_init(0) == 0
HAS_PRIO = L.nmx_set_option(b"accum_prio", 0) == 0  # a build from before the option knows only p0
RESIDENT = torch.cuda.get_device_properties(0).multi_processor_count * 768  # three 256-thread blocks per CU


def set_config(name):
    rounds, prio = int(name[1:name.index("p")]), int(name[name.index("p") + 1:])
    assert L.nmx_set_option(b"seg_lanes", rounds * RESIDENT) == 0
    if HAS_PRIO:
        assert L.nmx_set_option(b"accum_prio", prio) == 0
    else:
        assert prio == 0, "this build has no option accum_prio"


def measure(call, steps):
    for _ in range(3):
        call()
    per = []
    t0 = time.perf_counter()
    for _ in range(steps):
        t = time.perf_counter()
        call()
        per.append((time.perf_counter() - t) * 1e3)
    total = (time.perf_counter() - t0) * 1e3 / steps
    L.nmx_set_profiling(1)
    acc = np.zeros(12)
    for _ in range(5):
        call()
        buf = (ctypes.c_float * 12)()
        k = L.nmx_profile_last(buf, 12)
        acc[:k] += np.array(buf[:k])
    L.nmx_set_profiling(0)
    out = {"ms_per_step": round(total, 4), "call_ms_median": round(statistics.median(per), 4)}
    out.update({STAGES[i]: round(acc[i] / 5, 4) for i in range(7)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[20, 22])
    ap.add_argument("--configs", nargs="*", default=["r1p1", "r1p2", "r2p1", "r2p2"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    g = nova_amd.DlogGroup(0)
    for lg in a.log2n:
        n = 1 << lg
        ck = nova_amd.CommitmentKey.generate(0, n, k0=3)
        d = torch.from_numpy(util.random_scalars(0, n, seed=lg)).cuda()
        try:
            for rep in range(-1, a.reps):
                order = list(a.configs)
                if rep % 2:
                    order.reverse()
                for name in order:
                    set_config(name)
                    row = measure(lambda: g.vartime_multiscalar_mul(d, ck), a.steps)
                    if rep >= 0:
                        print(json.dumps({"log2n": lg, "config": name, "rep": rep, **row}), flush=True)
        finally:
            set_config("r0p0")
            ck.close()


if __name__ == "__main__":
    main()
