"""A/B of level 1 of the bucket partition with per-chunk count rows (option part_rows) in ONE process: configurations alternating with
the order reversed every repetition, one discarded repetition first (the form of scripts/accum_prio_ab.py).  Per repetition and
configuration `steps` driver-timed MSMs (wall clock around the call, profiling off), then five more with profiling on for the stage
means.  One JSON line per (shape, scalar set, configuration, repetition), then one summary line per (shape, scalar set).
BN254 G1, 2^log2n pairs on the key's tables, scalars in HBM.

  configurations  p<part_rows>: p1 = the counting and placing passes with global atomics, p2 = count rows wherever the shape allows,
                  p0 = by the library's rule (the build's default)
  scalar sets     random, equal, zero_rm1 (tests/util.scalar_set) or u<bits>

usage: part_rows_ab.py [--log2n 18 20 21 22] [--dist random u1 ...] [--configs p1 p0] [--reps 10] [--steps 20]"""
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


def set_config(name):
    assert L.nmx_set_option(b"part_rows", int(name[1:])) == 0


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
    ap.add_argument("--log2n", type=int, nargs="*", default=[18, 20, 21, 22])
    ap.add_argument("--dist", nargs="*", default=["random"])
    ap.add_argument("--configs", nargs="*", default=["p1", "p0"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    g = nova_amd.DlogGroup(0)
    for lg in a.log2n:
        n = 1 << lg
        ck = nova_amd.CommitmentKey.generate(0, n, k0=3)
        try:
            for dist in a.dist:
                d = torch.from_numpy(np.ascontiguousarray(util.scalar_set(0, n, dist, seed=lg))).cuda()
                ms = {name: [] for name in a.configs}
                for rep in range(-1, a.reps):
                    order = list(a.configs)
                    if rep % 2:
                        order.reverse()
                    for name in order:
                        set_config(name)
                        row = measure(lambda: g.vartime_multiscalar_mul(d, ck), a.steps)
                        if rep >= 0:
                            ms[name].append(row["ms_per_step"])
                            print(json.dumps({"log2n": lg, "dist": dist, "config": name, "rep": rep, **row}), flush=True)
                print(json.dumps({"log2n": lg, "dist": dist, "summary": {k: {"min": min(v), "median": round(statistics.median(v), 4), "max": max(v)}
                                                                         for k, v in ms.items() if v}}), flush=True)
        finally:
            set_config("p0")
            ck.close()


if __name__ == "__main__":
    main()
