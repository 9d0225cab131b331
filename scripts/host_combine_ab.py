"""A/B of the host combine (option host_combine) in ONE process, configurations alternating with the order reversed every repetition
(the form of profiles/r07_reduce/segdir_ab.txt): per repetition and configuration `steps` driver-timed MSMs (wall clock around the
call, profiling off), then five more with profiling on for the stage means.  One JSON line per (shape, configuration, repetition).

  pairs    BN254 G1, 2^log2n pairs on the key's tables, scalars in HBM: host_combine 1 (device) against 2 (host)
  sets     a fused batch of k vectors over a 2^14-point key (k = 1, 2, 4, 8, 16: as many bucket sets): 1 against 2
  buckets  keys of 2^10 / 2^14 / 2^17 / 2^20 / 2^22 points (128, 2^14, 2^15, 2^16, 2^19 buckets): the pair tree (reduce_form 1)
           against bit-sliced sums with the device's combine (2, 1) and with the host's (2, 2)

usage: host_combine_ab.py pairs|sets|buckets [--log2n 20 22] [--reps 10] [--steps 20]"""
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


def set_config(cfg):
    assert L.nmx_set_option(b"reduce_form", cfg["reduce_form"]) == 0
    assert L.nmx_set_option(b"host_combine", cfg["host_combine"]) == 0


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


def alternate(tag, configs, call, reps, steps):
    """One discarded repetition, then `reps` kept ones; the order of the configurations is reversed every repetition."""
    try:
        for rep in range(-1, reps):
            order = list(configs.items())
            if rep % 2:
                order.reverse()
            for name, cfg in order:
                set_config(cfg)
                row = measure(call, steps)
                if rep >= 0:
                    print(json.dumps({**tag, "config": name, "rep": rep, **row}), flush=True)
    finally:
        set_config({"reduce_form": 0, "host_combine": 0})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["pairs", "sets", "buckets"])
    ap.add_argument("--log2n", type=int, nargs="*", default=None)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--steps", type=int, default=None)
    a = ap.parse_args()
    g = nova_amd.DlogGroup(0)
    dev_host = {"device": {"reduce_form": 0, "host_combine": 1}, "host": {"reduce_form": 0, "host_combine": 2}}
    if a.mode == "pairs":
        for lg in a.log2n or [20, 22]:
            n = 1 << lg
            ck = nova_amd.CommitmentKey.generate(0, n, k0=3)
            d = torch.from_numpy(util.random_scalars(0, n, seed=lg)).cuda()
            alternate({"log2n": lg}, dev_host, lambda: g.vartime_multiscalar_mul(d, ck), a.reps or 10, a.steps or 20)
            ck.close()
    elif a.mode == "sets":
        n = 1 << 14
        ck = nova_amd.CommitmentKey.generate(0, n, k0=3)
        for k in (1, 2, 4, 8, 16):
            vecs = [torch.from_numpy(util.random_scalars(0, n, seed=100 + j)).cuda() for j in range(k)]
            forced = {"device": {"reduce_form": 2, "host_combine": 1}, "host": {"reduce_form": 2, "host_combine": 2}}
            alternate({"log2n": 14, "sets": k}, forced, lambda: g.batch_vartime_multiscalar_mul(vecs, ck), a.reps or 3, a.steps or 10)
        ck.close()
    else:
        forms = {"pair_tree": {"reduce_form": 1, "host_combine": 1}, "bitsliced_device": {"reduce_form": 2, "host_combine": 1},
                 "bitsliced_host": {"reduce_form": 2, "host_combine": 2}}
        for lg in a.log2n or [10, 14, 17, 20, 22]:
            n = 1 << lg
            ck = nova_amd.CommitmentKey.generate(0, n, k0=3)
            d = torch.from_numpy(util.random_scalars(0, n, seed=lg)).cuda()
            alternate({"log2n": lg}, forms, lambda: g.vartime_multiscalar_mul(d, ck), a.reps or 3, a.steps or 10)
            ck.close()


if __name__ == "__main__":
    main()
