#!/usr/bin/env python3
"""Consolidating duplicate arcs on the MI355X (csrc/consolidate.hip; carmel -C): carmel_hip_consolidate's kernel_ms (HIP events
around the kernels, not the copies) on synth.random_wfst at --states states and out-degree --degree, with every arc copied once
with probability 1/4 under a fresh weight (the copy follows its original in the state's list) and one state given a segment of
--hub members.  Modes sum and max.  One warm-up call each, then the median of --reps (3).  With the library's `timing` option
on, every call also writes its per-pass split (key and sort, heads, reduce, compact) to stderr.

Beside the time: the bytes the passes must move at the least -- the key pass reads the four fields and the weight of every arc
and writes an 8-byte key and a 4-byte id (32 B an arc); a radix sort of 12-byte pairs reads and writes them once per digit pass,
counted here as one pass only (24 B); heads, numbering and extents 20 B; the reduction an id and a weight (12 B); the compaction
16 B an old arc and 12 B a kept one -- as a fraction of the HBM peak (8 TB/s, datasheet).  A first measurement, unprofiled.

Prints one JSON object per line and writes all to --out (profiles/consolidate_time.json).  Without a device it fails.

    python tools/consolidate_time.py [--states 1000000] [--degree 10] [--hub 100000] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes a second, datasheet


def machine(states, degree, hub, seed=7):
    """-> (src, dst, isym, osym, logw) in arc-id order"""
    from carmel_amd import synth
    w = synth.random_wfst(states, degree, n_sym=64, p_eps=0.1, seed=seed)
    rng = np.random.default_rng(seed + 1)
    copies = 1 + (rng.random(w.n_arcs) < 0.25)
    order = np.repeat(np.arange(w.n_arcs), copies)
    logw = w.logw[order].copy()
    fresh = np.concatenate([[False], order[1:] == order[:-1]])
    logw[fresh] = np.log(rng.uniform(0.01, 1.0, int(fresh.sum())))
    cols = [w.src[order], w.dst[order], w.isym[order], w.osym[order]]
    q = states // 2  # one state gets `hub` more arcs of one key, at the end of its list
    at = int(np.searchsorted(cols[0], q, side="right"))
    extra = [np.full(hub, v, np.uint32) for v in (q, q + 1, 5, 6)]
    cols = [np.concatenate([c[:at], e, c[at:]]) for c, e in zip(cols, extra)]
    logw = np.concatenate([logw[:at], np.log(rng.uniform(0.2, 1.0, hub) / hub), logw[at:]])
    return cols + [logw]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=1000000)
    ap.add_argument("--degree", type=int, default=10)
    ap.add_argument("--hub", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consolidate_time.json"))
    a = ap.parse_args()
    from carmel_amd._capi import lib
    from carmel_amd.decode import consolidate_raw
    if lib.carmel_hip_device_count() < 1:
        sys.exit("consolidate_time: no HIP device")
    arcs = machine(a.states, a.degree, a.hub)
    n = len(arcs[0])
    res = []
    for mode in ("sum", "max"):
        ms, wall = [], []
        for rep in range(a.reps + 1):  # (the first is the warm-up: code objects, allocations)
            t0 = time.perf_counter()
            n_kept, kept_id, kept_logw, arc_map, kernel_ms = consolidate_raw(*arcs, mode=mode, clamp=True)
            t1 = time.perf_counter()
            if rep:
                ms.append(kernel_ms)
                wall.append((t1 - t0) * 1e3)
        least = (32 + 24 + 20 + 12 + 16) * n + 12 * n_kept
        med = statistics.median(ms)
        row = {"machine": "random_wfst, a quarter of the arcs copied, one segment of %d" % a.hub, "states": a.states, "arcs": n,
               "mode": mode, "arcs_kept": int(n_kept), "largest_segment": int(np.bincount(arc_map[arc_map != 0xFFFFFFFF]).max()),
               "median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "call_ms": statistics.median(wall), "least_bytes": int(least),
               "fraction_of_hbm_peak": least / (med * 1e-3) / HBM_PEAK}
        res.append(row)
        print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
