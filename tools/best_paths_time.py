#!/usr/bin/env python3
"""The K best paths of the whole machine on the MI355X (csrc/decode_best_paths.hip; carmel --best-paths=N): rounds,
states_selected, carmel_hip_decoder_last_ms (HIP events around every round's kernels and the read-out) and arcs merged per second
of carmel_hip_decoder_best_paths for K = 1, 8 and 64 on two machines of --states states (1 000 000) and out-degree --degree (10):

  hub     synth.random_wfst as it is: arc 0 of EVERY state enters the final state, so the final state has --states - 1 in-arcs and
          is merged by one wavefront while every other state (about 9 in-arcs) takes a lane;
  spread  the same machine with arc 0 of only every 1000th state left entering the final state (the others go to uniform
          non-final states): the final state has about --states / 1000 in-arcs.

"Arcs merged" is the sum over the rounds of the in-arcs of the states selected.  The library counts states, not arcs, so the tool
gives two bounds: `arcs_merged_low` counts every selected state at the mean in-degree of the states other than the final one
(the final state's share left out altogether), `arcs_merged_high` adds the final state's in-arcs once per round (it is selected
in at most every round).  On the hub machine the two are far apart, the final state holding a tenth of all arcs; both rates
divide by the kernels' time.
One warm-up call per (machine, K), then the median of --reps (3).  Prints one JSON object per line as it goes
and writes all to --out (profiles/best_paths_time.json).  Without a device it fails.

    python tools/best_paths_time.py [--states 1000000] [--degree 10] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def machines(n_states, degree):
    from carmel_amd import synth
    from carmel_amd.model import Wfst
    w = synth.random_wfst(n_states, degree, seed=5)
    yield "hub", w
    rng = np.random.default_rng(6)
    dst = w.dst.copy()
    arc0 = np.arange(0, w.n_arcs, degree)
    moved = arc0[(arc0 // degree) % 1000 != 0]
    dst[moved] = rng.integers(0, n_states - 1, len(moved))
    yield "spread", Wfst(w.n_states, w.final, w.src, dst, w.isym, w.osym, w.logw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=1000000)
    ap.add_argument("--degree", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "best_paths_time.json"))
    a = ap.parse_args()
    from carmel_amd._capi import lib
    from carmel_amd.decode import Decoder
    if lib.carmel_hip_device_count() < 1:
        sys.exit("best_paths_time: no HIP device")
    res = []
    for name, w in machines(a.states, a.degree):
        indeg = np.bincount(w.dst, minlength=w.n_states)
        d = Decoder(w)
        for K in a.k:
            ms, wall = [], []
            for rep in range(a.reps + 1):  # (the first is the warm-up: code objects, tables, allocations)
                t0 = time.perf_counter()
                logw, path_off, _ = d.best_paths_raw(K)
                t1 = time.perf_counter()
                if rep:
                    ms.append(d.last_ms())
                    wall.append((t1 - t0) * 1e3)
            rounds, selected = d.best_paths_stats()
            med = statistics.median(ms)
            low = selected * float(np.delete(indeg, w.final).mean())  # every selected state at the others' mean in-degree
            row = {"machine": name, "states": int(w.n_states), "arcs": int(w.n_arcs), "final_in_arcs": int(indeg[w.final]),
                   "mean_in_arcs": float(indeg.mean()), "k": K, "paths": len(logw), "longest_path": int(np.diff(path_off).max()),
                   "rounds": rounds, "states_selected": selected, "median_ms": med, "min_ms": min(ms), "max_ms": max(ms),
                   "call_ms": statistics.median(wall), "ms_per_round": med / max(rounds, 1),
                   "states_selected_per_s": selected / (med * 1e-3),
                   "arcs_merged_low_per_s": low / (med * 1e-3), "arcs_merged_high_per_s": (low + rounds * float(indeg[w.final])) / (med * 1e-3)}
            res.append(row)
            print(json.dumps(row), flush=True)
        d.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
