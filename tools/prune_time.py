#!/usr/bin/env python3
"""Pruning the whole machine by best-path weight on the MI355X (csrc/decode_prune.hip; carmel --prune-paths / --prune-states):
carmel_hip_decoder_last_ms (HIP events around every round's kernels, the walk-back, the ranking and the mark passes) and the
rounds of the forward and the backward pass -- what the front end's `timing: prune` line prints -- on the two machines of
tools/best_paths_time.py (--states states, out-degree --degree: `spread`, about --states / 1000 arcs into the final state, and
`hub`, an arc from every state into it; and `spread` once more with the final state cut off, where the backward pass ends at once
and the call is the forward pass and the mark passes alone), with carmel_hip_decoder_best_paths at K = 1 on the same handle as the yardstick: its
relaxation is the forward pass with the K-list bookkeeping around it.  Three calls: a ratio of 10, the same with a cap of a tenth of
the states (the ranking runs), and no ratio at all.
One warm-up call each, then the median of --reps (3).  Prints one JSON object per line and writes all to --out
(profiles/prune_time.json).  Without a device it fails.

    python tools/prune_time.py [--states 1000000] [--degree 10] [--reps 3]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(call, ms_of, reps):
    ms, wall = [], []
    for rep in range(reps + 1):  # (the first is the warm-up: code objects, tables, allocations)
        t0 = time.perf_counter()
        out = call()
        t1 = time.perf_counter()
        if rep:
            ms.append(ms_of())
            wall.append((t1 - t0) * 1e3)
    return out, {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "call_ms": statistics.median(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=1000000)
    ap.add_argument("--degree", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_time.json"))
    a = ap.parse_args()
    from best_paths_time import machines
    from carmel_amd._capi import lib
    from carmel_amd.decode import Decoder
    if lib.carmel_hip_device_count() < 1:
        sys.exit("prune_time: no HIP device")
    res = []

    def all_machines():
        from carmel_amd.model import Wfst
        for name, w in machines(a.states, a.degree):
            yield name, w
        # `spread` with the arcs into the final state at weight zero: the backward pass ends at once, so the call is the forward
        # pass and the mark passes alone, beside the same relaxation in best_paths(1)
        yield "spread, final cut off", Wfst(w.n_states, w.final, w.src, w.dst, w.isym, w.osym, np.where(w.dst == w.final, -np.inf, w.logw))

    for name, w in all_machines():
        d = Decoder(w)
        base = {"machine": name, "states": int(w.n_states), "arcs": int(w.n_arcs)}
        _, t = timed(lambda: d.best_paths_raw(1), d.last_ms, a.reps)
        rounds, selected = d.best_paths_stats()
        row = dict(base, call="best_paths(1)", rounds=rounds, states_selected=selected, **t)
        res.append(row)
        print(json.dumps(row), flush=True)
        for what, args in (("prune(ratio 10)", (math.log(10.0), None)), ("prune(ratio 10, cap |Q| / 10)", (math.log(10.0), w.n_states // 10)),
                           ("prune(no ratio)", (math.inf, None))):
            (state_keep, arc_keep), t = timed(lambda: d.prune(*args), d.last_ms, a.reps)
            f_rounds, r_rounds = d.prune_stats()
            row = dict(base, call=what, f_rounds=f_rounds, r_rounds=r_rounds, states_kept=int(state_keep.sum()), arcs_kept=int(arc_keep.sum()), **t)
            res.append(row)
            print(json.dumps(row), flush=True)
        d.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
