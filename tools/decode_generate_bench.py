#!/usr/bin/env python3
"""Batch generation on the MI355X (csrc/decode_generate.hip; carmel -G / -g): carmel_hip_decoder_last_ms -- the kernels' time, HIP
events around the counting and the writing pass of the walk -- of carmel_hip_decoder_generate for --paths paths (1 000 000) drawn
from the composed tagging machine of tools/decode_bench.py (tagging.fsa.trained.noe o tagging.fst: 46 states, 372 556 arcs, about
8 000 a state), in both modes, with --max-arcs (1000) and --tries (256), seed 1.  Per mode: the median of --reps runs (5) after
one warm-up, the least and the greatest, paths/s and arcs/s at the median, the arcs returned, the mean and the greatest number of
attempts a path took, and the call's wall time (tables, copies and the host's assembly included).  The paths are not fetched into
Python: only their count and their arcs' count are read.  Prints one JSON object and writes it to --out
(profiles/decode_generate_bench.json).  Without a device it fails.

    python tools/decode_generate_bench.py [--paths 1000000] [--reps 5] [--max-arcs 1000] [--tries 256]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
G = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-arcs", type=int, default=1000)
    ap.add_argument("--tries", type=int, default=256)
    ap.add_argument("--fst", default=os.path.join(G, "tagging.fst"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_generate_bench.json"))
    a = ap.parse_args()
    from carmel_amd._capi import check, lib, ptr
    from carmel_amd.decode import GENERATE_MODES, Decoder
    from carmel_amd.model import Wfst
    from decode_ref import golden_file
    from oracle import binding as ob
    if lib.carmel_hip_device_count() < 1:
        sys.exit("decode_generate_bench: no HIP device")
    tmp = tempfile.mkdtemp()
    oc = ob.OracleCascade([open(m).read() for m in (golden_file(G, "tagging.fsa.trained.noe", tmp), a.fst)], remember=False)
    w = oc.composed().arrays()
    W = Wfst(w["n_states"], w["final"], w["src"], w["dst"], w["isym"], w["osym"], w["logw"])
    d = Decoder(W)
    res = {"paths": a.paths, "reps": a.reps, "max_arcs": a.max_arcs, "max_tries": a.tries, "states": int(W.n_states),
           "arcs": int(W.n_arcs), "most_arcs_a_state": int(np.bincount(W.src).max())}
    tries = np.zeros(a.paths, np.uint32)
    for mode in ("joint", "conditional"):
        ms, wall = [], []
        n_paths, n_arcs = C.c_uint64(), C.c_uint64()
        for rep in range(a.reps + 1):  # (the first is the warm-up: code objects, tables, allocations)
            t0 = time.perf_counter()
            check(lib.carmel_hip_decoder_generate(d._h, GENERATE_MODES[mode], a.paths, 0, 1, a.max_arcs, a.tries, ptr(tries)),
                  "carmel_hip_decoder_generate")
            t1 = time.perf_counter()
            if rep:
                ms.append(d.last_ms())
                wall.append((t1 - t0) * 1e3)
        check(lib.carmel_hip_decoder_kbest_size(d._h, C.byref(n_paths), C.byref(n_arcs)), "carmel_hip_decoder_kbest_size")
        assert n_paths.value == a.paths
        med = statistics.median(ms)
        res[mode] = {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "call_ms": statistics.median(wall),
                     "paths_per_s": a.paths / (med * 1e-3), "arcs_per_s": n_arcs.value / (med * 1e-3), "path_arcs": int(n_arcs.value),
                     "mean_arcs_a_path": n_arcs.value / float(a.paths), "mean_tries": float(tries.mean()), "max_tries_used": int(tries.max())}
    d.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
