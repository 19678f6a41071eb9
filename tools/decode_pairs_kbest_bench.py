#!/usr/bin/env python3
"""Batch pair k-best alignments on the MI355X (csrc/decode_pairs_kbest.hip): carmel_hip_decoder_last_ms -- the kernels' time, HIP
events around the trellis and both passes of the walk -- of carmel_hip_decode_pairs and of carmel_hip_decode_pairs_kbest with K =
1, 4 and 16 on one handle in one process, the four alternating within every repetition, on two workloads:
  epron-jpron   the pairs of tests/golden/epron-jpron.data against tests/golden/epron-jpron.fst (a handful of pairs: what this
                measures is launches and the walk, not a rate);
  dense         --pairs pairs (4096) of one small dense machine of tests/decode_pairs_kbest_cases.py (--seed, default 4).
Per workload and entry: the median of --reps runs (5) after one warm-up, the least and the greatest, the paths returned, and for
K = 1 the ratio of the medians to carmel_hip_decode_pairs (K = 1 runs the k-list kernel; it is not routed to the 1-best kernel).
Rank 0 of every K is checked against carmel_hip_decode_pairs.  Prints one JSON object and writes it to --out
(profiles/decode_pairs_kbest_bench.json).  Without a device it fails.

    python tools/decode_pairs_kbest_bench.py [--pairs 4096] [--reps 5] [--seed 4]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
G = os.path.join(ROOT, "tests", "golden")
KS = (1, 4, 16)


def measure(W, side, xs, ys, reps):
    from carmel_amd.decode import Decoder
    d = Decoder(W, side=side)
    ms = {"decode_pairs": []}
    ms.update({"kbest_%d" % K: [] for K in KS})
    n_paths = {}
    for rep in range(reps + 1):  # (the first is the warm-up: code objects, allocations)
        best, paths1 = d.decode_pairs(xs, ys)
        t = d.last_ms()
        if rep:
            ms["decode_pairs"].append(t)
        for K in KS:
            line_paths, logw, path_off, arcs = d.decode_pairs_kbest_raw(xs, ys, K)
            t = d.last_ms()
            if rep:
                ms["kbest_%d" % K].append(t)
                continue
            n_paths["kbest_%d" % K] = int(line_paths[-1])
            for l in range(len(xs)):  # rank 0 is carmel_hip_decode_pairs' path and weight
                a, b = int(line_paths[l]), int(line_paths[l + 1])
                assert (a == b) == bool(np.isneginf(best[l])), l
                if a < b:
                    assert logw[a] == best[l] and list(arcs[int(path_off[a]):int(path_off[a + 1])]) == list(paths1[l]), l
    d.close()
    out = {"pairs": len(xs), "pairs_with_a_derivation": int(np.isfinite(best).sum()), "nodes": int(sum((len(x) + 1) * (len(y) + 1)
                                                                                                      for x, y in zip(xs, ys))) * W.n_states}
    for k, v in ms.items():
        out[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "paths": n_paths.get(k, out["pairs_with_a_derivation"])}
    out["kbest_1_over_decode_pairs"] = out["kbest_1"]["median_ms"] / out["decode_pairs"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_pairs_kbest_bench.json"))
    a = ap.parse_args()
    from carmel_amd._capi import lib
    from carmel_amd.model import Wfst
    if lib.carmel_hip_device_count() < 1:
        sys.exit("decode_pairs_kbest_bench: no HIP device")
    res = {"reps": a.reps}
    from oracle import binding as ob
    fst, data = os.path.join(G, "epron-jpron.fst"), os.path.join(G, "epron-jpron.data")
    ow = ob.OracleWfst.parse(open(fst).read())
    w, cp = ow.arrays(), ob.OracleCorpus.parse(ow, open(data).read()).arrays()
    n = len(cp["in_off"]) - 1
    line = lambda side, l: [int(s) for s in cp[side + "_sym"][int(cp[side + "_off"][l]):int(cp[side + "_off"][l + 1])]]
    W = Wfst(w["n_states"], w["final"], w["src"], w["dst"], w["isym"], w["osym"], w["logw"])
    res["epron_jpron"] = measure(W, 0, [line("in", l) for l in range(n)], [line("out", l) for l in range(n)], a.reps)
    from decode_pairs_cases import pairs_for
    from decode_pairs_kbest_cases import V, case
    c = case(a.seed)
    pairs = pairs_for(np.random.default_rng(a.seed), c["w"], c["side"], V, a.pairs)
    res["dense"] = measure(c["w"], c["side"], [x for x, _ in pairs], [y for _, y in pairs], a.reps)
    res["dense"].update(seed=a.seed, states=int(c["w"].n_states), arcs=int(c["w"].n_arcs))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
