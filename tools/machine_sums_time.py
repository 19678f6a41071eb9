#!/usr/bin/env python3
"""The sums over all paths of the whole machine on the MI355X (csrc/decode_machine_sums.hip; carmel --machine-sums):
carmel_hip_decoder_last_ms of one carmel_hip_decoder_machine_sums call (HIP events around the kernels, not the copies) on a
synthetic layered machine built here: state 0, --layers layers of --width states, the final state.  State 0 has an arc to every
state of the first layer, every state of a later layer has --degree in-arcs from random states of the layer before it, every state
of the last layer an arc to the final state.  A state that no arc leaves is a dead end: reachable, not useful.  One warm-up
call, then --reps calls; the median is reported.

Beside the time: the level counts, |U|, N, and the largest |device - reference| / bound over alpha and beta of every useful state,
the reference and the bound E being those of tests/machine_sums_ref.py restated on numpy arrays (np.longdouble, a layer at a
time), so that 10^7 arcs take seconds.  A first measurement, unprofiled: there is no earlier figure to compare it with.

Prints one JSON object and writes it to --out (profiles/machine_sums_time.json).  Without a device it fails.

    python tools/machine_sums_time.py [--layers 100] [--width 10000] [--degree 10] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LD = np.longdouble
U = LD(2.0) ** -53


def machine(layers, width, degree, seed=7):
    """-> (n_states, final, blocks): blocks[l] = (from, into, logw) of the arcs between two neighbouring layers, grouped by `into`"""
    rng = np.random.default_rng(seed)
    first = lambda l: 1 + l * width
    final = 1 + layers * width
    blocks = [(np.zeros(width, np.int64), first(0) + np.arange(width), rng.uniform(-3.0, -1.0, width))]
    for l in range(1, layers):
        into = np.repeat(first(l) + np.arange(width), degree)
        blocks.append((first(l - 1) + rng.integers(0, width, width * degree), into, rng.uniform(-3.0, -1.0, width * degree)))
    blocks.append((first(layers - 1) + np.arange(width), np.full(width, final), rng.uniform(-3.0, -1.0, width)))
    return final + 1, final, blocks


def sweep(n_states, start, blocks):
    """-> (sum, bound) per state in np.longdouble: blocks in sweep order, each (from, into, logw) -- the terms flow from `from`"""
    val = np.full(n_states, -np.inf, LD)
    err = np.zeros(n_states, LD)
    val[start] = 0
    for frm, into, w in blocks:
        order = np.argsort(into, kind="stable")
        frm, into, w = frm[order], into[order], w[order]
        t = val[frm] + w.astype(LD)
        live = t > -np.inf
        frm, into, t = frm[live], into[live], t[live]
        if not len(t):
            continue
        starts = np.flatnonzero(np.concatenate([[True], into[1:] != into[:-1]]))
        d = np.diff(np.concatenate([starts, [len(t)]]))
        m = np.maximum.reduceat(t, starts)
        s = np.add.reduceat(np.exp(t - np.repeat(m, d)), starts)
        v = np.where(d == 1, m, m + np.log(s))
        moved = np.maximum.reduceat(err[frm] + U * np.abs(t), starts)
        q = into[starts]
        val[q] = v
        err[q] = np.where(d == 1, moved, moved + (4 * d + 4) * U + U * np.abs(v))
    return val, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=100)
    ap.add_argument("--width", type=int, default=10000)
    ap.add_argument("--degree", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "machine_sums_time.json"))
    a = ap.parse_args()
    from carmel_amd._capi import lib
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    if lib.carmel_hip_device_count() < 1:
        sys.exit("machine_sums_time: no HIP device")
    Q, final, blocks = machine(a.layers, a.width, a.degree)
    src, dst, logw = (np.concatenate([b[i] for b in blocks]) for i in range(3))
    order = np.argsort(src, kind="stable")
    one = np.ones(len(src), np.uint32)
    w = Wfst(Q, final, src[order], dst[order], one, one, logw[order])
    d = Decoder(w)
    ms, wall = [], []
    for rep in range(a.reps + 1):  # (the first is the warm-up: code objects, the tables)
        t0 = time.perf_counter()
        Z, N, n_useful = d.machine_sums()
        t1 = time.perf_counter()
        if rep:
            ms.append(d.last_ms())
            wall.append((t1 - t0) * 1e3)
    alpha, beta, cf, cb, level = d.machine_sums_states()
    levels = d.machine_sums_stats()
    d.close()
    # the reference: beta first (it says which states are useful), then alpha over the useful states' arcs
    ref_b, err_b = sweep(Q, final, [(b[1], b[0], b[2]) for b in reversed(blocks)])
    useful = ref_b > -np.inf  # (every state is reachable from state 0)
    ref_a, err_a = sweep(Q, 0, [(b[0][useful[b[1]]], b[1][useful[b[1]]], b[2][useful[b[1]]]) for b in blocks])
    assert int(useful.sum()) == n_useful and ((level != 0xFFFFFFFF) == useful).all()
    assert (alpha[~useful] == -np.inf).all() and (beta[~useful] == -np.inf).all()
    ratio = 0.0
    for got, ref, err in ((alpha, ref_a, err_a), (beta, ref_b, err_b)):
        sel = useful & (err > 0)
        ratio = max(ratio, float((np.abs(got[sel].astype(LD) - ref[sel]) / err[sel]).max()))
    row = {"machine": "layered: state 0, %d layers of %d states, %d in-arcs a state, the final state" % (a.layers, a.width, a.degree),
           "states": Q, "arcs": int(w.n_arcs), "useful_states": int(n_useful), "forward_levels": levels[0], "backward_levels": levels[1],
           "total_logw": Z, "n_paths": N, "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
           "call_ms": statistics.median(wall), "largest_error_over_bound": ratio, "largest_bound": float(max(err_a.max(), err_b.max())),
           "gap_alpha_final_beta_0": abs(float(alpha[final]) - float(beta[0]))}
    print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
