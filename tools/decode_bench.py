#!/usr/bin/env python3
"""Batch 1-best and k-best decoding, all-paths sums, posterior path samples and arc posteriors on the MI355X (csrc/decode.hip,
csrc/decode_kbest.hip, csrc/decode_sum.hip, csrc/decode_sample.hip, csrc/decode_posterior.hip): the tagging machine (tagging.fsa.trained.noe o tagging.fst, words on
the output side as in `carmel -qbsriWIEk 1`) over tagging.data.noe repeated to about --lines lines, then the front end's
end-to-end time for the tutorial's three decode commands.  Every --kbest K adds the same lines through carmel_hip_decode_kbest
with that K ("kbest": kernel and call time, paths returned, and for K = 1 the ratio to the 1-best kernels' time of this run).
--sum adds the same lines through carmel_hip_decode_sum, timed in the same run ("sum": kernel and call time, lines per second,
the ratio to the 1-best kernels' time), and writes that run's figures to --sum-out (profiles/decode_sum_bench.json).
Every --sample N adds the same lines through carmel_hip_decode_sample with N samples a line (seed 1), beside the sum and the
1-best decode of the same run ("sample": kernel and call time, paths returned, the ratios to the sum's and the 1-best kernels'
time), and writes that run's figures to --sample-out (profiles/decode_sample_bench.json).
--posterior adds the same lines through carmel_hip_decode_posterior, beside the sum and --sample 1 of the same run ("posterior":
kernel and call time, lines per second, the ratios to the sum's, the one-sample and the 1-best kernels' time, the total of the
matched arcs' counts against the positions of the lines with a derivation), and writes that run's figures to --posterior-out
(profiles/decode_posterior_bench.json).
--pairs pairs every line with the other-side string of its 1-best path (a line without a derivation with the empty string) and
adds the pairs through carmel_hip_decode_pairs and carmel_hip_decode_pairs_sum (csrc/decode_pairs.hip), beside the 1-best decode
and the sum of the same run ("pairs": kernel and call time of both, pairs per second, trellis nodes per second, the ratios to the
1-best and the sum kernels' time, whether every pair of a line with a derivation has one), and writes that run's figures to
--pairs-out (profiles/decode_pairs_bench.json).
--pairs-posterior adds the same pairs through carmel_hip_decode_pairs_posterior (csrc/decode_pairs_posterior.hip), beside
carmel_hip_decode_pairs_sum timed in the same loop ("pairs_posterior": kernel and call time of both, pairs per second, the kernels'
time as a multiple of the pair sum's, whether the sums are the pair sum's bit for bit, the matched and the other-side arcs' counts
against the lengths of the pairs with a derivation), and writes that run's figures to --pairs-posterior-out
(profiles/decode_pairs_posterior_bench.json).
--pairs-sample[=N] (N = 8 if left out) adds the same pairs through carmel_hip_decode_pairs_sample (csrc/decode_pairs_sample.hip)
with N samples a pair (seed 1), beside carmel_hip_decode_pairs_sum and carmel_hip_decode_pairs_posterior timed in the same loop
("pairs_sample": kernel and call time of the three, pairs per second, the sampler's kernels' time as a multiple of the pair sum's
and of the pair posteriors', the memory tier, whether every pair with a sum has N paths and every path spells its pair), and
writes that run's figures to --pairs-sample-out (profiles/decode_pairs_sample_bench.json).
Prints one JSON object.

    python tools/decode_bench.py [--lines 100000] [--reps 5] [--fst tests/golden/tagging.fst] [--kbest 1 --kbest 4 ...] [--sum]
                                 [--sample 1 --sample 16] [--posterior] [--pairs] [--pairs-posterior] [--pairs-sample[=N]]

The tagging fst defaults to the untrained tests/golden/tagging.fst (same arcs as the trained one: the timing does not depend
on the weights); the cluster and cipher commands use their committed trained members."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
G = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "carmel_amd", "bin", "carmel")


def composed(members):
    """the composed machine as `carmel -HJ` prints it, read back through the oracle's composition (exact weights)"""
    from oracle import binding as ob
    oc = ob.OracleCascade([open(m).read() for m in members], remember=False)
    return oc, oc.composed().arrays()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fst", default=os.path.join(G, "tagging.fst"))
    ap.add_argument("--kbest", type=int, action="append", default=[], metavar="K")
    ap.add_argument("--sum", action="store_true")
    ap.add_argument("--sum-out", default=os.path.join(ROOT, "profiles", "decode_sum_bench.json"))
    ap.add_argument("--sample", type=int, action="append", default=[], metavar="N")
    ap.add_argument("--sample-out", default=os.path.join(ROOT, "profiles", "decode_sample_bench.json"))
    ap.add_argument("--posterior", action="store_true")
    ap.add_argument("--posterior-out", default=os.path.join(ROOT, "profiles", "decode_posterior_bench.json"))
    ap.add_argument("--pairs", action="store_true")
    ap.add_argument("--pairs-out", default=os.path.join(ROOT, "profiles", "decode_pairs_bench.json"))
    ap.add_argument("--pairs-posterior", action="store_true")
    ap.add_argument("--pairs-posterior-out", default=os.path.join(ROOT, "profiles", "decode_pairs_posterior_bench.json"))
    ap.add_argument("--pairs-sample", type=int, nargs="?", const=8, default=None, metavar="N")
    ap.add_argument("--pairs-sample-out", default=os.path.join(ROOT, "profiles", "decode_pairs_sample_bench.json"))
    a = ap.parse_args()
    sample_ns = a.sample + ([1] if a.posterior and 1 not in a.sample else [])  # (the posteriors are reported beside one sample a line)
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    from decode_ref import golden_file
    tmp = tempfile.mkdtemp()
    gf = lambda name: golden_file(G, name, tmp)  # (the larger fixtures are committed compressed)
    data = [l for l in open(os.path.join(G, "tagging.data")).read().split("\n") if l.split()]
    oc, w = composed([gf("tagging.fsa.trained.noe"), a.fst])
    c = oc.corpus("".join("\n%s\n" % l for l in data)).arrays()
    base = [c["out_sym"][int(c["out_off"][k]):int(c["out_off"][k + 1])] for k in range(len(data))]
    lines = (base * (a.lines // len(base) + 1))[:a.lines]
    W = Wfst(w["n_states"], w["final"], w["src"], w["dst"], w["isym"], w["osym"], w["logw"])
    d = Decoder(W, side=1)
    d.decode(lines[:1000])  # warm-up (code objects, allocations)
    ms, wall = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        best, paths = d.decode(lines)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(d.last_ms())
    kbest = {}
    for K in a.kbest:
        d.decode_kbest_raw(lines[:1000], K)
        kms_k, wall_k = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            line_paths, logw, path_off, arcs = d.decode_kbest_raw(lines, K)
            wall_k.append((time.perf_counter() - t0) * 1e3)
            kms_k.append(d.last_ms())
        kbest[str(K)] = {"kernel_ms": float(np.median(kms_k)), "kernel_ms_all": kms_k, "call_ms": float(np.median(wall_k)),
                         "paths": int(len(logw)), "path_arcs": int(len(arcs)),
                         "rank0_equals_1best": bool(np.array_equal(logw[line_paths[:-1][np.diff(line_paths) > 0].astype(np.int64)],
                                                                   best[~np.isneginf(best)]))}
    sums = None
    if a.sum or sample_ns or a.pairs:  # (the samples, the posteriors and the pairs are reported beside the sum of the same run)
        d.sum(lines[:1000])
        kms_s, wall_s = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            total = d.sum(lines)
            wall_s.append((time.perf_counter() - t0) * 1e3)
            kms_s.append(d.last_ms())
        sums = {"kernel_ms": float(np.median(kms_s)), "kernel_ms_all": kms_s, "call_ms": float(np.median(wall_s)),
                "lines_per_s": len(lines) / (float(np.median(kms_s)) * 1e-3), "no_derivation": int(np.isneginf(total).sum()),
                "sum_ln": float(total[~np.isneginf(total)].sum()), "viterbi_ln": float(best[~np.isneginf(best)].sum()),
                # (a line with one derivation sums its arcs in path order, the 1-best weight is added from the end: the last bit may differ)
                "max_1best_minus_sum": float(np.max(best[~np.isneginf(best)] - total[~np.isneginf(best)]))}
    samples = {}
    for N in sample_ns:
        d.sample_raw(lines[:1000], N, 1)
        kms_n, wall_n = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            line_paths, logw, path_off, arcs = d.sample_raw(lines, N, 1)
            wall_n.append((time.perf_counter() - t0) * 1e3)
            kms_n.append(d.last_ms())
        with_paths = np.diff(line_paths) > 0
        samples[str(N)] = {"kernel_ms": float(np.median(kms_n)), "kernel_ms_all": kms_n, "call_ms": float(np.median(wall_n)),
                           "paths": int(len(logw)), "path_arcs": int(len(arcs)),
                           "lines_per_s": len(lines) / (float(np.median(kms_n)) * 1e-3),
                           "every_line_with_a_sum_has_n_paths": bool(np.array_equal(with_paths, ~np.isneginf(total)) and
                                                                     (np.diff(line_paths)[with_paths] == N).all())}
    post = None
    if a.posterior:
        d.posterior(lines[:1000])
        kms_p, wall_p = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            psums, counts = d.posterior(lines)
            wall_p.append((time.perf_counter() - t0) * 1e3)
            kms_p.append(d.last_ms())
        has = ~np.isneginf(psums)
        post = {"kernel_ms": float(np.median(kms_p)), "kernel_ms_all": kms_p, "call_ms": float(np.median(wall_p)),
                "lines_per_s": len(lines) / (float(np.median(kms_p)) * 1e-3),
                "sums_equal_the_sum": bool(psums.tobytes() == total.tobytes()),
                "matched_count": float(counts[w["osym"] != 0].sum()),
                "positions_with_a_derivation": int(sum(len(x) for x, h in zip(lines, has) if h))}
    pairs = None
    if a.pairs:
        isym = np.asarray(w["isym"])
        other = [isym[p][isym[p] != 0] for p in paths]  # the tags of the line's best path
        d.decode_pairs(lines[:1000], other[:1000])
        d.sum_pairs(lines[:1000], other[:1000])
        kms_b, wall_b, kms_t, wall_t = [], [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            pbest, ppaths = d.decode_pairs(lines, other)
            wall_b.append((time.perf_counter() - t0) * 1e3)
            kms_b.append(d.last_ms())
            t0 = time.perf_counter()
            psum = d.sum_pairs(lines, other)
            wall_t.append((time.perf_counter() - t0) * 1e3)
            kms_t.append(d.last_ms())
        nodes = int(sum((len(x) + 1) * (len(y) + 1) for x, y in zip(lines, other))) * int(w["n_states"])
        pairs = {"best": {"kernel_ms": float(np.median(kms_b)), "kernel_ms_all": kms_b, "call_ms": float(np.median(wall_b))},
                 "sum": {"kernel_ms": float(np.median(kms_t)), "kernel_ms_all": kms_t, "call_ms": float(np.median(wall_t))},
                 "trellis_nodes": nodes, "no_derivation": int(np.isneginf(pbest).sum()),
                 "a_pair_has_a_derivation_where_its_line_has": bool(np.array_equal(np.isneginf(pbest), np.isneginf(best)) and
                                                                    np.array_equal(np.isneginf(psum), np.isneginf(best))),
                 # (the line's best path is a derivation of the pair: the pair's best is at least as good, to the bit)
                 "pair_best_equals_1best": bool(np.array_equal(pbest, best))}
        for v in (pairs["best"], pairs["sum"]):
            v["pairs_per_s"] = len(lines) / (v["kernel_ms"] * 1e-3)
            v["nodes_per_s"] = nodes / (v["kernel_ms"] * 1e-3)
    ppost = None
    if a.pairs_posterior:
        isym = np.asarray(w["isym"])
        other = [isym[p][isym[p] != 0] for p in paths]  # the tags of the line's best path
        d.sum_pairs(lines[:1000], other[:1000])
        d.posterior_pairs(lines[:1000], other[:1000])
        kms_t, wall_t, kms_p, wall_p = [], [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            psum = d.sum_pairs(lines, other)
            wall_t.append((time.perf_counter() - t0) * 1e3)
            kms_t.append(d.last_ms())
            t0 = time.perf_counter()
            qsum, counts = d.posterior_pairs(lines, other)
            wall_p.append((time.perf_counter() - t0) * 1e3)
            kms_p.append(d.last_ms())
        has = ~np.isneginf(qsum)
        ppost = {"sum": {"kernel_ms": float(np.median(kms_t)), "kernel_ms_all": kms_t, "call_ms": float(np.median(wall_t))},
                 "posterior": {"kernel_ms": float(np.median(kms_p)), "kernel_ms_all": kms_p, "call_ms": float(np.median(wall_p))},
                 "trellis_nodes": int(sum((len(x) + 1) * (len(y) + 1) for x, y in zip(lines, other))) * int(w["n_states"]),
                 "no_derivation": int((~has).sum()), "sums_equal_the_pair_sum": bool(qsum.tobytes() == psum.tobytes()),
                 "matched_count": float(counts[w["osym"] != 0].sum()),
                 "matched_positions_with_a_derivation": int(sum(len(x) for x, h in zip(lines, has) if h)),
                 "other_count": float(counts[w["isym"] != 0].sum()),
                 "other_positions_with_a_derivation": int(sum(len(y) for y, h in zip(other, has) if h))}
        for v in (ppost["sum"], ppost["posterior"]):
            v["pairs_per_s"] = len(lines) / (v["kernel_ms"] * 1e-3)
        ppost["posterior"]["kernel_ms_over_pair_sum"] = ppost["posterior"]["kernel_ms"] / ppost["sum"]["kernel_ms"]
    psamp = None
    if a.pairs_sample:
        N = a.pairs_sample
        isym, osym = np.asarray(w["isym"]), np.asarray(w["osym"])
        other = [isym[p][isym[p] != 0] for p in paths]  # the tags of the line's best path
        d.sum_pairs(lines[:1000], other[:1000])
        d.posterior_pairs(lines[:1000], other[:1000])
        d.sample_pairs_raw(lines[:1000], other[:1000], N, 1)
        kms_t, wall_t, kms_p, wall_p, kms_n, wall_n = [], [], [], [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            psum = d.sum_pairs(lines, other)
            wall_t.append((time.perf_counter() - t0) * 1e3)
            kms_t.append(d.last_ms())
            t0 = time.perf_counter()
            d.posterior_pairs(lines, other)
            wall_p.append((time.perf_counter() - t0) * 1e3)
            kms_p.append(d.last_ms())
            t0 = time.perf_counter()
            line_paths, logw, path_off, arcs = d.sample_pairs_raw(lines, other, N, 1)
            wall_n.append((time.perf_counter() - t0) * 1e3)
            kms_n.append(d.last_ms())
        with_paths = np.diff(line_paths) > 0
        # every sampled path spells its pair: its arcs' non-epsilon symbols, side by side, against the pairs' symbols repeated N times
        a64 = arcs.astype(np.int64)
        rep = lambda seqs: np.concatenate([np.tile(np.asarray(x, np.int64), N) for x, h in zip(seqs, with_paths) if h] + [np.zeros(0, np.int64)])
        spelt = bool(np.array_equal(osym[a64][osym[a64] != 0], rep(lines)) and np.array_equal(isym[a64][isym[a64] != 0], rep(other)))
        longest = max(min(len(x), len(y)) + 1 for x, y in zip(lines, other)) * int(w["n_states"])
        psamp = {"n_samples": N,
                 "sum": {"kernel_ms": float(np.median(kms_t)), "kernel_ms_all": kms_t, "call_ms": float(np.median(wall_t))},
                 "posterior": {"kernel_ms": float(np.median(kms_p)), "kernel_ms_all": kms_p, "call_ms": float(np.median(wall_p))},
                 "sample": {"kernel_ms": float(np.median(kms_n)), "kernel_ms_all": kms_n, "call_ms": float(np.median(wall_n))},
                 "trellis_nodes": int(sum((len(x) + 1) * (len(y) + 1) for x, y in zip(lines, other))) * int(w["n_states"]),
                 "tier": "lds" if 3 * longest <= 8192 else "global",  # (decided by the call's longest pair: decode_pairs.hip)
                 "paths": int(len(logw)), "path_arcs": int(len(arcs)),
                 "every_pair_with_a_sum_has_n_paths": bool(np.array_equal(with_paths, ~np.isneginf(psum)) and
                                                           (np.diff(line_paths)[with_paths] == N).all()),
                 "every_path_spells_its_pair": spelt}
        for v in (psamp["sum"], psamp["posterior"], psamp["sample"]):
            v["pairs_per_s"] = len(lines) / (v["kernel_ms"] * 1e-3)
        psamp["sample"]["kernel_ms_over_pair_sum"] = psamp["sample"]["kernel_ms"] / psamp["sum"]["kernel_ms"]
        psamp["sample"]["kernel_ms_over_pair_posterior"] = psamp["sample"]["kernel_ms"] / psamp["posterior"]["kernel_ms"]
    d.close()
    n_pos = int(sum(len(x) for x in lines))
    # matched relaxations: for every position, the arcs whose output is that symbol (each one add + compare)
    per_sym = np.bincount(w["osym"][w["logw"] > -np.inf].astype(np.int64))
    relax = int(sum(int(per_sym[x].sum()) if len(x) else 0 for x in [np.asarray(l, np.int64) for l in lines]))
    kms = float(np.median(ms))
    res = {"workload": "tagging decode (-r), %d lines, %d positions" % (len(lines), n_pos),
           "machine": {"states": int(w["n_states"]), "arcs": int(len(w["src"]))},
           "kernel_ms": kms, "kernel_ms_all": ms, "call_ms": float(np.median(wall)),
           "lines_per_s": len(lines) / (kms * 1e-3), "relaxations_per_s": relax / (kms * 1e-3), "relaxations": relax,
           "no_derivation": int(np.isneginf(best).sum())}
    if kbest:
        res["kbest"] = kbest
        for K, v in kbest.items():
            v["kernel_ms_over_1best"] = v["kernel_ms"] / kms
    cmds = {"cluster": ("cluster.data.noe", ["cat.fsa.trained.noe", "spellout.fst.trained"]),
            "tagging": ("tagging.data", ["tagging.fsa.trained.noe", a.fst]),
            "cipher": ("cipher.data", ["cipher.wfsa.noe", "cipher.fst.trained"])}
    e2e = {}
    for name, (data_file, members) in cmds.items():
        text = "".join(l + "\n" for l in open(gf(data_file)).read().split("\n") if l.split())
        t0 = time.perf_counter()
        p = subprocess.run([CLI, "-qbsriWIEk", "1"] + [gf(m) if not os.path.isabs(m) else m for m in members], input=text,
                           capture_output=True,
                           text=True, env=dict(os.environ, CARMEL_TIMING="1"), timeout=600)
        e2e[name] = {"rc": p.returncode, "seconds": time.perf_counter() - t0,
                     "timing": [l for l in p.stderr.split("\n") if l.startswith("timing: decode")]}
    res["end_to_end"] = e2e
    if sums:
        sums["kernel_ms_over_1best"] = sums["kernel_ms"] / kms
        res["sum"] = sums
    if samples:
        for v in samples.values():
            v["kernel_ms_over_sum"] = v["kernel_ms"] / sums["kernel_ms"]
            v["kernel_ms_over_1best"] = v["kernel_ms"] / kms
        res["sample"] = samples
    if a.sample:
        with open(a.sample_out, "w") as f:
            json.dump({"workload": res["workload"], "machine": res["machine"], "reps": a.reps,
                       "one_best": {"kernel_ms": kms, "kernel_ms_all": ms, "call_ms": res["call_ms"],
                                    "lines_per_s": res["lines_per_s"]}, "sum": sums, "sample": samples}, f)
            f.write("\n")
    if post:
        post["kernel_ms_over_sum"] = post["kernel_ms"] / sums["kernel_ms"]
        post["kernel_ms_over_sample_1"] = post["kernel_ms"] / samples["1"]["kernel_ms"]
        post["kernel_ms_over_1best"] = post["kernel_ms"] / kms
        res["posterior"] = post
        with open(a.posterior_out, "w") as f:
            json.dump({"workload": res["workload"], "machine": res["machine"], "reps": a.reps,
                       "one_best": {"kernel_ms": kms, "kernel_ms_all": ms, "call_ms": res["call_ms"],
                                    "lines_per_s": res["lines_per_s"]}, "sum": sums, "sample_1": samples["1"], "posterior": post}, f)
            f.write("\n")
    if pairs:
        pairs["best"]["kernel_ms_over_1best"] = pairs["best"]["kernel_ms"] / kms
        pairs["sum"]["kernel_ms_over_sum"] = pairs["sum"]["kernel_ms"] / sums["kernel_ms"]
        res["pairs"] = pairs
        with open(a.pairs_out, "w") as f:
            json.dump({"workload": res["workload"] + ", every line paired with the tags of its best path", "machine": res["machine"],
                       "reps": a.reps, "one_best": {"kernel_ms": kms, "kernel_ms_all": ms, "call_ms": res["call_ms"],
                                                    "lines_per_s": res["lines_per_s"]}, "sum": sums, "pairs": pairs}, f)
            f.write("\n")
    if ppost:
        res["pairs_posterior"] = ppost
        with open(a.pairs_posterior_out, "w") as f:
            json.dump({"workload": res["workload"] + ", every line paired with the tags of its best path", "machine": res["machine"],
                       "reps": a.reps, "pairs_posterior": ppost}, f)
            f.write("\n")
    if psamp:
        res["pairs_sample"] = psamp
        with open(a.pairs_sample_out, "w") as f:
            json.dump({"workload": res["workload"] + ", every line paired with the tags of its best path", "machine": res["machine"],
                       "reps": a.reps, "pairs_sample": psamp}, f)
            f.write("\n")
    if a.sum:
        with open(a.sum_out, "w") as f:
            json.dump({"workload": res["workload"], "machine": res["machine"], "reps": a.reps,
                       "one_best": {"kernel_ms": kms, "kernel_ms_all": ms, "call_ms": res["call_ms"],
                                    "lines_per_s": res["lines_per_s"]}, "sum": sums}, f)
            f.write("\n")
    shutil.rmtree(tmp)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
