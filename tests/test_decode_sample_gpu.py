"""GPU: batch posterior path sampling (carmel_hip_decode_sample, Decoder.sample, carmel -b --sample-paths=N;
csrc/decode_sample.hip) -- random machines against the reference of decode_sample_ref.py arc for arc (workload and reference:
decode_sample_cases.py, what they contain: test_decode_sample_host.py), empirical frequencies against the exact posterior, exact
small cases, the memory tiers and chunking, and the front end on the tutorial's cluster machines."""
import math

import numpy as np
import pytest

from decode_ref import decode_expected, golden_file
from decode_sample_cases import (FREQ_SEEDS, N_FREQ, N_RANDOM, SEED_FREQ, SEED_RANDOM, SEEDS, SIGMAS, case, check_frequencies,
                                 posterior, reference)
from decode_sample_ref import frequencies, is_derivation, paths_of, raw_line_matrix
from test_decode_gpu import check_random, lines_for, random_machine, run
from test_decode_host import noe

pytestmark = pytest.mark.gpu

TALLY = {"paths": 0, "ambiguous": 0}  # over test_random_machines_against_the_reference; the last test checks the share


def from_the_end(logw, path):
    w = 0.0
    for a in reversed(path):
        w = logw[a] + w
    return w


def within_sigmas(f, p, n):
    return abs(f - p) <= SIGMAS * (math.sqrt(p * (1.0 - p) / n) + 1.0 / n)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_machines_against_the_reference(hipopt, seed):
    from carmel_amd._capi import CarmelHipError
    from carmel_amd.decode import Decoder
    c = case(seed)
    w = c["w"]
    if c["lds_off"]:
        hipopt.set("decode_lds", "0")  # a small machine in the global tier
    ref_of = {side: (m, samples) for side, _, m, samples in reference(seed)}
    for side, lines, ref, _, _ in c["sides"]:
        d = Decoder(w, side=side)
        if ref is None:  # the epsilon arcs of this side have a cycle
            with pytest.raises(CarmelHipError, match="cycle") as e:
                d.sample(lines, N_RANDOM, SEED_RANDOM)
            assert e.value.code == -5  # CARMEL_HIP_ERR_UNSUPPORTED
            best, paths = d.decode(lines)  # the handle stays usable
            check_random(w, side, lines, best, paths)
            d.close()
            continue
        ws, paths = d.sample(lines, N_RANDOM, seed=SEED_RANDOM)
        sums = d.sum(lines)
        d.close()
        m, samples = ref_of[side]
        for l, line in enumerate(lines):
            if samples[l] is None:
                assert len(paths[l]) == 0 and len(ws[l]) == 0 and np.isneginf(sums[l]), (side, line)
                continue
            assert len(paths[l]) == N_RANDOM and len(ws[l]) == N_RANDOM and sums[l] > -np.inf, (side, line, len(paths[l]))
            mat, amb = samples[l]
            for s, (got, want) in enumerate(zip(paths[l], paths_of(mat))):
                got = [int(a) for a in got]
                assert is_derivation(m, line, got), (side, line, s, got)
                assert ws[l][s] == from_the_end(w.logw, got), (side, line, s, ws[l][s])
                TALLY["paths"] += 1
                if amb[s]:
                    TALLY["ambiguous"] += 1
                else:
                    assert got == want, (side, line, s, got, want)


def test_few_paths_were_left_out_as_ambiguous():
    """(over whichever cases of the test above ran in this process: 9 240 paths when all did)"""
    print("paths %(paths)d, left out as ambiguous %(ambiguous)d" % TALLY)
    assert TALLY["ambiguous"] <= 0.01 * TALLY["paths"], TALLY


@pytest.mark.parametrize("seed", FREQ_SEEDS)
def test_frequencies_against_the_exact_posterior(seed):
    from carmel_amd.decode import Decoder
    worst = 0.0
    for side, lines, post in posterior(seed):
        if not post:
            continue
        d = Decoder(case(seed)["w"], side=side)
        line_paths, _, path_off, arcs = d.sample_raw(lines, N_FREQ, SEED_FREQ)  # the whole workload: the lines keep their indices
        d.close()
        for l, exact in post.items():
            assert int(line_paths[l + 1] - line_paths[l]) == N_FREQ
            mat = raw_line_matrix(line_paths, path_off, arcs, l)
            worst = max(worst, check_frequencies(frequencies(mat), exact, N_FREQ, (seed, side, l)))
    print("seed %d: worst |f - p| in units of the bound's sigma: %.2f" % (seed, worst))


def share(paths, path):
    return sum(list(p) == path for p in paths) / float(len(paths))


def test_exact_cases():
    from carmel_amd._capi import CarmelHipError
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    # test_decode_sum_gpu.test_exact_cases' machine: 0 -1-> 1 twice (arcs 0 and 2), 0 -1-> 2, 1 -2-> 2
    lw = np.log([0.5, 0.25, 0.125, 0.5])
    w = Wfst(3, 2, [0, 0, 0, 1], [1, 2, 1, 2], [1, 1, 1, 2], [3, 4, 3, 5], lw)
    d = Decoder(w)
    lines = [[1, 2], [1], [2], [], [9]]
    n = 1000
    ws, paths = d.sample(lines, n, seed=3)
    assert [len(p) for p in paths] == [n, n, 0, 0, 0] and [len(x) for x in ws] == [n, n, 0, 0, 0]
    kinds = set(tuple(p) for p in paths[0])
    assert kinds == {(0, 3), (2, 3)}, kinds
    assert within_sigmas(share(paths[0], [0, 3]), 0.8, n), share(paths[0], [0, 3])
    for p, x in zip(paths[0], ws[0]):
        assert x == lw[p[0]] + (lw[3] + 0.0)
    assert all(list(p) == [1] for p in paths[1])
    assert d.last_ms() >= 0
    # the forward value the sampler used is the sum's: a line with one derivation reports that derivation's weight
    sums = d.sum(lines)
    assert ws[1][0] == sums[1] == lw[1] + 0.0
    assert np.isneginf(sums[2:]).all()
    # the entries alternate on one handle
    best, bpaths = d.decode(lines)
    assert list(bpaths[0]) == [0, 3]
    ws2, paths2 = d.sample(lines, n, seed=3)
    assert all(np.array_equal(a, b) for a, b in zip(ws, ws2))
    assert all(list(a) == list(b) for x, y in zip(paths, paths2) for a, b in zip(x, y))
    kw, _ = d.decode_kbest(lines, 4)
    assert len(kw[0]) == 2
    one_w, one = d.sample(lines, 1, seed=3)  # N = 1: sample 0 of the thousand
    assert [len(p) for p in one] == [1, 1, 0, 0, 0] and list(one[0][0]) == list(paths[0][0]) and one_w[0][0] == ws[0][0]
    for bad in (0, 65537):
        with pytest.raises(CarmelHipError) as e:
            d.sample(lines, bad)
        assert e.value.code == -1  # CARMEL_HIP_ERR_ARG
    assert d.sum(lines).tobytes() == sums.tobytes()
    new = lw.copy()
    new[2] = -np.inf  # a weight of zero removes the second derivation
    d.set_weights(new)
    _, paths3 = d.sample(lines, n, seed=3)
    assert len(paths3[0]) == n and all(list(p) == [0, 3] for p in paths3[0])
    d.close()
    # the empty line, and an epsilon arc into a state that matched arcs enter too: 0 -eps-> 1, 0 -1-> 1, 1 -1-> 1, final 1
    lw = np.log([0.5, 0.25, 0.125])
    w = Wfst(2, 1, [0, 0, 1], [1, 1, 1], [0, 1, 1], [0, 1, 1], lw)
    d = Decoder(w)
    ws, paths = d.sample([[], [1]], n, seed=4)
    d.close()
    assert len(paths[0]) == n and all(list(p) == [0] for p in paths[0]) and all(x == lw[0] + 0.0 for x in ws[0])
    assert set(tuple(p) for p in paths[1]) == {(1,), (0, 2)}
    assert within_sigmas(share(paths[1], [1]), 0.8, n), share(paths[1], [1])  # 0.25 against 0.5 x 0.125
    assert within_sigmas(share(paths[1], [0, 2]), 0.2, n)


def test_samples_are_deterministic(hipopt):
    """two runs, two chunkings of the batch and the two memory tiers give the same bytes; another seed does not"""
    from carmel_amd.decode import Decoder
    rng = np.random.default_rng(7)
    w = random_machine(rng, 40, 5, 160, p_eps=0.2, cyclic=False)
    lines = lines_for(rng, w, 0, 5, 300)
    d = Decoder(w)
    same = lambda a, b: all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    a = d.sample_raw(lines, 5, 11)
    assert int(a[0][-1]) >= 5 * 30 and len(a[1]) == int(a[0][-1]) and len(a[2]) == len(a[1]) + 1
    again = d.sample_raw(lines, 5, 11)
    other = d.sample_raw(lines, 5, 12)
    hipopt.set("decode_chunk_bytes", "4096")
    chunked = d.sample_raw(lines, 5, 11)
    hipopt.unset("decode_chunk_bytes")
    hipopt.set("decode_lds", "0")
    glob = d.sample_raw(lines, 5, 11)
    d.close()
    assert same(a, again) and same(a, chunked) and same(a, glob)
    assert a[0].tobytes() == other[0].tobytes() and not same(a, other)  # the same lines have paths; the paths differ


def test_front_end_sample_paths_on_the_cluster_machines(oracle, golden_dir, tmp_path):
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    gold = decode_expected(golden_dir)["cluster"]
    members = [golden_file(golden_dir, m, tmp_path) for m in ("cat.fsa.trained.noe", "spellout.fst.trained")]
    lines = noe(golden_dir, gold["data"])[:60]
    text = "".join(l + "\n" for l in lines)
    form = ["-qbsriWIE", "--sample-paths=3"]
    rc, out, err = run(form + ["-R", "7"] + members, stdin=text, env={"CARMEL_TIMING": "1"})
    assert rc == 0, err
    assert "timing: sample " in err and "timing: decode " not in err
    rep = [l for l in err.split("\n") if l and not l.startswith("timing:")]
    assert rep == ["Derivations found for all %d inputs." % len(lines)], rep  # no Viterbi line: no best path is computed
    printed = out.split("\n")[:-1]
    assert len(printed) == 3 * len(lines)
    rc2, out2, _ = run(form + ["-R", "7"] + members, stdin=text)
    rc8, out8, _ = run(form + ["-R", "8"] + members, stdin=text)
    assert rc2 == 0 and rc8 == 0 and out2 == out and out8 != out and len(out8.split("\n")) == len(out.split("\n"))
    # every printed line is the input side of a path whose output side spells the line: the same call on the oracle's
    # composition (lines on its output side, -r; seed 7) samples the same paths
    oc = oracle.OracleCascade([open(m).read() for m in members], remember=False)
    w = oc.composed().arrays()
    cp = oc.corpus("".join("%s\n%s\n" % (p, lines[k // 3]) for k, p in enumerate(printed))).arrays()
    seq = lambda name, k: [int(x) for x in cp[name + "_sym"][int(cp[name + "_off"][k]):int(cp[name + "_off"][k + 1])]]
    d = Decoder(Wfst(w["n_states"], w["final"], w["src"], w["dst"], w["isym"], w["osym"], w["logw"]), side=1)
    _, paths = d.sample([seq("out", 3 * l) for l in range(len(lines))], 3, seed=7)
    d.close()
    n_distinct = 0
    for l in range(len(lines)):
        assert len(paths[l]) == 3
        for s, p in enumerate(paths[l]):
            assert [int(x) for x in w["osym"][p] if x] == seq("out", 3 * l + s), (l, s)
            assert [int(x) for x in w["isym"][p] if x] == seq("in", 3 * l + s), (l, s, printed[3 * l + s])
        n_distinct += len(set(printed[3 * l:3 * l + 3])) > 1
    assert n_distinct  # (a posterior, not an arg-max)
    # with --sum-paths: stdout unchanged, the three sum lines of a -k 1 --sum-paths run
    rcs, outs, errs = run(form + ["-R", "7", "--sum-paths"] + members, stdin=text)
    rc1, _, err1 = run(["-qbsriWIEk", "1", "--sum-paths"] + members, stdin=text)
    assert rcs == 0 and rc1 == 0 and outs == out
    reps, rep1 = [l for l in errs.split("\n") if l], [l for l in err1.split("\n") if l]
    assert len(rep1) == 5 and reps == [rep1[0], rep1[1], rep1[2], rep1[4]], (reps, rep1)
    assert reps[3].startswith("Sum (all paths) ")
    # a line with an unknown symbol: three fill lines, counted
    some = lines[:5] + ["no_such_symbol"]
    rc, out, err = run(form + ["-R", "7"] + members, stdin="".join(l + "\n" for l in some))
    assert rc == 0, err
    got = out.split("\n")[:-1]
    assert len(got) == 18 and got[-3:] == ["", "", ""] and got[:15] == printed[:15]  # (a line's samples: its index, not its neighbours)
    assert [l for l in err.split("\n") if l] == ["No derivations found for 1 of 6 inputs."]
    rc, out, err = run(["-qbsriIE", "--sample-paths=3", "-R", "7"] + members, stdin="".join(l + "\n" for l in some))
    assert rc == 0 and out.split("\n")[-4:-1] == ["0", "0", "0"], err  # (without -W: print_kbest's fill line)
    # what is refused
    rc, out, err = run(form + ["--kbest=3"] + members, stdin=text)
    assert rc != 0 and out == "" and "--sample-paths" in err and "--kbest" in err
    rc, out, err = run(["-qbsriWIE", "-G", "3"] + members, stdin=text)
    assert rc != 0 and out == "" and "-G" in err


def test_front_end_refuses_sampling_over_an_epsilon_cycle(tmp_path):
    """test_front_end_refuses_the_sum_over_an_epsilon_cycle's machine: the library's error, no output"""
    m = tmp_path / "loop.fst"
    m.write_text("F\n(S (A a x 0.5))\n(A (B *e* *e* 0.5))\n(B (A *e* *e* 0.5))\n(A (F b y 0.5))\n")
    rc, out, err = run(["-qbsriWIE", "--sample-paths=3", "-R", "7", str(m)], stdin="x y\n")
    assert rc != 0 and out == ""
    assert "carmel_hip_decode_sample" in err and "cycle" in err
