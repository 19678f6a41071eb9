"""CPU: pair decoding (carmel --post-b; carmel_hip_decode_pairs, carmel_hip_decode_pairs_sum) -- the numpy reference
(decode_pairs_ref.py) proved three ways (against exhaustive enumeration, against the CPU oracle's composition-based lattices, in
f64 against longdouble), what the GPU test's random workload contains, the front end's --pair-lines / --pair-alignments switches
where no device is needed, and the kernels' resources.  Nothing here needs a GPU.

The tolerance is the sum tests' RTOL = 1e-10 max(1, |ref|) (test_decode_sum_gpu.py derives it: one rounding of a value of
magnitude <= ~1e2 per dependent trellis step and a few ulp per read-out); a pair has at most (n + m + 1)(levels + 1) dependent
steps with n, m <= 14, fewer than 6 levels: below 1e-11.  Measured worst errors: profiles/measurement_log_decode_pairs.md."""
import os
import re

import numpy as np
import pytest

from decode_pairs_cases import MAX_LEN, SEEDS, case
from decode_pairs_ref import CycleError, Prepared, count, enumerate_paths, pair_best, pair_sum, rescore
from test_decode_host import run, signed
from test_kernel_resources import device_asm, kernels

RTOL = 1e-10


def close_enough(got, ref):
    return abs(got - ref) <= RTOL * max(1.0, abs(ref))


def tiny_machine(rng):
    """2 .. 6 states, <= 16 arcs, symbols 1 and 2 on either side, 00 arcs only forward in state order (0M and M0 arcs may loop),
    some arcs of weight zero"""
    Q = int(rng.integers(2, 7))
    n = int(rng.integers(Q, 17))
    src = np.sort(rng.integers(0, Q, n))
    dst = rng.integers(0, Q, n)
    msym = rng.integers(0, 3, n)
    osym = rng.integers(0, 3, n)
    both = (msym == 0) & (osym == 0) & (dst <= src)
    msym[both] = 1
    logw = np.log(rng.uniform(0.01, 1.0, n))
    logw[rng.uniform(size=n) < 0.05] = -np.inf
    return Prepared(Q, Q - 1, src, dst, msym, osym, logw)


@pytest.mark.parametrize("seed", range(40))
def test_reference_equals_exhaustive_enumeration(seed):
    rng = np.random.default_rng(1900 + seed)
    P = tiny_machine(rng)
    line = lambda: [int(s) for s in rng.integers(1, 3, rng.integers(0, 5))]
    checked = 0
    for x, y in [([], [])] + [(line(), line()) for _ in range(10)]:
        every = enumerate_paths(P, x, y, limit=1024)
        if every is None:  # (more than 1024 derivations: not enumerated)
            continue
        checked += 1
        assert count(P, x, y) == len(every), (x, y)
        got, (best, path, tied) = pair_sum(P, x, y), pair_best(P, x, y)
        if not every:
            assert got == -np.inf and best == -np.inf and path is None, (x, y)
            continue
        fwd = [rescore(P, x, y, p)[0] for p in every]
        want = float(np.logaddexp.reduce(np.array(fwd, np.longdouble)))
        assert close_enough(got, want), (x, y, got, want)
        assert best == max(fwd) and rescore(P, x, y, path)[0] == best, (x, y)  # max is exact: bit for bit
        assert tied == (sum(f == best for f in fwd) > 1) or tied, (x, y)  # (a tie at a node of the path may not reach the end)
        if not tied:
            assert path == every[int(np.argmax(fwd))]
    assert checked >= 6


def test_reference_refuses_a_00_cycle_and_takes_a_0m_loop():
    # 0 -a:b-> 1, 1 -e:e-> 2, 2 -e:e-> 1, 1 -e:c-> 1
    args = (3, 1, [0, 1, 1, 2], [1, 2, 1, 1], [1, 0, 0, 0], [2, 0, 3, 0])
    with pytest.raises(CycleError):
        Prepared(*args, np.log([0.5, 0.5, 0.5, 0.5]))
    P = Prepared(*args, [np.log(0.25), np.log(0.5), np.log(0.5), -np.inf])  # an arc of weight zero is no arc: no cycle
    assert pair_sum(P, [1], [2, 3, 3]) == np.log(0.25) + np.log(0.5) + np.log(0.5)
    assert count(P, [1], [2, 3, 3]) == 1 and pair_best(P, [1], [2, 3, 3])[1] == [0, 2, 2]
    assert count(P, [1], [2, 3, 1]) == 0 and pair_sum(P, [1], [3]) == -np.inf


def small_seeds():
    return [s for s in SEEDS if s % 10 and case(s)["P"] is not None]


def test_reference_equals_the_oracle_lattice(oracle):
    """the same pairs through the CPU oracle's E-step: a lattice per pair built by composition, an independent route"""
    from carmel_amd.model import Corpus
    worst, n = 0.0, 0
    for s in small_seeds():
        c = case(s)
        pairs = [(y, x) if c["side"] else (x, y) for x, y in c["pairs"]]  # the corpus is (input, output)
        r = oracle.estimate(oracle.OracleWfst.from_arrays(c["w"]), oracle.OracleCorpus.from_arrays(Corpus.from_lists(pairs)))
        has = np.array([k > 0 for k in c["count"]])
        assert np.array_equal(has, r["has_deriv"]), s
        for got, ref in zip(c["sum"][has], r["pair_logprob"][has]):
            assert close_enough(got, ref), (s, got, ref)
            worst, n = max(worst, abs(got - ref) / max(1.0, abs(ref))), n + 1
    print("reference against the oracle: %d pairs, worst relative difference %.3g" % (n, worst))
    assert n >= 800


def test_reference_in_f64_equals_longdouble():
    worst, n = 0.0, 0
    for s in SEEDS:
        c = case(s)
        if c["P"] is None:
            continue
        for (x, y), got in zip(c["pairs"], c["sum"]):
            ref = pair_sum(c["P"], x, y, np.longdouble)
            best = pair_best(c["P"], x, y, np.longdouble)[0]
            assert (got == -np.inf) == (ref == -np.inf) == (best == -np.inf)
            if got > -np.inf:
                assert close_enough(got, float(ref)), (s, x, y, got, ref)
                worst, n = max(worst, abs(got - float(ref)) / max(1.0, abs(float(ref)))), n + 1
    print("reference f64 against longdouble: %d pairs, worst relative difference %.3g" % (n, worst))
    assert n >= 800


def test_gpu_test_inputs_really_pair():
    """the conditions on test_decode_pairs_gpu.py's random workload (over the pairs of the machines without a 00 cycle)"""
    n = with_d = several = differ = shorter = longer = levels = loops_cyclic = cycles = tied = 0
    for s in SEEDS:
        c = case(s)
        pairs = c["pairs"]
        assert len(pairs) == (6 if s % 10 == 0 else 16) and all(len(x) <= MAX_LEN and len(y) <= MAX_LEN for x, y in pairs)
        assert pairs[0] == ([], []) and max(pairs[1][0]) > 6 and max(pairs[2][1]) > 6  # (the symbols are 1 .. V <= 5)
        if c["P"] is None:
            cycles += 1
            continue
        levels = max(levels, c["P"].n_levels)
        loops_cyclic += c["loop"] and c["matched_cyclic"]
        assert c["count"][1] == 0 and c["count"][2] == 0
        for (x, y), k, (best, path, t) in zip(pairs, c["count"], c["best"]):
            n += 1
            assert (k > 0) == (path is not None)
            if k:
                with_d += 1
                several += k > 1
                differ += len(x) != len(y)
                shorter += len(x) < len(y)
                longer += len(x) > len(y)
                tied += t
    print("pairs %d: with a derivation %.0f %%, with several %.0f %%, of those with one n != m %.0f %% (n < m %d, n > m %d), tied %d; "
          "highest 00 level %d; 0M-loop machines with a matched-side epsilon cycle %d; machines with a 00 cycle %d"
          % (n, 100.0 * with_d / n, 100.0 * several / n, 100.0 * differ / with_d, shorter, longer, tied, levels, loops_cyclic, cycles))
    assert with_d >= 0.60 * n
    assert several >= 0.08 * n
    assert differ >= 0.30 * with_d and shorter and longer
    assert levels >= 2
    assert loops_cyclic >= 1 and cycles >= 1
    assert sum(case(s)["w"].n_states > 4096 for s in SEEDS) == 10 and sum(case(s)["lds_off"] for s in SEEDS) == 10


G = lambda golden_dir, n: os.path.join(golden_dir, n)
MACHINES = ["cat.fsa.trained.noe", "spellout.fst.trained"]


@pytest.mark.parametrize("args,word", [
    (["-qbsriWIE", "--kbest=3", "--pair-lines=x"], "--pair-lines"),
    (["-qbsriWIE", "--sample-paths=3", "--pair-lines=x"], "--pair-lines"),
    (["-qbsriWIEk", "1", "--posterior-counts=c", "--pair-lines=x"], "--pair-lines"),
    (["-q", "-t", "--pair-lines=x"], "--pair-lines"),
    (["-q", "-S", "--pair-lines=x"], "--pair-lines"),
    (["-qbsriWIEk", "1", "-t", "--pair-lines=x"], "--pair-lines"),
    (["-q", "--pair-lines=x"], "--pair-lines"),
    (["-qbsriWIEk", "1", "--pair-lines="], "--pair-lines"),
    (["-qbsriWIEk", "1", "--pair-alignments=a"], "--pair-alignments"),
    (["-q", "--pair-alignments=a"], "--pair-alignments"),
])
def test_pair_switches_out_of_place_are_refused(golden_dir, args, word):
    rc, out, err = run(args + [G(golden_dir, m) for m in MACHINES], stdin="c1 c2\n")
    assert signed(rc) == -12, err
    assert word in err and "HIP" not in err
    assert out == ""


def test_post_b_is_still_refused(golden_dir):
    rc, out, err = run(["-qbsriWIEk", "1", "--post-b=x"] + [G(golden_dir, m) for m in MACHINES], stdin="c1 c2\n")
    assert signed(rc) == -12, err
    assert "--post-b" in err and "not implemented" in err and "HIP" not in err


@pytest.mark.parametrize("form", [["-qbsriWIEk", "1"], ["-qbsriWIEk", "1", "--sum-paths"], ["-qsriWIEk", "1"],
                                  ["-qbsrOEk", "1", "--pair-alignments=%s"]])
def test_pair_lines_get_past_the_switches(golden_dir, tmp_path, form):
    """--pair-lines with -k 1 batch decoding fails only where the device is needed (-11, "no HIP device"); with a GPU it succeeds"""
    from carmel_amd._capi import lib
    other = tmp_path / "other"
    other.write_text("c1\n")
    form = [f % (tmp_path / "align") if "%s" in f else f for f in form]
    rc, out, err = run(form + ["--pair-lines=%s" % other] + [G(golden_dir, m) for m in MACHINES], stdin="c1 c2\n")
    if lib.carmel_hip_device_count() > 0:
        assert rc == 0, err
        assert len(out.split("\n")) == 2 and "Viterbi (best path) product of probs=" in err
        return
    assert signed(rc) == -11, err
    assert "not implemented" not in err and "no HIP device" in err and "carmel_hip_decoder_create" in err


def test_a_short_pair_file_ends_the_run_before_decoding(golden_dir, tmp_path):
    other = tmp_path / "other"
    other.write_text("c1\n")
    rc, out, err = run(["-qbsriWIEk", "1", "--pair-lines=%s" % other] + [G(golden_dir, m) for m in MACHINES], stdin="c1 c2\nc1\n")
    assert signed(rc) == -3, err
    assert "--pair-lines file didn't have as many lines as -b file." in err and out == ""


def test_help_names_the_pair_switches():
    rc, out, err = run(["-h"])
    assert rc == 0 and "--pair-lines" in out and "--pair-alignments" in out


def test_pair_kernels_use_no_scratch_memory():
    ks = kernels(device_asm("decode_pairs.hip"))
    assert len(ks) == 6, list(ks)  # the trellis around its two accumulators in its two tiers, the walk's two passes
    assert sum("pair_trellis_kernel" in k and "BestAcc" in k for k in ks) == 2
    assert sum("pair_trellis_kernel" in k and "SumAcc" in k for k in ks) == 2
    assert sum("pair_walk_kernel" in k for k in ks) == 2
    for name, (body, tail) in ks.items():
        m = re.search(r"; ScratchSize: (\d+)", tail)
        assert m and int(m.group(1)) == 0, (name, m and m.group(0))
        assert "scratch_" not in body, name
