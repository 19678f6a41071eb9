"""The sums over all paths of the whole machine (carmel --machine-sums, carmel_hip_decoder_machine_sums), what can be proved without
a device: the Python reference of the rule (machine_sums_ref.py) against an enumeration of all paths, the properties the case
machines of machine_sums_cases.py are named for, that every case's bound stays under the ceiling, the kernels' resources, the front
end's usage errors, and that -c prints what it printed."""
import math
import re

import numpy as np
import pytest

from machine_sums_cases import DEFAULT_WAVE_DEGREE, DEGREES, HAND, RANDOM_SEEDS, REFUSED, SINGLE_PATH, accepted, machine, names, reference
from machine_sums_ref import LD, NONE, U, enumerate_paths
from sweep_ref import CEILING
from test_decode_host import run, signed


ENUMERABLE = [n for n in accepted() if reference(n).N <= 10000]


@pytest.mark.parametrize("name", ENUMERABLE)
def test_reference_equals_the_enumeration_of_all_paths(name):
    """on every case of at most 10^4 paths: the count exactly, the sum to 1e-12, every arc's posterior as the share of the paths
    through it, and the posteriors of the arcs out of state 0 sum to 1"""
    w, ref = machine(name), reference(name)
    assert not ref.refused
    paths = enumerate_paths(w)
    assert paths is not None and len(paths) == ref.N, (name, ref.N)
    if not paths:
        assert ref.Z == -np.inf and ref.n_useful == 0 and all(g == -np.inf for g in ref.ln_gamma)
        return
    pw = [sum((LD(w.logw[k]) for k in p), LD(0.0)) for p in paths]
    top = max(pw)
    total = top + np.log(sum((np.exp(x - top) for x in pw), LD(0.0)))
    assert abs(total - ref.Z) <= 1e-12, (name, float(total), float(ref.Z))
    assert abs(ref.beta[0] - ref.Z) <= 1e-12
    through = [LD(0.0)] * w.n_arcs
    for p, x in zip(paths, pw):
        for k in p:
            through[k] += np.exp(x - total)
    for k in range(w.n_arcs):
        assert abs(np.exp(ref.ln_gamma[k]) - through[k]) <= 1e-12, (name, k)
        assert (through[k] > 0) == ref.arc_useful[k]
    if w.final != 0:
        assert abs(sum(np.exp(ref.ln_gamma[k]) for k in range(w.n_arcs) if w.src[k] == 0) - 1) <= 1e-12
    on_path = {0} | {int(w.dst[k]) for p in paths for k in p}
    assert on_path == {q for q in range(w.n_states) if ref.useful[q]}
    longest = max(len(p) for p in paths)
    assert ref.levels == (longest + 1, longest + 1) and ref.level[w.final] == longest


@pytest.mark.parametrize("name", names())
def test_every_bound_stays_under_the_ceiling(name):
    """a condition on the chosen cases: a case that broke it would be changed, not the ceiling"""
    ref = reference(name)
    assert ref.worst_bound() < CEILING, (name, float(ref.worst_bound()))
    if not ref.refused:
        assert ref.E[0] == 0 and ref.Eb[machine(name).final] == 0  # the constants 0.0


def test_the_cases_are_what_their_names_say():
    assert reference("grid").N == math.comb(10, 5) == 252
    assert reference("layers").N == 3 ** 40 > 2 ** 53
    hub, big = reference("hub"), reference("level5000")
    assert hub.N == 200 and hub.F.degree[201] == 200 and hub.B.degree[0] == 200 and hub.levels == (3, 3)
    assert big.N == 5000 and big.levels == (3, 3) and sum(1 for l in big.level if l == 1) == 5000
    deep = reference("chain3000")
    assert deep.levels == (3000, 3000) and deep.N == 1 and deep.E[2999] < 1e-11
    deg = reference("degrees")
    for form in (deg.F, deg.B):  # a state of every degree in both directions, on both sides of every threshold
        assert set(DEGREES) <= set(form.degree)
    assert {DEFAULT_WAVE_DEGREE, DEFAULT_WAVE_DEGREE + 1, 8, 9, 64, 65} <= set(DEGREES)
    assert max(machine("positive").logw) > 0 and reference("positive").Z > 0
    assert (machine("neg_inf").logw == -np.inf).sum() == 3 and reference("neg_inf").N == reference("diamond").N == 2
    assert reference("neg_inf").Z == reference("diamond").Z
    for name in ("final0", "single_state"):
        r = reference(name)
        assert r.Z == 0 and r.N == 1 and r.n_useful == 1 and r.levels == (1, 1)
    for name in ("unreachable_final", "no_arcs"):
        r = reference(name)
        assert r.Z == -np.inf and r.N == 0 and r.n_useful == 0 and r.levels == (0, 0) and set(r.level) == {NONE}
    for name in ("cycle_dead_end", "cycle_unreachable"):  # a cycle, but not among the useful states
        r = reference(name)
        assert not r.refused and r.N == 2 and r.n_useful == 4 and r.Z == reference("diamond").Z
    assert {n: reference(n).stuck for n in REFUSED} == REFUSED
    assert reference("cycle_in_u").stuck not in (4, 5)  # the named state lies behind the cycle, not on it
    for name in SINGLE_PATH:
        assert reference(name).N == 1
    live = [s for s in RANDOM_SEEDS if reference("random%d" % s).N > 1]
    assert len(live) >= 12, live  # most random machines have several paths
    w = [machine("random%d" % s) for s in RANDOM_SEEDS]
    assert all(m.n_states <= 60 for m in w) and any((m.logw == -np.inf).any() for m in w) and any(m.logw.max() > 0 for m in w)
    assert any(not all(reference("random%d" % s).useful) and reference("random%d" % s).n_useful > 2 for s in RANDOM_SEEDS)
    assert "layers" not in ENUMERABLE and {"grid", "hub", "level5000", "chain3000"} <= set(ENUMERABLE) < set(accepted())
    assert set(HAND) >= {"chain5", "diamond", "grid", "hub", "level5000", "chain3000", "layers", "positive", "neg_inf", "final0"}


def test_machine_sums_kernels_use_no_scratch_memory():
    from test_kernel_resources import device_asm, kernels
    ks = {k: v for k, v in kernels(device_asm("decode_machine_sums.hip")).items() if "ms_" in k and "_kernel" in k}
    assert len(ks) == 9, list(ks)
    for name, (body, tail) in ks.items():
        m = re.search(r"; ScratchSize: (\d+)", tail)
        assert m and int(m.group(1)) == 0, (name, m and m.group(0))


def G(golden_dir, name):
    import os
    return os.path.join(golden_dir, name)


REFUSALS = [(["-b"], "-b"), (["-i"], "-i"), (["-s"], "-s"), (["-r"], "-r"), (["-t"], "-t"), (["--train-cascade"], "--train-cascade"),
            (["--crp"], "--crp"), (["-S"], "-S"), (["-k", "2"], "-k"), (["--best-paths=2"], "--best-paths=N"),
            (["--generate-paths=2", "-I"], "--generate-paths=N"), (["--generate-pairs=2"], "--generate-pairs=N"),
            (["--generate-max-arcs=5"], "--generate-max-arcs=L"), (["--generate-tries=5"], "--generate-tries=T"),
            (["--pair-lines=x"], "--pair-lines=FILE")]


@pytest.mark.parametrize("option", ["--machine-sums", "--machine-counts=FILE"])
@pytest.mark.parametrize("args,what", REFUSALS)
def test_machine_sums_usage_errors(golden_dir, tmp_path, option, args, what):
    """each exits -12 naming the option and what it does not go with, before any device call; nothing is written"""
    target = tmp_path / "counts.fst"
    given = option.replace("FILE", str(target))
    rc, out, err = run([given] + args + [G(golden_dir, "train.a.w")])
    assert signed(rc) == -12, err
    assert "HIP" not in err and out == "" and not target.exists()
    assert "%s with %s is not implemented" % (option, what) in err, err


def test_machine_counts_needs_a_file_name_and_sum_names_the_new_option(golden_dir):
    rc, out, err = run(["--machine-counts=", G(golden_dir, "train.a.w")])
    assert signed(rc) == -12 and "--machine-counts=FILE needs a file name" in err and out == ""
    rc, out, err = run(["--sum", G(golden_dir, "train.a.w")])  # carmel's own spelling stays refused; the hint names both switches
    assert signed(rc) == -12 and "--sum is not implemented under that name" in err and "--sum-paths" in err and "--machine-sums" in err
    rc, out, err = run(["-h"])
    assert rc == 0 and "--machine-sums" in out and "--machine-counts=FILE" in out


ACYCLIC = """3
(0 (1 a a 0.5) (1 b b 0.25) (2 a a 0.125))
(1 (2 a a 0.5) (3 b b 0.1))
(2 (3 a a 0.9) (3 b b 0.3))
(3)
"""


def test_a_valid_command_reaches_the_device(golden_dir, tmp_path):
    """on a machine without a cycle (the tutorial machines have one among their useful states): with a device the two lines, 8 paths;
    without one the library's error, not a usage error"""
    from carmel_amd._capi import lib
    machine_file = str(tmp_path / "acyclic.fsa")
    with open(machine_file, "w") as f:
        f.write(ACYCLIC)
    for args in (["--machine-sums"], ["--machine-counts=%s" % (tmp_path / "c.fst")], ["-C", "--machine-sums"],
                 ["--prune-paths=1000", "--machine-sums", "-Z"]):
        rc, out, err = run(["-q"] + args + [machine_file])
        if lib.carmel_hip_device_count() > 0:
            assert rc == 0 and out.startswith("Number of paths in result: 8\nSum of all paths in result: "), (out, err)
        else:
            assert signed(rc) == -11 and "no HIP device" in err and "not implemented" not in err, err


def test_c_prints_its_two_lines_as_before(golden_dir):
    """-c stays the report of states and arcs: the path count is --machine-sums' line, not a third line here"""
    for members in (["train.a.w"], ["cat.fsa.trained.noe", "spellout.fst.trained"]):
        rc, out, err = run(["-q", "-c"] + [G(golden_dir, m) for m in members])
        assert rc == 0, err
        assert re.fullmatch(r"Number of states in result: \d+\nNumber of arcs in result: \d+\n", out), out


def test_the_abi_without_a_device_or_a_handle():
    """a null handle is CARMEL_HIP_ERR_ARG from all four entry points, with or without a device"""
    import ctypes as C
    from carmel_amd._capi import lib
    z, n, u = C.c_double(7.0), C.c_double(7.0), C.c_uint64(7)
    assert lib.carmel_hip_decoder_machine_sums(None, C.byref(z), C.byref(n), C.byref(u)) == -1
    assert (z.value, n.value, u.value) == (7.0, 7.0, 7)
    assert lib.carmel_hip_decoder_machine_sums_states(None, None, None, None, None, None) == -1
    assert lib.carmel_hip_decoder_machine_sums_arcs(None, None) == -1
    assert lib.carmel_hip_decoder_machine_sums_stats(None, None, None) == -1
    assert b"carmel_hip_decoder_machine_sums_stats" in lib.carmel_hip_last_error()
