"""Pruning the whole machine by best-path weight (carmel --prune-paths / --prune-states / --prune-arcs, carmel_hip_decoder_prune),
what can be proved without a device: the Python reference of the rule (prune_ref.py) against a brute-force enumeration of all
paths where every sum is exact, its forward pass against best_paths_ref's K = 1 lists, the `ulp` case, the cap's order, the
kernels' resources, and the front end's usage errors.  Transducer::keep is tested through the front end on a device
(test_prune_cli_gpu.py), not by a stand-alone program."""
import os

import numpy as np
import pytest

import best_paths_ref
from best_paths_cases import RANDOM_SEEDS
from prune_cases import LOG_RATIOS, MIN_ARC_LOGWS, OWN, dag_case, distances, grid, machine, max_states_grid, names, reference, ulp, ulp_property
from prune_ref import NO_CAP, Distances, all_paths, machines, prune
from test_decode_host import run, signed

NEG_INF = -np.inf


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_reference_equals_the_enumeration_on_acyclic_dyadic_machines(seed):
    """log weights -m / 8: every sum is exact, whatever its order, so T(a) is the weight of the best path through a and an arc
    is kept iff some path through it has a weight >= best / ratio (the limit F[final] - log_ratio rounded once, as the rule has
    it); a state likewise.  No cap."""
    w = dag_case(seed)
    for min_arc_logw in (NEG_INF, -1.0):
        m, _ = machines(w, min_arc_logw)
        paths = all_paths(m)
        assert paths or min_arc_logw > NEG_INF
        best = max([v for v, _ in paths] + [NEG_INF])
        d = Distances(w, min_arc_logw)
        assert d.F[m.final] == best
        for log_ratio in LOG_RATIOS + (0.5, 1.0):
            limit = NEG_INF if log_ratio == np.inf else best - log_ratio
            good = [p for v, p in paths if v >= limit]
            state_keep, arc_keep = d.masks(log_ratio)
            if log_ratio == np.inf:  # no ratio test: every arc that exists stays, on a path or not
                assert arc_keep.tolist() == [int(x > NEG_INF and bool(paths)) for x in m.logw]
                continue
            want_arcs = {a for p in good for a in p}
            want_states = {m.src[a] for a in want_arcs} | {m.dst[a] for a in want_arcs} | ({0} if good else set())
            assert set(np.flatnonzero(arc_keep)) == want_arcs, (seed, log_ratio)
            assert set(np.flatnonzero(state_keep)) == want_states, (seed, log_ratio)


@pytest.mark.parametrize("name", [n for n in names() if n not in ("medium", "hub", "chain")])
def test_forward_pass_is_the_best_paths_list_at_k_1(name):
    """F's entries are best_paths_ref's K = 1 lists, field for field, and P* is its one path"""
    w = machine(name)
    d = distances(name, NEG_INF)
    lists = best_paths_ref.rounds(best_paths_ref.Machine(w), 1)[0]
    assert [None if not l else l[0][:3] for l in lists] == d.fwd
    got = best_paths_ref.read_out(d.m, lists)
    assert [p for _, _, p in got] == ([d.pstar] if got else [])


def test_the_ulp_case_has_the_property_and_keeps_the_best_path():
    w = ulp()
    d = Distances(w)
    below = ulp_property(w)
    assert below and all(d.T_arc[a] < d.F[w.final] for a in below)
    assert all(abs(d.T_arc[a] - d.F[w.final]) < 1e-12 for a in below)  # (by rounding alone)
    state_keep, arc_keep = d.masks(0.0)
    assert all(arc_keep[a] for a in d.pstar)
    assert all(state_keep[q] for a in d.pstar for q in (d.m.src[a], d.m.dst[a]))
    assert arc_keep.sum() == len(d.pstar)  # and nothing else: the detours are far worse


@pytest.mark.parametrize("name", ["cap_tie", "medium", "hub", "random3", "dyadic11", "final_is_start"])
def test_the_cap_keeps_the_first_states_of_the_stated_order(name):
    """before the ratio test: with no ratio test, exactly min(max_states, |Q|) states by (T(q) descending, state id ascending) --
    unless an endpoint is among the lost ones, when nothing stays"""
    w = machine(name)
    d = distances(name, NEG_INF)
    T = np.array(d.T_state)
    order = sorted(range(w.n_states), key=lambda q: (-T[q], q))
    assert order == d.order
    for n in max_states_grid(w.n_states) + (w.n_states, w.n_states + 5):
        state_keep, _ = d.masks(np.inf, n)
        first = order[:min(n, w.n_states)]
        if 0 in first and w.final in first:
            assert sorted(np.flatnonzero(state_keep)) == sorted(first), (name, n)
        else:
            assert not state_keep.any(), (name, n)
    if name == "cap_tie":
        state_keep, arc_keep = d.masks(np.inf, 3)
        assert T[2] == T[3] and state_keep.tolist() == [1, 1, 1, 0, 0]
        assert [(d.m.src[a], d.m.dst[a]) for a in np.flatnonzero(arc_keep)] == [(0, 2), (2, 1)]


def test_hand_made_edges():
    s, a, F, R = prune(machine("unreachable"))
    assert not s.any() and not a.any() and F[2] == NEG_INF and R[2] == 0.0
    s, a, F, R = prune(OWN["final_is_start"], 0.0)
    assert s.tolist() == [1, 0, 0] and not a.any() and F[0] == R[0] == 0.0  # the empty path alone
    s, a, _, _ = prune(OWN["zero_self_loop"], 0.0)
    assert s.tolist() == [1, 1, 1] and a.tolist() == [1, 0, 1, 1]  # the loop and both arcs of P*; the direct arc is worse
    s, a, _, _ = prune(OWN["zero_self_loop"], np.inf, NO_CAP, float(np.log(0.25)))
    assert a.tolist() == [1, 0, 1, 1]  # ln 0.125 < ln 0.25: the direct arc does not exist
    for name in names():  # the grid's references exist and the masks agree with themselves
        for r, n, p in grid(name)[:4]:
            state_keep, arc_keep = reference(name, r, n, p)
            d = distances(name, p)
            assert all(state_keep[d.m.src[k]] and state_keep[d.m.dst[k]] for k in np.flatnonzero(arc_keep))
    assert len(MIN_ARC_LOGWS) == 2


def test_prune_kernels_use_no_scratch_memory():
    import re
    from test_kernel_resources import device_asm, kernels
    ks = {k: v for k, v in kernels(device_asm("decode_prune.hip")).items() if "prune_" in k and "hipcub" not in k and "rocprim" not in k}
    assert len(ks) == 10, list(ks)
    for name, (body, tail) in ks.items():
        m = re.search(r"; ScratchSize: (\d+)", tail)
        assert m and int(m.group(1)) == 0, (name, m and m.group(0))
        assert "scratch_" not in body, name


def G(golden_dir, name):
    return os.path.join(golden_dir, name)


@pytest.mark.parametrize("args,needle", [
    (["-w", "2"], "--prune-paths"), (["-z", "3"], "--prune-states"), (["-p", "0.1"], "--prune-arcs"),
    (["--prune-states=0"], "--prune-states=N needs"), (["--prune-states=x"], "--prune-states=N needs"),
    (["--prune-paths=abc"], "--prune-paths=W needs a weight"), (["--prune-arcs="], "--prune-arcs=W needs a weight"),
    (["--prune-paths=2", "-b"], "--prune-paths=W with -b is"), (["--prune-paths=2", "-i"], "--prune-paths=W with -i is"),
    (["--prune-states=3", "-t"], "--prune-states=N with -t is"), (["--prune-arcs=0.1", "-S"], "--prune-arcs=W with -S is"),
    (["--prune-paths=2", "--train-cascade"], "--prune-paths=W with --train-cascade is"),
    (["--prune-paths=2", "--crp"], "--prune-paths=W with --crp is"),
    (["--prune-states=3", "--best-paths=2"], "--prune-states=N with --best-paths=N is"),
    (["--prune-paths=2", "--generate-paths=2", "-I"], "--prune-paths=W with --generate-paths=N is"),
    (["--prune-arcs=0.1", "--generate-pairs=2"], "--prune-arcs=W with --generate-pairs=N is"),
])
def test_prune_usage_errors(golden_dir, args, needle):
    """each exits -12 naming the long option (and what it does not go with), before any device call"""
    rc, out, err = run(args + [G(golden_dir, "train.a.w")])
    assert signed(rc) == -12, err
    assert "HIP" not in err and out == ""
    assert needle in err, err


def test_a_valid_command_reaches_the_device(golden_dir):
    from carmel_amd._capi import lib
    for args in (["--prune-paths=2"], ["--prune-states=3", "-c"], ["--prune-arcs=0.1", "--prune-paths=e^1"]):
        rc, out, err = run(["-q"] + args + [G(golden_dir, "train.a.w")])
        if lib.carmel_hip_device_count() > 0:
            assert rc == 0 and out, err
        else:
            assert signed(rc) == -11 and "no HIP device" in err and "not implemented" not in err, err
    rc, out, err = run(["-h"])
    assert rc == 0 and all(x in out + err for x in ("--prune-paths=W", "--prune-states=N", "--prune-arcs=W"))
