"""What the generation tests share (test_decode_generate_host.py proves it on the CPU, test_decode_generate_gpu.py compares the
device with it): small machines (|Q| <= 8, <= 40 arcs) -- hand-made ones for the edges of the rule, random ones of
test_decode_gpu.random_machine -- each with its cap L on a path's arcs, the reference's paths of decode_generate_ref.py for the
committed workload, and for the frequency tests the (machine, mode) with 2 .. 64 accepted paths and their exact distribution.
Computed once."""
import functools

import numpy as np

from carmel_amd.model import Wfst
from decode_generate_ref import CONDITIONAL, JOINT, Machine, enumerate_paths, generate
from decode_sample_cases import check_frequencies  # noqa: F401
from test_decode_gpu import random_machine

MODES = (JOINT, CONDITIONAL)
N_PATHS, SEED, TRIES = 200, 2024, 64      # the equality workload: per (machine, mode) 200 paths, at most 64 attempts each
N_FREQ, SEED_FREQ, L_FREQ = 4000, 777, 4  # the frequency tests: 4000 paths; random machines with at most 4 arcs a path
RANDOM_SEEDS = range(40)
LN = np.log
ZERO = -np.inf


def _hand():
    """-> {name: (Wfst, L)}; symbols: input a b c = 1 2 3, output x y z = 1 2 3, 0 = epsilon"""
    h = {}
    # the start state is final: every path is empty, whatever leaves the state
    h["start_is_final"] = (Wfst(1, 0, [0], [0], [1], [1], LN([0.5])), 5)
    # one state with a self-loop and an exit
    h["loop_and_exit"] = (Wfst(2, 1, [0, 0], [0, 1], [1, 2], [1, 2], LN([0.6, 0.4])), 6)
    # a state with a single arc, then a choice
    h["single_arc"] = (Wfst(3, 2, [0, 1, 1], [1, 2, 2], [1, 1, 2], [1, 2, 2], LN([0.3, 0.25, 0.75])), 5)
    # a zero-weight arc first and last in a list (and, conditionally, first and last in the group of symbol a)
    h["zero_first_and_last"] = (Wfst(2, 1, [0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 2, 1], [1, 2, 3, 1, 2],
                                     [ZERO, LN(0.3), LN(0.7), LN(0.5), ZERO]), 3)
    # a dead-end state: half of the joint attempts are rejected there
    h["dead_end"] = (Wfst(3, 1, [0, 0, 0], [1, 2, 1], [1, 2, 3], [1, 1, 1], LN([0.25, 0.5, 0.25])), 4)
    # a group of one symbol beside a group of three arcs, and an epsilon group (epsilon input: the first group of state 0)
    h["groups"] = (Wfst(3, 2, [0, 0, 0, 0, 0, 1, 1], [1, 1, 2, 1, 2, 2, 2], [2, 1, 1, 1, 0, 0, 3], [1, 1, 2, 3, 1, 2, 0],
                        LN([0.1, 0.2, 0.3, 0.15, 0.25, 0.5, 0.5])), 4)
    # weights 800 apart in one list: exp(-800) underflows to 0 and the arc is never chosen
    h["underflow"] = (Wfst(3, 2, [0, 0, 0, 1], [2, 1, 2, 2], [1, 1, 1, 2], [1, 2, 3, 1], [-800.0, -1.0, 0.0, -0.5]), 4)
    # an epsilon cycle of the input side (0 -> 1 -> 0 on *e*:x, *e*:y) beside the exit
    h["epsilon_cycle"] = (Wfst(3, 2, [0, 0, 1, 1], [1, 2, 0, 2], [0, 1, 0, 2], [1, 3, 2, 3], LN([0.5, 0.5, 0.7, 0.3])), 6)
    # a cycle of *e*:*e* arcs, which every pair entry point refuses
    h["cycle_00"] = (Wfst(3, 2, [0, 0, 1, 1], [1, 2, 0, 2], [0, 1, 0, 2], [0, 1, 0, 2], LN([0.4, 0.6, 0.5, 0.5])), 6)
    # a path of exactly L = 4 arcs (0 1 2 3 4) beside one of L + 1 (0 1 2 3 5 4), which is never accepted
    h["exactly_L"] = (Wfst(6, 4, [0, 1, 2, 3, 3, 5], [1, 2, 3, 4, 5, 4], [1, 1, 2, 2, 3, 3], [1, 2, 1, 2, 1, 2],
                           LN([1.0, 1.0, 1.0, 0.5, 0.5, 1.0])), 4)
    return h


HAND = _hand()
# the final state cannot be reached: every path fails (CARMEL_HIP_ERR_STATE); not part of the equality workload
UNREACHABLE = Wfst(3, 2, [0, 1], [1, 0], [1, 2], [1, 2], LN([1.0, 1.0]))


@functools.lru_cache(maxsize=None)
def random_case(seed):
    """-> (Wfst, L): |Q| in 2 .. 8, at most 40 arcs, some with an epsilon self-loop, one arc in ten of weight zero"""
    rng = np.random.default_rng(9000 + seed)
    Q = int(rng.integers(2, 9))
    w = random_machine(rng, Q, int(rng.integers(2, 4)), int(rng.integers(Q, 41 - Q)), p_eps=0.2, cyclic=seed % 4 == 3, p_zero=0.1)
    assert w.n_states <= 8 and w.n_arcs <= 40
    return w, int(rng.integers(3, 13))


def names():
    return list(HAND) + ["random%d" % s for s in RANDOM_SEEDS]


def machine(name):
    """-> (Wfst, L, side): the random machines of odd seed are seen from the output side"""
    if name in HAND:
        return HAND[name] + (0,)
    seed = int(name[len("random"):])
    return random_case(seed) + (seed % 2,)


@functools.lru_cache(maxsize=None)
def model(name):
    w, _, side = machine(name)
    return Machine(w.n_states, w.final, w.src, w.dst, w.osym if side else w.isym, w.logw)


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    """-> (paths, tries, draws, ambiguous draws) of the equality workload, or None if a path of it fails (the machine is then
    left out of the workload: its final state is out of reach for some path within TRIES attempts of L arcs)"""
    _, L, _ = machine(name)
    paths, tries, draws, n_amb = generate(model(name), mode, N_PATHS, SEED, L, TRIES)
    return None if any(p is None for p in paths) else (paths, tries, draws, n_amb)


def workload():
    """-> [(name, mode)] with a reference"""
    return [(n, mode) for n in names() for mode in MODES if reference(n, mode) is not None]


@functools.lru_cache(maxsize=None)
def exact(name, mode):
    """-> (L, {path: probability among the accepted}, P(accept)) with 2 .. 64 accepted paths and P(accept) >= 0.3 (so that TRIES
    attempts all fail with probability 0.7^64 < 1e-9 a path), or None"""
    L = machine(name)[1] if name in HAND else L_FREQ
    every = enumerate_paths(model(name), mode, L)
    if every is None or not 2 <= len(every[0]) <= 64 or every[1] < 0.3:
        return None
    return (L,) + every


def frequency_cases():
    return [(n, mode) for n in names() for mode in MODES if exact(n, mode) is not None]
