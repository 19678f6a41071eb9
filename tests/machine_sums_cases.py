"""The machines of the machine-sums tests (carmel_hip_decoder_machine_sums), by name, each with its reference (machine_sums_ref.py)
computed once and shared.  test_machine_sums_host.py holds the references to an enumeration of all paths and the cases to the
properties they are named for; test_machine_sums_gpu.py holds the device to the references on every one of them.

Symbols play no part in the rule: every arc carries symbol 1.  An arc list is (src, dst, log weight); arc ids are the positions
after a stable sort by source state, the order Transducer::flatten gives."""
import functools
import math

import numpy as np

from carmel_amd.model import Wfst
from machine_sums_ref import MachineSums

NEG_INF = -np.inf
DEFAULT_WAVE_DEGREE = 32  # csrc/decode_machine_sums.hip: kWaveDegree
WAVE_SETTINGS = ["0", None, "8", "4294967295"]  # every state by a wavefront; the default; a low threshold; every state by a lane
DEGREES = [1, 2, 8, 9, 31, 32, 33, 63, 64, 65, 130]  # around every setting's threshold, the wavefront's width and twice over it
RANDOM_SEEDS = list(range(20))


def build(n_states, final, arcs):
    arcs = sorted(arcs, key=lambda a: a[0])  # (stable)
    one = np.ones(len(arcs), np.uint32)
    return Wfst(n_states, final, [a[0] for a in arcs], [a[1] for a in arcs], one, one, [a[2] for a in arcs])


def weights(seed, n, lo=-4.0, hi=-0.05):
    return np.random.default_rng(seed).uniform(lo, hi, n).tolist()


def chain(n, w):
    return build(n, n - 1, [(q, q + 1, w[q]) for q in range(n - 1)])


DIAMOND = [(0, 1, math.log(0.5)), (0, 2, math.log(0.25)), (1, 3, math.log(0.75)), (2, 3, math.log(0.125))]


def grid():
    """6 x 6 states, arcs to the right and downwards: C(10, 5) = 252 paths"""
    w = iter(weights(3, 60))
    arcs = []
    for i in range(6):
        for j in range(6):
            if j < 5:
                arcs.append((6 * i + j, 6 * i + j + 1, next(w)))
            if i < 5:
                arcs.append((6 * i + j, 6 * i + j + 6, next(w)))
    return build(36, 35, arcs)


def fan(n, seed):
    """state 0 -> n middle states -> the final state: n in-arcs forwards, n out-arcs backwards, one level of n states"""
    w = weights(seed, 2 * n)
    return build(n + 2, n + 1, [(0, 1 + i, w[i]) for i in range(n)] + [(1 + i, n + 1, w[n + i]) for i in range(n)])


def degrees():
    """a state of d in-arcs for every d of DEGREES (from the first d of 130 middle states), and, turned round, a state of d
    out-arcs: every size at which a setting of machine_sums_wave_degree changes the form, and the wavefront's 64 lanes"""
    n = max(DEGREES)
    w = iter(weights(5, 10000))
    arcs = [(0, 1 + i, next(w)) for i in range(n)]
    final = 1 + n + 2 * len(DEGREES)
    for k, d in enumerate(DEGREES):
        gather, spread = 1 + n + 2 * k, 2 + n + 2 * k
        arcs += [(1 + i, gather, next(w)) for i in range(d)]   # d in-arcs
        arcs.append((gather, spread, next(w)))
        arcs += [(spread, final, next(w)) for _ in range(d)]   # d parallel out-arcs
    return build(final + 1, final, arcs)


def layers():
    """40 layers of 3 parallel arcs: 3^40 paths, above 2^53"""
    w = iter(weights(6, 120, -2.0, -0.5))
    return build(41, 40, [(q, q + 1, next(w)) for q in range(40) for _ in range(3)])


def random_dag(seed):
    """at most 60 states in a random order of their own (state ids are not topological), at most 4 parallel arcs between two states,
    a tenth of the arcs of weight 0 (log -inf), weights up to e; the final state is any state"""
    rng = np.random.default_rng(9000 + seed)
    n = int(rng.integers(2, 61))
    order = [0] + (1 + rng.permutation(n - 1)).tolist()  # state 0 comes first: something is reachable
    arcs = []
    for i in range(n):
        for j in range(i + 1, n):
            if rng.random() < min(1.0, 3.0 / n + 0.7 * (j == i + 1)):
                for _ in range(int(rng.integers(1, 5))):
                    arcs.append((order[i], order[j], NEG_INF if rng.random() < 0.1 else float(rng.uniform(-5.0, 1.0))))
    final = order[int(rng.integers(max(1, n - 3), n))] if rng.random() < 0.9 else order[int(rng.integers(0, n))]
    return build(n, final, arcs)


HAND = {
    "chain5": lambda: chain(5, [math.log(x) for x in (0.5, 0.25, 0.9, 0.1)]),
    "diamond": lambda: build(4, 3, DIAMOND),
    "grid": grid,
    "hub": lambda: fan(200, 1),            # 200 parallel two-arc routes: the wavefront form in both directions
    "level5000": lambda: fan(5000, 2),     # one level of 5 000 states
    "degrees": degrees,
    "chain3000": lambda: chain(3000, weights(4, 2999, -0.011, -0.009)),  # deep, and its bound stays small
    "layers": layers,
    "positive": lambda: build(4, 3, [(0, 1, 1.5), (0, 2, 0.25), (1, 3, 2.0), (2, 3, -0.5), (0, 3, 3.0)]),  # weights above 1, no cycle
    # arcs of weight 0 do not exist: 3 -> 0 and 1 -> 1 would be cycles, 0 -> 3 a third path
    "neg_inf": lambda: build(4, 3, DIAMOND + [(3, 0, NEG_INF), (1, 1, NEG_INF), (0, 3, NEG_INF)]),
    "final0": lambda: build(3, 0, [(0, 1, -1.0), (1, 2, -1.0), (2, 1, -0.5)]),  # the empty path alone; a dead end with a cycle
    "single_state": lambda: build(1, 0, []),
    "unreachable_final": lambda: build(4, 3, [(0, 1, -1.0), (2, 3, -1.0), (1, 1, -0.1)]),
    "no_arcs": lambda: build(3, 2, []),
    "cycle_dead_end": lambda: build(6, 3, DIAMOND + [(1, 4, -0.5), (4, 5, -0.5), (5, 4, -0.5), (5, 5, 0.5)]),
    "cycle_unreachable": lambda: build(6, 3, DIAMOND + [(4, 5, -0.5), (5, 4, -0.5), (5, 3, -0.5), (4, 4, 0.5)]),
    # refused: the lowest state the peeling leaves is named
    "cycle_in_u": lambda: build(6, 2, [(0, 1, -1.0), (1, 4, -1.0), (4, 5, -1.0), (5, 4, -1.0), (5, 2, -1.0), (0, 3, -1.0), (3, 2, -1.0)]),
    "self_loop": lambda: build(3, 2, [(0, 1, -1.0), (1, 1, -2.0), (1, 2, -1.0)]),
    "arc_into_0": lambda: build(3, 2, [(0, 1, -1.0), (1, 0, -2.0), (1, 2, -1.0)]),
    "arc_out_of_final": lambda: build(3, 1, [(0, 1, -1.0), (1, 2, -1.0), (2, 1, -1.0)]),
    "final0_loop": lambda: build(2, 0, [(0, 1, -1.0), (1, 0, -1.0)]),
}
REFUSED = {"cycle_in_u": 2, "self_loop": 1, "arc_into_0": 0, "arc_out_of_final": 1, "final0_loop": 0}  # the state the message names
SINGLE_PATH = ["chain5", "chain3000"]


def names():
    return list(HAND) + ["random%d" % s for s in RANDOM_SEEDS]


def accepted():
    return [n for n in names() if n not in REFUSED]


@functools.lru_cache(maxsize=None)
def machine(name):
    return HAND[name]() if name in HAND else random_dag(int(name[len("random"):]))


@functools.lru_cache(maxsize=None)
def reference(name):
    """computed once, shared by every test, never written to"""
    return MachineSums(machine(name))
