"""What the best-paths tests share (test_best_paths_host.py proves the reference on the CPU, test_best_paths_gpu.py compares the
device with it): hand-made machines for the edges of the rule, the random machines of test_decode_gpu.random_machine (|Q| 2 .. 8,
at most 40 arcs), the same with dyadic weights, and one medium machine.  References are computed once."""
import functools

import numpy as np

from carmel_amd.model import Wfst
from best_paths_ref import best_paths
from test_decode_gpu import random_machine

KS = (1, 2, 5, 16)
RANDOM_SEEDS = range(40)
LN = np.log
ZERO = -np.inf


def M(n_states, final, arcs):
    """arcs: (src, dst, log weight), sorted by source here (stable); symbols play no part"""
    arcs = sorted(arcs, key=lambda a: a[0])
    one = np.ones(len(arcs), np.uint32)
    return Wfst(n_states, final, [a[0] for a in arcs], [a[1] for a in arcs], one, one, [float(a[2]) for a in arcs])


def _hub():
    # 200 states 1 .. 200, each entered from state 0 and entering the final state 201; equal and unequal weights mixed
    arcs = [(0, 1 + i, -0.125 * (i % 7)) for i in range(200)] + [(1 + i, 201, -0.25 * (i % 5) - (0.1 if i % 3 == 0 else 0.0))
                                                                  for i in range(200)]
    return M(202, 201, arcs)


def _hand():
    h = {}
    # the start state is final: the empty path first, then the cycles back to it
    h["start_is_final"] = M(2, 0, [(0, 0, LN(0.5)), (0, 1, LN(0.25)), (1, 0, LN(0.5)), (0, 0, LN(0.125))])
    # a zero-weight self-loop (arc 1) of lower arc id than the arc entering its state (arc 3): without the length key rank 0 of
    # state 1 would be (loop, rank 0), pointing at itself
    h["self_loop_trap"] = M(4, 3, [(0, 2, LN(0.5)), (1, 1, 0.0), (1, 3, LN(0.5)), (2, 1, LN(0.5))])
    # a two-state cycle of weight zero
    h["zero_cycle"] = M(2, 1, [(0, 1, 0.0), (1, 0, 0.0)])
    # parallel arcs of equal weight
    h["parallel"] = M(3, 2, [(0, 1, LN(0.5)), (0, 1, LN(0.5)), (0, 1, LN(0.5)), (1, 2, LN(0.25)), (1, 2, LN(0.25))])
    # a final state with out-arcs that return to it
    h["final_returns"] = M(3, 1, [(0, 1, LN(0.5)), (1, 2, LN(0.5)), (2, 1, LN(0.75)), (1, 1, LN(0.25))])
    # arcs that do not exist, first and last in a state's in-list
    h["zero_first_and_last"] = M(3, 2, [(0, 2, ZERO), (0, 1, LN(0.5)), (0, 2, LN(0.3)), (1, 2, LN(0.9)), (1, 2, ZERO)])
    # a DAG with 3 paths: K = 16 returns 3
    h["dag3"] = M(4, 3, [(0, 1, LN(0.5)), (0, 2, LN(0.4)), (1, 3, LN(0.5)), (2, 3, LN(0.5)), (0, 3, LN(0.1))])
    # the final state cannot be reached: success with no paths
    h["unreachable"] = M(3, 2, [(0, 1, LN(0.5)), (1, 0, LN(0.5)), (2, 2, LN(0.5))])
    # an arc of weight above 1 off every cycle is legal (the cycle 1 -> 1 beside it has weight below 1)
    h["positive_off_cycle"] = M(3, 2, [(0, 1, LN(3.0)), (1, 1, LN(0.5)), (1, 2, LN(2.0)), (0, 2, LN(1.5))])
    h["hub"] = _hub()
    h["chain"] = M(256, 255, [(i, i + 1, -0.5 - (i % 3)) for i in range(255)])
    return h


HAND = _hand()
# refused with CARMEL_HIP_ERR_UNSUPPORTED: (machine, the arc the message names)
REFUSED = {
    "positive_on_cycle": (M(3, 2, [(0, 1, LN(0.5)), (1, 0, LN(2.0)), (1, 2, LN(0.5))]), 1),
    "positive_self_loop": (M(2, 1, [(0, 0, LN(1.5)), (0, 1, LN(0.5))]), 0),
}


@functools.lru_cache(maxsize=None)
def random_case(seed, dyadic=False):
    """|Q| in 2 .. 8, at most 40 arcs, a quarter with cyclic=True, one arc in ten of weight zero; dyadic: log weights -m / 8,
    m in 4 .. 12, so that every sum of them is exact"""
    rng = np.random.default_rng(4200 + seed)
    Q = int(rng.integers(2, 9))
    w = random_machine(rng, Q, 3, int(rng.integers(Q, 41 - Q)), p_eps=0.2, cyclic=seed % 4 == 3, p_zero=0.1)
    assert w.n_states <= 8 and w.n_arcs <= 40
    if dyadic:
        m = rng.integers(4, 13, w.n_arcs) / 8.0
        w = Wfst(w.n_states, w.final, w.src, w.dst, w.isym, w.osym, np.where(np.isfinite(w.logw), -m, ZERO))
    return w


@functools.lru_cache(maxsize=None)
def medium():
    return random_machine(np.random.default_rng(77), 300, 3, 2988, p_eps=0.2, cyclic=True, p_zero=0.1)


def names():
    return list(HAND) + ["random%d" % s for s in RANDOM_SEEDS] + ["dyadic%d" % s for s in RANDOM_SEEDS] + ["medium"]


def machine(name):
    if name in HAND:
        return HAND[name]
    if name == "medium":
        return medium()
    return random_case(int(name[6:]), name.startswith("dyadic"))


@functools.lru_cache(maxsize=None)
def reference(name, K):
    """-> [(value, reported weight, [arc ids])]"""
    return best_paths(machine(name), K)
