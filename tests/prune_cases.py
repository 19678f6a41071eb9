"""What the pruning tests share (test_prune_host.py proves the reference on the CPU, test_prune_gpu.py compares the device with
it): the machines of best_paths_cases.py (hand-made edges -- among them a final state that is state 0, a zero-weight self-loop, an
unreachable final state, positive arcs off every cycle, the hub whose final state has 200 in-arcs, the chain of 256 states --, the
random and the dyadic machines, the medium one), three more for the edges of this rule, and the grid of parameters.  The
distances of a (machine, arc threshold) are computed once."""
import functools

import numpy as np

import best_paths_cases
from carmel_amd.model import Wfst
from best_paths_cases import LN, REFUSED, M  # noqa: F401 (REFUSED: for the tests)
from prune_ref import NO_CAP, Distances

LOG_RATIOS = (0.0, float(LN(2.0)), float(LN(10.0)), np.inf)
MIN_ARC_LOGWS = (-np.inf, float(LN(0.25)))


def max_states_grid(n_states):
    return (NO_CAP, 1, 3, n_states - 1)


def _ulp_machine(seed):
    """a chain 0 -> 1 -> ... -> 6 with weights that are no dyadic fractions, and worse detours i -> i + 2"""
    rng = np.random.default_rng(9100 + seed)
    arcs = [(i, i + 1, LN(rng.uniform(0.3, 0.9))) for i in range(6)] + [(i, i + 2, LN(rng.uniform(0.01, 0.05))) for i in range(5)]
    return M(7, 6, arcs)


def ulp_property(w):
    """-> the arcs of P* whose T(a) is below F[final]: what the exemption of P* is for"""
    d = Distances(w)
    return [a for a in d.pstar if d.T_arc[a] < d.F[w.final]]


@functools.lru_cache(maxsize=None)
def ulp():
    for seed in range(200):  # found on the CPU: the forward fold of a prefix plus the backward fold of the rest rounds differently
        w = _ulp_machine(seed)
        if ulp_property(w):
            return w
    raise AssertionError("no seed gives the property")


def _own():
    h = {}
    # the final state is state 0, and nothing else is worth keeping at a ratio of 1
    h["final_is_start"] = M(3, 0, [(0, 1, LN(0.5)), (1, 0, LN(0.5)), (1, 2, LN(0.5)), (2, 0, LN(0.25)), (0, 0, LN(0.75))])
    # a self-loop of weight one on the best path's middle state: T of the loop equals the best path's value
    h["zero_self_loop"] = M(3, 2, [(0, 1, LN(0.5)), (1, 1, 0.0), (1, 2, LN(0.5)), (0, 2, LN(0.125))])
    # states 2 and 3 have the same T(q) = -1 and ranks 2 and 3: a cap of 3 keeps state 2, by its id, and the path through it
    h["cap_tie"] = M(5, 1, [(0, 2, -0.5), (2, 1, -0.5), (0, 3, -0.5), (3, 1, -0.5), (0, 4, -1.0), (4, 1, -1.0)])
    return h


OWN = _own()


@functools.lru_cache(maxsize=None)
def dag_case(seed):
    """the dyadic random machine with its backward arcs and self-loops taken away (weight zero): acyclic, every sum exact, and
    the spine still reaches the final state"""
    w = best_paths_cases.random_case(seed, dyadic=True)
    return Wfst(w.n_states, w.final, w.src, w.dst, w.isym, w.osym, np.where(w.dst > w.src, w.logw, -np.inf))


def names():
    return best_paths_cases.names() + list(OWN) + ["ulp"]


def machine(name):
    if name == "ulp":
        return ulp()
    return OWN[name] if name in OWN else best_paths_cases.machine(name)


@functools.lru_cache(maxsize=None)
def distances(name, min_arc_logw):
    return Distances(machine(name), min_arc_logw)


def grid(name):
    """-> every (log_ratio, max_states, min_arc_logw) of the grid for this machine"""
    return [(r, n, p) for p in MIN_ARC_LOGWS for n in max_states_grid(machine(name).n_states) for r in LOG_RATIOS]


def reference(name, log_ratio, max_states, min_arc_logw):
    """-> (state_keep, arc_keep) as uint8 arrays"""
    return distances(name, min_arc_logw).masks(log_ratio, max_states)
