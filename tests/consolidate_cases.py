"""What the consolidation tests share (test_consolidate_host.py checks the cases and the reference on the CPU,
test_consolidate_gpu.py compares the device with the reference of consolidate_ref.py): machines that are each the smallest that
can break a pass of csrc/consolidate.hip, the grid of (mode, clamp), and the references, computed once.

A case is a Wfst; state 0 is the start, `final` a state of the machine.  Symbol 0 is epsilon where a Decoder is built."""
import functools

import numpy as np

from carmel_amd.model import Wfst
from consolidate_ref import Consolidated

LN = np.log
NEG_INF = -np.inf
GRID = (("sum", True), ("sum", False), ("max", True))
SEGMENT_SIZES = (63, 64, 65, 200, 5000)
ARC_COUNTS = (1, 63, 64, 65, 257, 10000)
WAVE_SETTINGS = (None, "1", str(2 ** 20))  # option consolidate_wave_members: unset (64), every segment of two or more by a wavefront, none
DEFAULT_WAVE_MEMBERS = 64
RANDOM_SEEDS = tuple(range(24))


def M(n_states, final, arcs):
    """arcs: (src, dst, in, out, logw), sorted by src here (stably: a state's arcs stay in the order given)"""
    arcs = sorted(arcs, key=lambda a: a[0])
    cols = list(zip(*arcs)) if arcs else [[], [], [], [], []]
    return Wfst(n_states, final, cols[0], cols[1], cols[2], cols[3], cols[4])


def _sizes():
    """state k holds one segment of SEGMENT_SIZES[k] members, every seventh arc of another key in between; the weights of a
    segment add up to about a half, so that no clamp hides a sum"""
    rng = np.random.default_rng(4100)
    arcs = []
    for k, size in enumerate(SEGMENT_SIZES):
        for i in range(size):
            arcs.append((k, k + 1, 1, 2, float(LN(rng.uniform(0.2, 1.0) / (1.2 * size)))))
            if i % 7 == 3:
                arcs.append((k, k + 1, 2, 1, float(LN(rng.uniform(0.1, 0.2) / size))))
    return M(len(SEGMENT_SIZES) + 1, len(SEGMENT_SIZES), arcs)


def _count(n):
    """n arcs over a few states, two arcs in three duplicates; at 10 000 one segment of 3 000 members, spread over its state"""
    rng = np.random.default_rng(4200 + n)
    Q = max(2, min(40, n // 8))
    arcs = []
    for i in range(n):
        q = int(rng.integers(0, Q))
        arcs.append((q, int(rng.integers(0, Q)), int(rng.integers(0, 3)), int(rng.integers(0, 3)), float(LN(rng.uniform(1e-4, 2e-4)))))
    if n == 10000:
        for i in rng.choice(n, 3000, replace=False):
            arcs[i] = (7, 9, 2, 2, arcs[i][4])
    return M(Q, Q - 1, arcs)


def random_case(seed):
    """1-12 states, 0-200 arcs, symbols 0-3, a tenth of the weights -inf, one arc in three a copy of an earlier arc of the same
    state with a fresh weight"""
    rng = np.random.default_rng(4300 + seed)
    Q = int(rng.integers(1, 13))
    n = int(rng.integers(0, 201))
    by_state = [[] for _ in range(Q)]
    for _ in range(n):
        q = int(rng.integers(0, Q))
        w = NEG_INF if rng.random() < 0.1 else float(LN(rng.uniform(0.02, 0.3)))
        if by_state[q] and rng.random() < 1.0 / 3.0:
            old = by_state[q][int(rng.integers(0, len(by_state[q])))]
            by_state[q].append(old[:4] + (w,))
        else:
            by_state[q].append((q, int(rng.integers(0, Q)), int(rng.integers(0, 4)), int(rng.integers(0, 4)), w))
    return M(Q, int(rng.integers(0, Q)), [a for st in by_state for a in st])


def _hand():
    h = {}
    h["no_arcs"] = M(1, 0, [])
    h["one_arc"] = M(2, 1, [(0, 1, 1, 2, LN(0.5))])
    h["all_neg_inf"] = M(2, 1, [(0, 1, 1, 1, NEG_INF), (0, 1, 1, 1, NEG_INF), (1, 1, 2, 1, NEG_INF)])
    h["three_self_loops"] = M(1, 0, [(0, 0, 1, 1, LN(0.2)), (0, 0, 1, 1, LN(0.3)), (0, 0, 1, 1, LN(0.1))])
    # the first member of the segment does not exist: the representative is arc 1
    h["dead_first_member"] = M(2, 1, [(0, 1, 1, 1, NEG_INF), (0, 1, 1, 1, LN(0.25)), (0, 1, 2, 1, LN(0.5)), (0, 1, 1, 1, LN(0.125))])
    # duplicates that are not neighbours in arc order
    h["interleaved"] = M(2, 1, [(0, 1, 1, 1, LN(0.1)), (0, 1, 2, 2, LN(0.2)), (0, 1, 1, 1, LN(0.05)), (0, 1, 2, 2, LN(0.025)),
                                (0, 1, 1, 1, LN(0.3))])
    # four pairs that agree on three fields and differ in one alone (src, dst, in, out in turn): nothing merges
    h["one_field_apart"] = M(7, 6, [(0, 5, 2, 2, LN(0.5)), (1, 5, 2, 2, LN(0.25)), (2, 5, 3, 3, LN(0.5)), (2, 6, 3, 3, LN(0.25)),
                                    (3, 5, 4, 4, LN(0.5)), (3, 5, 5, 4, LN(0.25)), (4, 5, 6, 6, LN(0.5)), (4, 5, 6, 7, LN(0.25))])
    # symbols that a key of fewer than 32 bits a field would confuse with 5, each twice
    big, top = 0x80000005, 0xFFFFFFFE
    syms = [(5, 5), (big, 5), (5, big), (top, 5), (5, top), (top, top), (big, big)]
    h["wide_symbols"] = M(2, 1, [(0, 1, i, o, LN(0.03 * (k + 1))) for k, (i, o) in enumerate(syms)] +
                          [(0, 1, i, o, LN(0.01 * (k + 1))) for k, (i, o) in enumerate(syms)])
    # a destination of 70 000 beside 70 000 mod 2^16 = 4 464, in a machine of 70 001 states and a dozen arcs
    far = 70000
    h["far_state"] = M(far + 1, far, [(0, far, 1, 1, LN(0.1)), (0, far & 0xFFFF, 1, 1, LN(0.2)), (0, far, 1, 1, LN(0.05)),
                                      (0, far & 0xFFFF, 1, 1, LN(0.025)), (0, far, 1, 1, LN(0.0125)), (4464, far, 1, 1, LN(0.5)),
                                      (4464, far, 1, 1, LN(0.25)), (69999, far, 1, 1, LN(0.5)), (69999, 4464, 1, 1, LN(0.5)),
                                      (69999, far, 1, 1, LN(0.125)), (far, far, 1, 1, LN(0.5)), (far, 0, 1, 1, LN(0.25))])
    # sums below 1, exactly 1 and above 1, a lone arc above 1 (which no clamp touches), and a pair whose larger member is above 1
    h["clamp"] = M(6, 5, [(0, 1, 1, 1, LN(0.25)), (0, 1, 1, 1, LN(0.25)), (1, 2, 1, 1, LN(0.5)), (1, 2, 1, 1, LN(0.5)),
                          (2, 3, 1, 1, LN(0.75)), (2, 3, 1, 1, LN(0.75)), (3, 4, 1, 1, LN(2.0)), (4, 5, 1, 1, LN(3.0)), (4, 5, 1, 1, LN(0.5))])
    # two hops of two parallel arcs each: four paths of the same states and symbols
    h["parallel_paths"] = M(3, 2, [(0, 1, 1, 1, LN(0.5)), (0, 1, 1, 1, LN(0.25)), (0, 1, 2, 1, LN(0.125)), (1, 2, 1, 2, LN(0.5)),
                                   (1, 2, 1, 2, LN(0.0625))])
    return h


HAND = _hand()


def names():
    return list(HAND) + ["sizes"] + ["count%d" % n for n in ARC_COUNTS] + ["random%d" % s for s in RANDOM_SEEDS]


@functools.lru_cache(maxsize=None)
def machine(name):
    if name in HAND:
        return HAND[name]
    if name == "sizes":
        return _sizes()
    if name.startswith("count"):
        return _count(int(name[5:]))
    return random_case(int(name[6:]))


@functools.lru_cache(maxsize=None)
def reference(name, mode, clamp):
    w = machine(name)
    return Consolidated(w.src, w.dst, w.isym, w.osym, w.logw, mode, clamp)


DECODER_SEEDS = (0, 1, 5)  # random machines of 71, 188 and 178 arcs


@functools.lru_cache(maxsize=None)
def decoder_case(seed):
    """-> (Wfst, lines) for a Decoder on side 0.  Of the 24 random machines only two have a side without an epsilon cycle and a
    path out of state 0, so a machine is made fit the way prune_cases.dag_case does it: the arcs with input symbol 0 (epsilon on
    side 0) that do not lead to a higher state get weight zero, which leaves the input epsilons acyclic and every other arc, the
    duplicates among them, alone.  The final state is the state that random walks from state 0 reach with the most distinct input
    strings; the lines are up to 40 of those strings, each with a derivation by construction, and two without."""
    r = random_case(seed)
    logw = np.where((r.isym == 0) & (r.dst <= r.src), NEG_INF, r.logw)
    by = {}
    for a in np.flatnonzero(logw > NEG_INF):
        by.setdefault(int(r.src[a]), []).append(int(a))
    rng = np.random.default_rng(4400 + seed)
    ends = {}
    for _ in range(400):
        q, line = 0, []
        for _ in range(6):
            if q not in by:
                break
            a = by[q][int(rng.integers(0, len(by[q])))]
            if r.isym[a]:
                line.append(int(r.isym[a]))
            q = int(r.dst[a])
            ends.setdefault(q, set()).add(tuple(line))
    final = max(sorted(ends), key=lambda q: len(ends[q]))
    w = Wfst(r.n_states, final, r.src, r.dst, r.isym, r.osym, logw)
    assert epsilon_acyclic_side(w) == 0
    return w, [list(l) for l in sorted(ends[final])[:40]] + [[3] * 9, [1, 2, 3] * 4]


def epsilon_acyclic_side(w):
    """-> 0 or 1: a side on which the existing arcs with symbol 0 form no cycle (what Decoder.sum needs), or None"""
    for side in (0, 1):
        sym = w.isym if side == 0 else w.osym
        eps = [(int(s), int(d)) for s, d, x, lw in zip(w.src, w.dst, sym, w.logw) if x == 0 and lw > NEG_INF]
        left = set(range(w.n_states))
        while True:  # peel the states without an epsilon arc coming in from what is left
            entered = {d for s, d in eps if s in left and d in left}
            peeled = left - entered
            if not peeled:
                break
            left -= peeled
        if not left:
            return side
    return None
