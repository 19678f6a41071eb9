"""The random workload of the pair decoding tests (test_decode_pairs_host.py proves the reference and what the workload contains,
test_decode_pairs_gpu.py runs it): per seed one random machine (test_decode_gpu.random_machine, p_eps = 0.3 on either side), a
side, its pairs, and decode_pairs_ref.py's sums, bests and exact derivation counts, computed once and shared.

Every seed has the pairs ([], []), (a symbol no arc carries, a known line) and (a known line, a symbol no arc carries); the other
pairs are the two strings of a random walk that stops at the final state, and in 15 % of them one symbol of y is drawn again.
Every tenth seed is beyond the LDS tier (|Q| > 4096, 6 pairs), one in ten forces the global tier on a small machine, some
machines get a 0M self-loop (an epsilon cycle of the matched side: legal for pairs), some a 00 cycle (refused)."""
import functools

import numpy as np

from decode_pairs_ref import CycleError, Prepared, count, pair_best, pair_sum
from decode_sum_ref import epsilon_levels
from test_decode_gpu import random_machine

SEEDS = range(100)
MAX_LEN = 14


def sides(w, side):
    """-> (matched symbols, other symbols) of the machine's arcs for a decoder of that side"""
    return (w.osym, w.isym) if side else (w.isym, w.osym)


def add_arc(w, src, dst, isym, osym, logw):
    from carmel_amd.model import Wfst
    at = int(np.searchsorted(w.src, src, side="right"))  # the last of its state's arcs: the arcs stay state-major
    ins = lambda a, v: np.insert(a, at, v)
    return Wfst(w.n_states, w.final, ins(w.src, src), ins(w.dst, dst), ins(w.isym, isym), ins(w.osym, osym), ins(w.logw, logw))


def walk_pair(rng, w, side, to_final):
    """the two strings of a random walk from the start that stops when it first reaches the final state; None if it got too long"""
    msym, osym = sides(w, side)
    q, x, y = 0, [], []
    for _ in range(4 * MAX_LEN):
        if q == w.final:
            return x, y
        k = np.nonzero((w.src == q) & (w.logw > -np.inf))[0]
        if not len(k):
            return None
        nearer = k[to_final[w.dst[k]] < to_final[q]]
        a = rng.choice(nearer) if len(nearer) and rng.uniform() < 0.7 else rng.choice(k)
        if msym[a]:
            x.append(int(msym[a]))
        if osym[a]:
            y.append(int(osym[a]))
        if len(x) > MAX_LEN or len(y) > MAX_LEN:
            return None
        q = int(w.dst[a])
    return None


def distance_to_final(w):
    """arcs to the final state, over the arcs of non-zero weight (unreachable: a large number)"""
    dist = np.full(w.n_states, 1 << 30, np.int64)
    dist[w.final] = 0
    ok = w.logw > -np.inf
    src, dst = w.src[ok].astype(np.int64), w.dst[ok].astype(np.int64)
    for _ in range(w.n_states):
        nd = dist.copy()
        np.minimum.at(nd, src, dist[dst] + 1)
        if (nd == dist).all():
            break
        dist = nd
    return dist


def pairs_for(rng, w, side, V, n):
    to_final = distance_to_final(w)
    known = None
    out = []
    for _ in range(40 * n):
        if len(out) >= n - 3:
            break
        p = walk_pair(rng, w, side, to_final)
        if p is None:
            continue
        x, y = p
        known = known or (p if x and y else None)
        if y and rng.uniform() < 0.15:
            y = list(y)
            y[int(rng.integers(0, len(y)))] = int(rng.integers(1, V + 1))
        out.append((x, y))
    kx, ky = known or ([1], [1])
    fixed = [([], []), ([V + 7], ky), (kx, [V + 7])]  # the empty pair; a symbol no arc carries, on either side
    return fixed + out


@functools.lru_cache(maxsize=None)
def case(seed):
    """-> {"w", "side", "lds_off", "loop", "matched_cyclic", "pairs", "P" (None: the 00 arcs have a cycle), "sum", "best",
    "count"}: best[l] = (value, path or None, tied)"""
    rng = np.random.default_rng(7000 + seed)
    big = seed % 10 == 0
    Q = int(rng.integers(4100, 4400)) if big else int(rng.integers(2, 40))  # every tenth: beyond the LDS tier
    V = int(rng.integers(2, 6))
    side = 1 if seed % 3 == 1 else 0
    n_arcs = int(rng.integers(Q, 4 * Q + 20)) if big else int(rng.integers(2 * Q, 6 * Q + 20))  # dense: several derivations a pair
    w = random_machine(rng, Q, V, n_arcs, p_eps=0.3, cyclic=seed % 7 == 3)
    loop = seed % 4 == 1
    if loop:  # a 0M self-loop: an insertion on the other side, an epsilon cycle of the matched side
        q, v, lw = int(rng.integers(0, Q)), int(rng.integers(1, V + 1)), float(np.log(rng.uniform(0.1, 0.9)))
        w = add_arc(w, q, q, v if side else 0, 0 if side else v, lw)
    msym, osym = sides(w, side)
    pairs = pairs_for(rng, w, side, V, 6 if big else 16)
    try:
        epsilon_levels(w.n_states, w.src, w.dst, np.nonzero((w.logw > -np.inf) & (msym == 0))[0])
        matched_cyclic = False
    except CycleError:
        matched_cyclic = True
    c = {"w": w, "side": side, "lds_off": seed % 10 == 5, "loop": loop, "matched_cyclic": matched_cyclic, "pairs": pairs}
    try:
        P = Prepared(w.n_states, w.final, w.src, w.dst, msym, osym, w.logw)
    except CycleError:
        c.update(P=None, sum=None, best=None, count=None)
        return c
    c.update(P=P, sum=np.array([pair_sum(P, x, y) for x, y in pairs]), best=[pair_best(P, x, y) for x, y in pairs],
             count=[count(P, x, y) for x, y in pairs])
    return c
