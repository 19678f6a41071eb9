"""The workload of the pair k-best tests (test_decode_pairs_kbest_host.py proves the reference and what the workload contains,
test_decode_pairs_kbest_gpu.py runs it).  decode_pairs_cases' own machines are too unambiguous for k-best lists, so the machines
here are small and dense: two symbols a side, 8 to 14 arcs a state.

48 seeds, rng = default_rng(9000 + seed), V = 2, side = seed % 2, random_machine(p_eps = 0.25, acyclic).  Normally Q in [3, 7],
n_arcs in [8 Q, 14 Q + 8) and K = (1, 2, 3, 5, 8, 16)[seed % 6]; every eighth seed (seed % 8 == 7) is wider, Q in [40, 60], n_arcs
in [3 Q, 5 Q), K = 16: beyond LDS by size whenever min(n, m) >= 3.  seed % 4 == 1 adds a 0M self-loop (an insertion on the other
side: an epsilon cycle of the matched side, legal for pairs).  12 pairs a seed from decode_pairs_cases.pairs_for: the empty pair
and both unknown-symbol pairs first.  Every fifth seed has, additionally, a TIE variant: the same machine and pairs with the
weights drawn from {ln 1/2, ln 1/4}, so that derivations of equal value occur.

A case is (seed, tie).  Per case the machine, the pairs, the exact derivation counts and decode_pairs_kbest_ref's lists, computed
once and shared."""
import functools

import numpy as np

from decode_pairs_cases import add_arc, pairs_for, sides
from decode_pairs_kbest_ref import kbest
from decode_pairs_ref import Prepared, count
from test_decode_gpu import random_machine

SEEDS = range(48)
CASES = [(s, False) for s in SEEDS] + [(s, True) for s in SEEDS if s % 5 == 0]
N_PAIRS = 12
V = 2
LDS_DOUBLES = 8192  # the three diagonals of the largest pair, K doubles a state, fit 64 KiB


@functools.lru_cache(maxsize=None)
def case(seed, tie=False):
    """-> {"w", "side", "K", "loop", "wide", "pairs", "P", "count", "diag" (3 (min(n, m) + 1) |Q| K of the largest pair)}"""
    rng = np.random.default_rng(9000 + seed)
    wide = seed % 8 == 7
    side = seed % 2
    if wide:
        Q = int(rng.integers(40, 61))
        n_arcs = int(rng.integers(3 * Q, 5 * Q))
        K = 16
    else:
        Q = int(rng.integers(3, 8))
        n_arcs = int(rng.integers(8 * Q, 14 * Q + 8))
        K = (1, 2, 3, 5, 8, 16)[seed % 6]
    w = random_machine(rng, Q, V, n_arcs, p_eps=0.25, cyclic=False)
    loop = seed % 4 == 1
    if loop:  # a 0M self-loop
        q, v, lw = int(rng.integers(0, Q)), int(rng.integers(1, V + 1)), float(np.log(rng.uniform(0.1, 0.9)))
        w = add_arc(w, q, q, v if side else 0, 0 if side else v, lw)
    pairs = pairs_for(rng, w, side, V, N_PAIRS)
    if tie:  # (drawn from a generator of its own: the machine's shape and the pairs are the seed's)
        from carmel_amd.model import Wfst
        t = np.random.default_rng(19000 + seed).choice([np.log(0.5), np.log(0.25)], size=len(w.logw))
        w = Wfst(w.n_states, w.final, w.src, w.dst, w.isym, w.osym, np.where(w.logw > -np.inf, t, -np.inf))
    msym, osym = sides(w, side)
    P = Prepared(w.n_states, w.final, w.src, w.dst, msym, osym, w.logw)
    diag = max(3 * (min(len(x), len(y)) + 1) * Q * K for x, y in pairs)
    return {"w": w, "side": side, "K": K, "loop": loop, "wide": wide, "pairs": pairs, "P": P,
            "count": [count(P, x, y) for x, y in pairs], "diag": diag}


@functools.lru_cache(maxsize=None)
def reference(seed, tie=False):
    """-> per pair of case(seed, tie) the reference's (values, paths, tied) at the case's K"""
    c = case(seed, tie)
    return [kbest(c["P"], x, y, c["K"]) for x, y in c["pairs"]]
