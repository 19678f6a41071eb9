"""The inputs of the k-best GPU test (test_decode_kbest_gpu.py) and their reference results, computed once a process with
decode_kbest_ref.py alone.  test_decode_kbest_host.py checks on the CPU that these inputs exercise the k lists: enough lines with
several derivations, few lines whose K + 1 best values tie."""
import functools

import numpy as np

from decode_kbest_ref import kbest
from test_decode_gpu import lines_for, random_machine

KS = (1, 2, 3, 5, 8, 64)
# seed s runs with K = KS[s % 6].  The seeds were picked with the reference alone so that few lines are tied (with many
# derivations of a short line over a small machine, permuted sums of the same arcs tie often, mostly at K = 8 and 64):
# per K the first seeds with at least five lines that have a derivation and at most a tenth of them tied; for K = 64, where
# those have few full lists, 11 and 47 (many full lists, half of them tied) replace two of them.
SEEDS = (0, 24, 30, 36, 42, 60, 78, 1, 19, 31, 49, 55, 85, 91, 74, 80, 92, 104, 122, 158, 170, 9, 21, 39, 51, 87, 93, 99,
         10, 40, 46, 70, 88, 112, 130, 59, 107, 173, 179, 293, 11, 47)
BIG = "big"  # |Q| K = 70 x 64 > 4096: the global tier, chosen by size
TIER_SEEDS = (0, 1, 80, 99, 46, 47)  # one seed per K: run again with decode_lds=0, and chunked


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(w, K, sides=[(side, lines, [(values, paths, tied) per line])])"""
    if name == BIG:
        rng = np.random.default_rng(7000)
        Q, V, K = 70, 4, 64
    else:
        rng = np.random.default_rng(5000 + name)
        Q, V, K = int(rng.integers(2, 41)), int(rng.integers(2, 7)), KS[name % len(KS)]
    w = random_machine(rng, Q, V, int(rng.integers(Q, 4 * Q + 20)), p_eps=0.2, cyclic=False)
    sides = []
    for side in (0, 1):
        lines = lines_for(rng, w, side, V, 10)
        msym = (w.osym if side else w.isym).astype(np.int64)
        ref = [kbest(w.n_states, w.final, w.src, w.dst, msym, w.logw, line, K) for line in lines]
        sides.append((side, lines, msym, ref))
    return dict(w=w, K=K, sides=sides)


def all_cases():
    return list(SEEDS) + [BIG]
