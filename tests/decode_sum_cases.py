"""The random workload of the all-paths sum tests (test_decode_sum_host.py proves what it contains, test_decode_sum_gpu.py runs
it): per seed one random machine and, per side, its lines with the numpy forward's sums and the exact derivation counts of
decode_sum_ref.py, computed once and shared."""
import functools

import numpy as np

from decode_sum_ref import CycleError, count, forward, prepare
from test_decode_gpu import lines_for, random_machine

SEEDS = range(100)


@functools.lru_cache(maxsize=None)
def case(seed):
    """-> {"w", "lds_off", "sides": [(side, lines, ref sums or None if the epsilon arcs have a cycle, counts, epsilon levels)]}"""
    rng = np.random.default_rng(5000 + seed)
    Q = int(rng.integers(2, 60)) if seed % 10 else int(rng.integers(4100, 4400))  # every tenth: beyond the LDS tier
    V = int(rng.integers(2, 6))
    w = random_machine(rng, Q, V, int(rng.integers(Q, 4 * Q + 20)), p_eps=0.2, cyclic=seed % 7 == 3)
    sides = []
    for side in (0, 1):
        lines = lines_for(rng, w, side, V, 24 if Q < 4096 else 6)
        msym = (w.osym if side else w.isym).astype(np.int64)
        try:
            prep = prepare(w.n_states, w.src, w.dst, msym, w.logw)
        except CycleError:
            sides.append((side, lines, None, None, 0))
            continue
        ref = np.array([forward(w.n_states, w.final, w.src, w.dst, msym, w.logw, l, prep) for l in lines])
        counts = [count(w.n_states, w.final, w.src, w.dst, msym, w.logw, l, prep) for l in lines]
        sides.append((side, lines, ref, counts, len(prep[4])))
    return {"w": w, "lds_off": seed % 10 == 5, "sides": sides}


def cross_checked(c):
    """per acyclic side of a case, the indices of the lines the k-best cross-check takes: 1 .. 1024 derivations"""
    return [(side, lines, ref, counts, [l for l, n in enumerate(counts) if 1 <= n <= 1024])
            for side, lines, ref, counts, _ in c["sides"] if ref is not None]
