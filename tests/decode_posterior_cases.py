"""What the arc posterior tests share (test_decode_posterior_host.py proves it on the CPU, test_decode_posterior_gpu.py compares the
device with it): on the random workload of the sum tests (decode_sum_cases.py), per seed and acyclic side the counts of
decode_posterior_ref.py in f64, without line weights and with the weights of line_weights().  Computed once."""
import functools

import numpy as np

from decode_posterior_ref import posterior
from decode_sample_cases import msym_of
from decode_sum_cases import SEEDS, case  # noqa: F401
from decode_sum_ref import prepare


def line_weights(seed, side, n):
    """a weight per line: fractions, whole numbers and, for every fourth line or so, 0"""
    rng = np.random.default_rng(90000 + 2 * seed + side)
    w = np.round(rng.uniform(0.0, 3.0, n), 3)
    w[rng.random(n) < 0.25] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def prepared(seed, side):
    w = case(seed)["w"]
    return prepare(w.n_states, w.src, w.dst, msym_of(w, side), w.logw)


def reference_in(seed, dtype, weighted):
    """-> [(side, lines, line weights or None, sums, counts)] for the acyclic sides of case(seed), in `dtype`"""
    w = case(seed)["w"]
    out = []
    for side, lines, ref, _, _ in case(seed)["sides"]:
        if ref is None:
            continue
        wt = line_weights(seed, side, len(lines)) if weighted else None
        sums, counts = posterior(w.n_states, w.final, w.src, w.dst, msym_of(w, side), w.logw, lines, wt, dtype, prepared(seed, side))
        out.append((side, lines, wt, sums, counts))
    return out


@functools.lru_cache(maxsize=None)
def reference(seed, weighted=False):
    return reference_in(seed, np.float64, weighted)
