"""What the pair arc posterior tests share (test_decode_pairs_posterior_host.py proves it on the CPU,
test_decode_pairs_posterior_gpu.py compares the device with it): on the random workload of the pair tests
(decode_pairs_cases.case, unchanged), per seed without a 00 cycle the counts of decode_pairs_posterior_ref.py, per pair and
summed, without pair weights and with the weights of pair_weights().  Computed once."""
import functools

import numpy as np

from decode_pairs_cases import SEEDS, case  # noqa: F401
from decode_pairs_posterior_ref import pair_posterior


def pair_weights(seed, n):
    """a weight per pair: fractions, whole numbers and, for every fourth pair or so, 0"""
    rng = np.random.default_rng(91000 + seed)
    w = np.round(rng.uniform(0.0, 3.0, n), 3)
    w[rng.random(n) < 0.25] = 0.0
    return w


def per_pair_in(seed, dtype):
    """-> (sums [n_pairs], counts [n_pairs, n_arcs]) of case(seed) in `dtype`: every pair's own counts; None if the 00 arcs have
    a cycle"""
    c = case(seed)
    if c["P"] is None:
        return None
    got = [pair_posterior(c["P"], x, y, dtype) for x, y in c["pairs"]]
    return np.array([z for z, _ in got], dtype), np.array([k for _, k in got], dtype)


@functools.lru_cache(maxsize=None)
def per_pair(seed):
    return per_pair_in(seed, np.float64)


def summed(sums, counts, weights):
    """the counts of a batch from its pairs' own: pairs in order, a pair without a derivation left out"""
    total = np.zeros(counts.shape[1], counts.dtype)
    for l in np.flatnonzero(sums > -np.inf):
        total += counts[l] if weights is None else counts.dtype.type(weights[l]) * counts[l]
    return total


@functools.lru_cache(maxsize=None)
def reference(seed, weighted=False):
    """-> (pair weights or None, sums, counts [n_arcs]) in f64; None if the 00 arcs have a cycle"""
    if per_pair(seed) is None:
        return None
    sums, counts = per_pair(seed)
    wt = pair_weights(seed, len(sums)) if weighted else None
    return wt, sums, summed(sums, counts, wt)
