"""What the pair sampling tests share (test_decode_pairs_sample_host.py proves it on the CPU, test_decode_pairs_sample_gpu.py
compares the device with it): on the random workload of the pair tests (decode_pairs_cases.py), per seed the reference's samples
of decode_pairs_sample_ref.py, and for the frequency tests the pairs with 2 .. 64 derivations with their exact posteriors.
Computed once."""
import functools
import math

from decode_pairs_cases import SEEDS, case  # noqa: F401
from decode_pairs_ref import enumerate_paths
from decode_pairs_sample_ref import sample
from decode_sample_cases import N_FREQ, N_RANDOM, SEED_FREQ, SEED_RANDOM, SIGMAS, check_frequencies  # noqa: F401

FREQ_SEEDS = [s for s in SEEDS if s % 5 == 1]


@functools.lru_cache(maxsize=None)
def reference(seed):
    """-> None if the 00 arcs of case(seed) have a cycle, else per pair None or (mat, ambiguous): N = 8, seed 12345"""
    c = case(seed)
    return None if c["P"] is None else sample(c["P"], c["pairs"], N_RANDOM, SEED_RANDOM)


@functools.lru_cache(maxsize=None)
def posterior(seed):
    """-> {pair index: {path tuple: exact posterior probability}} over the pairs of case(seed) with 2 .. 64 derivations:
    p = exp(w - Z), w the derivation's arcs added in path order, Z the reference's sum; the derivations by brute force"""
    c = case(seed)
    post = {}
    if c["P"] is None:
        return post
    for l, (x, y) in enumerate(c["pairs"]):
        if 2 <= c["count"][l] <= 64:
            every = enumerate_paths(c["P"], x, y)
            assert len(every) == c["count"][l], (seed, l, len(every), c["count"][l])
            post[l] = {}
            for p in every:
                w = 0.0
                for a in p:
                    w += c["P"].logw[a]
                post[l][tuple(p)] = math.exp(w - c["sum"][l])
    return post
