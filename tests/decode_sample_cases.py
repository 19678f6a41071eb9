"""What the sampling tests share (test_decode_sample_host.py proves it on the CPU, test_decode_sample_gpu.py compares the device
with it): on the random workload of the sum tests (decode_sum_cases.py), per seed and acyclic side the reference's samples of
decode_sample_ref.py, and for the frequency tests the lines with 2 .. 64 derivations with their exact posteriors.  Computed once."""
import functools
import math

import numpy as np

from decode_sample_ref import Model, enumerate_derivations, sample
from decode_sum_cases import SEEDS, case  # noqa: F401

N_RANDOM, SEED_RANDOM = 8, 12345
N_FREQ, SEED_FREQ = 4000, 777
FREQ_SEEDS = [s for s in SEEDS if s % 5 == 1]
SIGMAS = 5.0


def msym_of(w, side):
    return (w.osym if side else w.isym).astype(np.int64)


@functools.lru_cache(maxsize=None)
def model(seed, side):
    w = case(seed)["w"]
    return Model(w.n_states, w.final, w.src, w.dst, msym_of(w, side), w.logw)


@functools.lru_cache(maxsize=None)
def reference(seed):
    """-> [(side, lines, model, per line None or (mat, ambiguous))] for the acyclic sides of case(seed): N = 8, seed 12345"""
    out = []
    for side, lines, ref, _, _ in case(seed)["sides"]:
        if ref is not None:
            m = model(seed, side)
            out.append((side, lines, m, sample(m, lines, N_RANDOM, SEED_RANDOM)))
    return out


@functools.lru_cache(maxsize=None)
def posterior(seed):
    """-> [(side, lines, {line index: {path tuple: exact posterior probability}})] over the lines with 2 .. 64 derivations of the
    acyclic sides of case(seed): p = exp(w - Z), w the derivation's arcs added in path order, Z the reference's forward value"""
    out = []
    for side, lines, ref, counts, _ in case(seed)["sides"]:
        if ref is None:
            continue
        m = model(seed, side)
        post = {}
        for l, c in enumerate(counts):
            if 2 <= c <= 64:
                every = enumerate_derivations(m, lines[l])
                assert len(every) == c, (seed, side, l, len(every), c)
                post[l] = {tuple(p): math.exp(w - ref[l]) for p, w in every}
        out.append((side, lines, post))
    return out


def check_frequencies(freq, post, n, where):
    """every derivation's empirical share f against its posterior p: |f - p| <= 5 (sqrt(p (1 - p) / n) + 1 / n); -> the worst
    ratio of |f - p| to that bound's unit.  A sampled path that is no derivation fails."""
    assert set(freq) <= set(post), (where, sorted(set(freq) - set(post)))
    worst = 0.0
    for path, p in post.items():
        f = freq.get(path, 0.0)
        unit = math.sqrt(p * (1.0 - p) / n) + 1.0 / n
        worst = max(worst, abs(f - p) / unit)
        assert abs(f - p) <= SIGMAS * unit, (where, path, f, p, abs(f - p) / unit)
    return worst
