"""A Python restatement of batch generation (carmel_hip_decoder_generate, Decoder.generate; carmel -G / -g) for the generation
tests, written from the arc arrays with lists of its own, not from the device's tables, and an exact enumerator beside it.

The rule (include/carmel_hip.h and DESIGN.md state it in the same words).
Arcs.  Only arcs of weight > 0 (log weight > -inf) exist for generation.
Lists.  JOINT mode has one list per state: its arcs by arc id.  CONDITIONAL mode has one list per (state, matched-side symbol):
that group's arcs by arc id; a state's groups are in ascending symbol id, epsilon (0) first.
Cumulative values of a list w_0 .. w_{m-1}.  M = max w_k, p_k = exp(w_k - M) by math.exp (the host libm, as the builder uses),
cum_k = cum_{k-1} + p_k in f64, in list order, S = cum_{m-1}.
Choice with a uniform u.  t = u S, one f64 multiply; the arc is the first k with cum_k > t; if there is none, because t rounded
up to S, the first k with cum_k == S.  An arc whose p_k underflowed to 0 is therefore never chosen.
Attempt a = 0, 1, ... of path P.  Start with s = 0, n = 0 and repeat: 1. if s is the final state, accept; 2. if n == max_arcs, or
s has no list, reject; 3. JOINT: u = uniform(seed, a, P, n), chosen in s's list; CONDITIONAL: G the number of s's groups,
g = min(G - 1, floor(uniform(seed, a, P, 2n) G)), the arc chosen in group g with uniform(seed, a, P, 2n + 1); 4. append the arc,
set s to its destination, increment n.  A rejected attempt is followed by a + 1; after max_tries rejected attempts the path has
failed.
Reported weight.  The path's arcs' logs added from the END, w1 + (w2 + (... + (wn + 0))); the empty path has 0.0.

A draw is AMBIGUOUS if some cum_k other than the last lies within 1e-9 S of t: there a builder whose exp differs from this
one's in the last bit may choose the neighbouring arc.  The margin is derived, not measured: two exps each good to an ulp differ
by <= 2.2e-16 relative; a list of <= 1e4 arcs accumulates <= 2.2e-12 S; 1e-9 leaves two orders over that."""
import bisect
import math

from decode_sample_ref import uniform

NINF = -math.inf
AMBIGUITY = 1e-9
JOINT, CONDITIONAL = "joint", "conditional"


class Machine(object):
    """a machine seen from one side: msym the matched side's symbols (0 = epsilon); per state its lists, for both modes"""

    def __init__(self, n_states, final, src, dst, msym, logw):
        self.Q, self.final = int(n_states), int(final)
        self.src = [int(x) for x in src]
        self.dst = [int(x) for x in dst]
        self.msym = [int(x) for x in msym]
        self.logw = [float(x) for x in logw]
        by_state = [{} for _ in range(self.Q)]
        for k in range(len(self.src)):  # (ascending k: every list is in arc-id order)
            if self.logw[k] > NINF:
                by_state[self.src[k]].setdefault(self.msym[k], []).append(k)
        # groups[mode][s] = [(arc ids, cum)] in the state's group order; no entry without arcs
        self.groups = {JOINT: [], CONDITIONAL: []}
        for s in range(self.Q):
            every = sorted(k for arcs in by_state[s].values() for k in arcs)
            self.groups[JOINT].append([self._list(every)] if every else [])
            self.groups[CONDITIONAL].append([self._list(by_state[s][x]) for x in sorted(by_state[s])])

    def _list(self, arcs):
        M = max(self.logw[k] for k in arcs)
        cum, run = [], 0.0
        for k in arcs:
            run += math.exp(self.logw[k] - M)
            cum.append(run)
        return arcs, cum


def choose(cum, u):
    """-> (index in the list, the draw is ambiguous)"""
    S = cum[-1]
    t = u * S
    k = bisect.bisect_right(cum, t)  # the first cum_k > t
    if k == len(cum):
        k = bisect.bisect_left(cum, S)  # t rounded up to S: the first cum_k == S
    lo = bisect.bisect_left(cum, t - AMBIGUITY * S)
    hi = bisect.bisect_right(cum, t + AMBIGUITY * S)
    amb = any(abs(cum[j] - t) <= AMBIGUITY * S for j in range(lo, min(hi, len(cum) - 1)))
    return k, amb


def attempt(m, mode, seed, a, P, max_arcs):
    """-> (accepted, arc ids, draws, ambiguous draws) of attempt a of path P"""
    s, path, draws, n_amb = 0, [], 0, 0
    while True:
        if s == m.final:
            return True, path, draws, n_amb
        groups = m.groups[mode][s]
        n = len(path)
        if n == max_arcs or not groups:
            return False, path, draws, n_amb
        if mode == JOINT:
            arcs, cum = groups[0]
            u = uniform(seed, a, P, n)
        else:
            G = len(groups)
            arcs, cum = groups[min(G - 1, int(uniform(seed, a, P, 2 * n) * G))]
            u = uniform(seed, a, P, 2 * n + 1)
        k, amb = choose(cum, u)
        draws += 1
        n_amb += amb
        path.append(arcs[k])
        s = m.dst[arcs[k]]


def generate_path(m, mode, seed, P, max_arcs, max_tries):
    """-> (arc ids or None if the path failed, attempts used, draws, ambiguous draws)"""
    draws = n_amb = 0
    for a in range(max_tries):
        ok, path, d, na = attempt(m, mode, seed, a, P, max_arcs)
        draws += d
        n_amb += na
        if ok:
            return path, a + 1, draws, n_amb
    return None, max_tries, draws, n_amb


def generate(m, mode, n, seed, max_arcs, max_tries, first=0):
    """-> (paths [n] (None: failed), tries [n], draws, ambiguous draws)"""
    paths, tries, draws, n_amb = [], [], 0, 0
    for p in range(n):
        path, t, d, na = generate_path(m, mode, seed, first + p, max_arcs, max_tries)
        paths.append(path)
        tries.append(t)
        draws += d
        n_amb += na
    return paths, tries, draws, n_amb


def reported_weight(m, path):
    w = 0.0
    for k in reversed(path):
        w = m.logw[k] + w
    return w


def path_order_weight(m, path):
    w = 0.0
    for k in path:
        w += m.logw[k]
    return w


def is_walk(m, path, max_arcs):
    """starts in state 0, reaches the final state with its last arc and not before, uses no arc of weight zero, <= max_arcs arcs"""
    s = 0
    for k in path:
        if s == m.final or m.src[k] != s or not m.logw[k] > NINF:
            return False
        s = m.dst[k]
    return s == m.final and len(path) <= max_arcs


def enumerate_paths(m, mode, max_arcs, limit=200000):
    """-> ({path tuple: probability among the accepted walks}, P(accept)), or None if more than `limit` walks would be visited.
    Every walk from state 0 of <= max_arcs arcs that ends the first time it reaches the final state, with the product of its local
    probabilities: 1 / G for the group (conditional mode) times p_k / S for the arc, p_k and S as the lists have them."""
    found = {}
    visited = [0]

    def go(s, path, p):
        visited[0] += 1
        if visited[0] > limit:
            raise OverflowError
        if s == m.final:
            found[tuple(path)] = p
            return
        groups = m.groups[mode][s]
        if len(path) == max_arcs or not groups:
            return
        for arcs, cum in groups:
            prev = 0.0
            for k, c in zip(arcs, cum):
                pk = c - prev  # (the share of [0, S) in which the rule chooses k: p_k up to the sums' rounding, 0 if it underflowed)
                prev = c
                if pk > 0.0:
                    path.append(k)
                    go(m.dst[k], path, p * (pk / cum[-1]) / len(groups))
                    path.pop()

    try:
        go(0, [], 1.0)
    except OverflowError:
        return None
    accept = math.fsum(found.values())
    return {path: p / accept for path, p in found.items()}, accept


def frequencies(paths):
    """-> {path tuple: share of the paths}"""
    out = {}
    for p in paths:
        out[tuple(p)] = out.get(tuple(p), 0) + 1
    return {p: c / float(len(paths)) for p, c in out.items()}
