"""A Python restatement of k-best decoding (carmel -b -k n) for the k-best tests, independent of
csrc/decode_kbest.hip: a dynamic programme over the trellis nodes (position i, state q) in a topological order that carries
WHOLE paths, no back-pointers.  Every node keeps its best K + 1 entries (value, arc tuple); the extra one shows whether the
K-th place is tied.

A derivation runs from state 0 to the final state, its matched-side symbols without epsilons spell the line, and it uses no arc of
weight zero.  Its value is its arcs' weights added in path order from the start in f64.  Candidates at a node are (arc a into it,
rank r in the source node's list), ordered by value descending, matched arcs before epsilon arcs, arc id ascending, r ascending."""
import numpy as np

from decode_ref import CycleError

NINF = -np.inf


def eps_order(n_states, src, dst, eps):
    """the states in a topological order of the epsilon arcs `eps` (Kahn); CycleError if there is none"""
    indeg = [0] * n_states
    outs = [[] for _ in range(n_states)]
    for a in eps:
        outs[src[a]].append(a)
        indeg[dst[a]] += 1
    order = [q for q in range(n_states) if not indeg[q]]
    at = 0
    while at < len(order):
        for a in outs[order[at]]:
            indeg[dst[a]] -= 1
            if not indeg[dst[a]]:
                order.append(int(dst[a]))
        at += 1
    if len(order) < n_states:
        raise CycleError("the epsilon arcs have a cycle")
    return order


def kbest(n_states, final, src, dst, msym, logw, line, K):
    """-> (values, paths, tied): the min(K, number of derivations) best derivations of `line`, best first -- their values (path
    order sums) and arc-id tuples -- and whether two of the best K + 1 have equal values (then which paths are returned, and in
    which order, is decided by the tie rule alone)"""
    src, dst, msym = (np.asarray(a).astype(np.int64) for a in (src, dst, msym))
    logw = np.asarray(logw, np.float64)
    live = [a for a in range(len(src)) if logw[a] > NINF]
    eps_into = [[] for _ in range(n_states)]
    for a in live:
        if msym[a] == 0:
            eps_into[dst[a]].append(a)
    order = eps_order(n_states, src, dst, [a for a in live if msym[a] == 0])
    keep = K + 1

    def node(cands):
        cands.sort(key=lambda c: (-c[0], c[1], c[2], c[3]))
        return [(c[0], c[4]) for c in cands[:keep]]

    def position(prev, x):
        into = [[] for _ in range(n_states)]
        if prev is not None:
            for a in live:
                if msym[a] != 0 and msym[a] == x:
                    into[dst[a]].append(a)
        row = [None] * n_states
        for q in order:
            cands = []
            if prev is None and q == 0:
                cands.append((0.0, -1, -1, 0, ()))
            for a in into[q]:
                for r, (v, p) in enumerate(prev[src[a]]):
                    cands.append((v + logw[a], 0, a, r, p + (a,)))
            for a in eps_into[q]:
                for r, (v, p) in enumerate(row[src[a]]):
                    cands.append((v + logw[a], 1, a, r, p + (a,)))
            row[q] = node(cands)
        return row

    row = position(None, None)
    for x in line:
        row = position(row, int(x))
    ents = row[final]
    vals = [v for v, _ in ents]
    tied = len(set(vals)) < len(vals)
    return vals[:K], [p for _, p in ents[:K]], tied


def enumerate_all(n_states, final, src, dst, msym, logw, line):
    """every derivation of `line` by depth-first search -> [(value, arc tuple)] (the epsilon arcs must be acyclic)"""
    out = []
    by_src = [[] for _ in range(n_states)]
    for a in range(len(src)):
        if logw[a] > NINF:
            by_src[int(src[a])].append(a)

    def go(q, i, v, p):
        if q == final and i == len(line):
            out.append((v, p))
        for a in by_src[q]:
            if msym[a] == 0:
                go(int(dst[a]), i, v + logw[a], p + (a,))
            elif i < len(line) and msym[a] == line[i]:
                go(int(dst[a]), i + 1, v + logw[a], p + (a,))

    go(0, 0, 0.0, ())
    return out
