"""The rule of carmel_hip_decoder_best_paths (include/carmel_hip.h, csrc/decode_best_paths.hip) restated in Python and f64, with
the same additions in the same order, so that the device is held to it bit for bit; and an exhaustive enumerator of the walks of
at most L arcs, which anchors the rule itself where every sum is exact (test_best_paths_host.py).

An entry is (value, length, last arc, rank); NONE is the arc of the empty path."""
import functools

import numpy as np

NONE = 0xFFFFFFFF
NEG_INF = float("-inf")


class Machine(object):
    def __init__(self, w):
        self.n_states, self.final = w.n_states, w.final
        self.src = [int(x) for x in w.src]
        self.dst = [int(x) for x in w.dst]
        self.logw = [float(x) for x in w.logw]
        self.ins = [[] for _ in range(self.n_states)]   # per state: (src, w, arc id) of the arcs into it, in arc-id order
        self.outs = [[] for _ in range(self.n_states)]  # per state: (dst, w, arc id)
        for a, (s, t, x) in enumerate(zip(self.src, self.dst, self.logw)):
            if x > NEG_INF:  # only these arcs exist
                self.ins[t].append((s, x, a))
                self.outs[s].append((t, x, a))


def merge(m, q, lists, K):
    """-> the list of state q, computed from `lists`"""
    arcs = m.ins[q]
    heads = [0] * len(arcs)
    cand = [(lists[s][0][0] + w, lists[s][0][1] + 1) if lists[s] else None for s, w, _ in arcs]
    out, empty = [], q == 0
    while len(out) < K:
        bi, bv, bl = -1, None, None
        for i, c in enumerate(cand):  # in arc-id order: only a strictly earlier candidate replaces the one held
            if c is not None and (bi < 0 or c[0] > bv or (c[0] == bv and c[1] < bl)):
                bi, bv, bl = i, c[0], c[1]
        if empty and (bi < 0 or not bv > 0.0):  # the empty path comes before anything of equal value
            out.append((0.0, 0, NONE, 0))
            empty = False
            continue
        if bi < 0:
            break
        s, w, a = arcs[bi]
        h = heads[bi]
        out.append((bv, bl, a, h))
        heads[bi] = h = h + 1
        cand[bi] = (lists[s][h][0] + w, lists[s][h][1] + 1) if h < len(lists[s]) else None
    return out


def rounds(m, K, worklist=True):
    """-> (lists, rounds run, states recomputed): the lists of the first round that equal the previous round's.  worklist: a state
    none of whose sources' lists changed keeps its list (by definition; False recomputes every state every round)"""
    lists = [[] for _ in range(m.n_states)]
    lists[0] = [(0.0, 0, NONE, 0)]
    changed = {0}
    n_rounds = n_selected = 0
    while True:
        active = sorted({t for q in changed for t, _, _ in m.outs[q]}) if worklist else range(m.n_states)
        if worklist and not active:
            return lists, n_rounds, n_selected
        assert n_rounds <= K * m.n_states + 1, "did not converge"
        n_rounds += 1
        n_selected += len(active)
        new = {q: merge(m, q, lists, K) for q in active}
        changed = {q for q, l in new.items() if l != lists[q]}
        if not worklist and not changed:
            return lists, n_rounds, n_selected
        for q in changed:
            lists[q] = new[q]


def read_out(m, lists):
    """-> [(value, reported weight, [arc ids])] of list(final), best first; asserts that every walk back ends at the empty path
    with lengths strictly decreasing"""
    out = []
    for r, (value, length, _, _) in enumerate(lists[m.final]):
        q, arcs = m.final, []
        while True:
            v, l, a, pr = lists[q][r]
            assert l == length - len(arcs)  # strictly decreasing by one
            if a == NONE:
                assert q == 0 and l == 0
                break
            arcs.append(a)
            q, r = m.src[a], pr
        arcs.reverse()
        assert len(arcs) == length
        w = 0.0
        for a in reversed(arcs):  # the reported weight: the arcs added from the end
            w = m.logw[a] + w
        v = 0.0
        for a in arcs:
            v = v + m.logw[a]
        assert v == value
        out.append((value, w, arcs))
    return out


def best_paths(w, K):
    """-> [(value, reported weight, [arc ids])]: what carmel_hip_decoder_best_paths(k = K) returns for the Wfst w"""
    m = Machine(w)
    return read_out(m, rounds(m, K)[0])


def positive_cycle_arc(w):
    """-> the lowest id of an existing arc of log weight > 0 whose source and destination lie on a common cycle, or None
    (reachability by a transitive closure: for the small machines of the tests)"""
    m = Machine(w)
    reach = np.zeros((m.n_states, m.n_states), bool)
    for q in range(m.n_states):
        for t, _, _ in m.outs[q]:
            reach[q, t] = True
    for k in range(m.n_states):
        reach |= np.outer(reach[:, k], reach[k, :])
    for a, (s, t, x) in enumerate(zip(m.src, m.dst, m.logw)):
        if x > 0.0 and reach[t, s]:  # (a self-loop: reach[s, s] through the arc itself)
            return a
    return None


def enumerate_walks(m, L, exact_length=None):
    """-> [(value, [arc ids])]: every walk of at most L arcs from state 0 that ends in the final state (exact_length: only those
    of exactly that many arcs); values added in path order"""
    out, arcs = [], []

    def go(q, v):
        if q == m.final and (exact_length is None or len(arcs) == exact_length):
            out.append((v, list(arcs)))
        if len(arcs) == L:
            return
        for t, x, a in m.outs[q]:
            arcs.append(a)
            go(t, v + x)
            arcs.pop()

    go(0, 0.0)
    return out


def sorted_walks(m, walks, K):
    """-> the first K of `walks` in the order the rule gives where every sum is exact: value descending, length ascending, last
    arc ascending, then the prefixes in the same order"""
    vals = {}

    def value(p):
        if p not in vals:
            v = 0.0
            for a in p:
                v = v + m.logw[a]
            vals[p] = v
        return vals[p]

    def cmp(p, q):
        while True:
            vp, vq = value(p), value(q)
            if vp != vq:
                return -1 if vp > vq else 1
            if len(p) != len(q):
                return -1 if len(p) < len(q) else 1
            if not p:
                return 0
            if p[-1] != q[-1]:
                return -1 if p[-1] < q[-1] else 1
            p, q = p[:-1], q[:-1]

    if len(walks) > K:  # only walks as good as the K-th value can be among the first K
        cut = sorted((v for v, _ in walks), reverse=True)[K - 1]
        walks = [x for x in walks if x[0] >= cut]
    return sorted((tuple(p) for _, p in walks), key=functools.cmp_to_key(cmp))[:K]
