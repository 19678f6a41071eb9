"""The rule of carmel_hip_decoder_prune (include/carmel_hip.h, csrc/decode_prune.hip) restated in Python and f64, with the same
additions in the same order, so that the device is held to it bit for bit; and a brute-force enumeration of all paths, which
anchors the rule itself on acyclic machines where every sum is exact (test_prune_host.py).

An entry is (value, length, last arc) or None; NONE is the arc of the empty path."""
import numpy as np

from best_paths_ref import NEG_INF, NONE, Machine

NO_CAP = 0xFFFFFFFF


class _View(object):
    def __init__(self, n_states, final, src, dst, logw):
        self.n_states, self.final, self.src, self.dst, self.logw = n_states, final, src, dst, logw


def machines(w, min_arc_logw=NEG_INF):
    """-> (forward machine, reversed machine) over the arcs that exist: log weight > -inf and >= min_arc_logw"""
    logw = [float(x) if float(x) >= min_arc_logw else NEG_INF for x in w.logw]
    return Machine(_View(w.n_states, w.final, w.src, w.dst, logw)), Machine(_View(w.n_states, w.final, w.dst, w.src, logw))


def relax(m, start):
    """-> (entries, rounds): the K = 1 lists of best_paths_ref.rounds, started at `start`: Jacobi rounds over a worklist, the
    candidates of a state in arc-id order, the greatest value, then the smallest length, then the lowest arc id"""
    ent = [None] * m.n_states
    ent[start] = (0.0, 0, NONE)
    changed, n_rounds = {start}, 0
    while True:
        active = sorted({t for q in changed for t, _, _ in m.outs[q]})
        if not active:
            return ent, n_rounds
        n_rounds += 1
        assert n_rounds <= m.n_states + 1, "did not converge"
        new = {}
        for q in active:
            best = None
            for s, x, a in m.ins[q]:  # in arc-id order: only a strictly earlier candidate replaces the one held
                if ent[s] is None:
                    continue
                v, l = ent[s][0] + x, ent[s][1] + 1
                if best is None or v > best[0] or (v == best[0] and l < best[1]):
                    best = (v, l, a)
            if q == start and (best is None or not best[0] > 0.0):  # the empty path comes before anything of equal value
                best = (0.0, 0, NONE)
            if best is not None:
                new[q] = best
        changed = {q for q, e in new.items() if e != ent[q]}
        for q in changed:
            ent[q] = new[q]


def values(ent):
    return [NEG_INF if e is None else e[0] for e in ent]


def best_path(m, fwd):
    """-> P*'s arcs in path order, following the back-pointers from the final state ([] also when there is no path)"""
    if fwd[m.final] is None:
        return []
    q, arcs = m.final, []
    for k in range(fwd[m.final][1], 0, -1):
        assert fwd[q][1] == k
        arcs.append(fwd[q][2])
        q = m.src[arcs[-1]]
    assert q == 0 and fwd[0] == (0.0, 0, NONE)
    return arcs[::-1]


class Distances(object):
    """what depends on the machine and the arc threshold alone"""

    def __init__(self, w, min_arc_logw=NEG_INF):
        self.m, rev = machines(w, min_arc_logw)
        self.fwd, self.fwd_rounds = relax(self.m, 0)
        self.bwd, self.bwd_rounds = relax(rev, self.m.final)
        self.F, self.R = values(self.fwd), values(self.bwd)
        self.pstar = best_path(self.m, self.fwd)
        m = self.m
        self.T_state = [self.F[q] + self.R[q] for q in range(m.n_states)]
        self.T_arc = [(self.F[s] + x) + self.R[t] if x > NEG_INF else NEG_INF for s, t, x in zip(m.src, m.dst, m.logw)]
        self.order = sorted(range(m.n_states), key=lambda q: (-self.T_state[q], q))  # the cap's order

    def masks(self, log_ratio=np.inf, max_states=NO_CAP):
        """-> (state_keep, arc_keep) as uint8 arrays"""
        m = self.m
        state_keep, arc_keep = np.zeros(m.n_states, np.uint8), np.zeros(len(m.logw), np.uint8)
        f_final = self.F[m.final]
        limit = NEG_INF if log_ratio == np.inf else f_final - log_ratio
        on_arc = set(self.pstar)
        on_state = {m.src[a] for a in self.pstar} | {m.dst[a] for a in self.pstar}
        if f_final > NEG_INF:
            on_state.add(0)  # (the empty path)
        for rank, q in enumerate(self.order):
            state_keep[q] = rank < max_states and (self.T_state[q] >= limit or q in on_state)
        for a, (s, t, x) in enumerate(zip(m.src, m.dst, m.logw)):
            arc_keep[a] = x > NEG_INF and state_keep[s] and state_keep[t] and (self.T_arc[a] >= limit or a in on_arc)
        if not f_final > NEG_INF or not state_keep[0] or not state_keep[m.final]:
            state_keep[:], arc_keep[:] = 0, 0
        return state_keep, arc_keep


def prune(w, log_ratio=np.inf, max_states=NO_CAP, min_arc_logw=NEG_INF):
    """-> (state_keep, arc_keep, F, R): what carmel_hip_decoder_prune and carmel_hip_decoder_prune_distances return for the Wfst w"""
    d = Distances(w, min_arc_logw)
    return d.masks(log_ratio, max_states) + (np.array(d.F), np.array(d.R))


def all_paths(m):
    """-> [(value, [arc ids])] of an ACYCLIC machine: every path from state 0 to the final state, values added in path order"""
    out, arcs = [], []

    def go(q, v):
        assert len(arcs) < m.n_states, "a cycle"
        if q == m.final:
            out.append((v, list(arcs)))
        for t, x, a in m.outs[q]:
            arcs.append(a)
            go(t, v + x)
            arcs.pop()

    go(0, 0.0)
    return out
