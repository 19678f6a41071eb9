"""A Python restatement of the sums over all paths of the whole machine (carmel_hip_decoder_machine_sums,
csrc/decode_machine_sums.hip; include/carmel_hip.h has the rule) for the machine-sums tests: the useful states U, the levels of
both directions, alpha, beta and ln gamma in np.longdouble, the path counts cf and cb as Python integers, and beside every sum an
error bound that is computed from these reference values alone, never from what a device returned.

The rule, restated.  Only arcs of log weight > -inf exist.  q is in U iff it is reachable from state 0 and reaches the final state
over existing arcs; useful arcs have both ends in U.  U is peeled by in-degree over the useful arcs, state 0 at level 0,
level(q) = 1 + max level(src a); a useful state that never reaches in-degree 0 lies on or behind a cycle inside U, and the lowest
such state is what the refusal names (`stuck`).  alpha[0] = 0, alpha[q] = ln sum exp(alpha[src a] + w(a)) over the useful in-arcs;
beta the same on the reversed machine from the final state; Z = alpha[final]; cf[0] = 1, cf[q] = sum cf[src a]; N = cf[final];
ln gamma(a) = alpha[src a] + w(a) + beta[dst a] - Z for a useful arc, -inf otherwise.

The bound E(q) on |alpha_device[q] - alpha[q]|, u = 2^-53.  E(0) = 0: alpha[0] is the constant 0.0.
  * One useful in-arc (d = 1).  The device returns fl(alpha_device[src] + w) bit for bit (Lse keeps a single term as it is).  The
    operand is off by at most E(src), the addition rounds once, by at most u |t| with t = alpha[src] + w:
    E(q) = E(src) + u |t|.
  * d > 1 in-arcs.  Every term t_i = alpha[src_i] + w_i reaches Lse off by at most E(src_i) + u |t_i|.  A log-sum-exp is a weighted
    mean of its terms' perturbations (its partial derivatives are the posteriors, non-negative and summing to 1), so moving every
    term by at most e moves the value by at most e: max_i (E(src_i) + u |t_i|).  Lse itself, on the terms it is given, is within
    (4 d + 4) u + u |value| of the exact log-sum-exp: the bound tests/test_sweep_math_host.py holds sweep_math.hpp to on the host
    and tests/test_sweep_math_gpu.py on the device (profiles/measurement_log_sweep_math.md: exp within 1 ulp, log within 2.5 ulp).
    E(q) = max_i (E(src_i) + u |t_i|) + (4 d + 4) u + u |alpha[q]|.
    The wavefront form stays inside the same figure.  A lane folds its own d_l <= ceil(d / 64) terms through an Lse of its own,
    4 d_l u relative on its scaled sum; a shuffle step combines two (m, acc) pairs as acc_hi + acc_lo exp(m_lo - m_hi), under 5 u
    of the combined sum (one rounded difference, one exp, one product, one addition: tests/test_consolidate_gpu.py derives it),
    and leaves the operands' relative errors as a weighted mean.  Up to 64 terms every lane holds one term, exactly, and only
    ceil(log2 d) steps combine two non-empty pairs: 5 ceil(log2 d) u <= (4 d + 4) u for every d >= 2.  Above 64 terms:
    (4 ceil(d / 64) + 30) u <= (4 d + 4) u.
beta is bounded in the same way on the reversed machine (Eb).  ln gamma(a) is three more additions of values each off by at most
E(src a), Eb(dst a) and E(final): its bound is E(src) + Eb(dst) + E(final) + 4 u max |term|, the terms being the partial sums
alpha + w, alpha + w + beta, Z and the result.
The reference's own arithmetic is np.longdouble (64 bits of mantissa where the tests run: 2^-11 of u a step); it is not part of
the bound.

The path counts are exact integers here.  The device adds f64s: exact while every count is below 2^53; above, cf[q] carries a
relative error of at most k u / (1 - k u), k = `adds`[q] = max_i adds[src_i] + (d - 1), the longest chain of rounded additions
behind it (adding 0.0 from a lane without terms is exact, and a tree over d leaves is no deeper than d - 1)."""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
NONE = 0xFFFFFFFF
NEG_INF = LD(-np.inf)


def lse(terms):
    """ln sum exp over longdoubles (none: -inf)"""
    if not terms:
        return NEG_INF
    m = max(terms)
    if len(terms) == 1:
        return m
    return m + np.log(sum((np.exp(t - m) for t in terms), LD(0.0)))


class Direction(object):
    """one direction's sweep: levels, sums, their bounds, path counts.  into[q]: the useful arcs (id, from-state) into q in arc-id
    order; order: the states of U in peeling order"""

    def __init__(self, n_states, start, useful, arcs, logw):
        self.level = [NONE] * n_states
        self.sum = [NEG_INF] * n_states
        self.bound = [LD(0.0)] * n_states
        self.count = [0] * n_states
        self.adds = [0] * n_states
        self.degree = [0] * n_states
        into = [[] for _ in range(n_states)]
        out = [[] for _ in range(n_states)]
        for a, s, t in arcs:  # (arc id, the state the sums flow from, the state they flow into), in arc-id order
            into[t].append((a, s))
            out[s].append(t)
        deg = [len(x) for x in into]
        self.degree = list(deg)
        self.levels = 0
        self.n_peeled = 0
        front = [start] if useful[start] and deg[start] == 0 else []
        if front:
            self.sum[start], self.count[start] = LD(0.0), 1
        lvl = 0
        while front:
            nxt = []
            for q in front:
                self.level[q] = lvl
                self.n_peeled += 1
                if lvl:
                    self._state(q, into[q], logw)
                for t in out[q]:
                    deg[t] -= 1
                    if deg[t] == 0:
                        nxt.append(t)
            front = nxt
            lvl += 1
        self.levels = lvl
        self.stuck = min([q for q in range(n_states) if useful[q] and self.level[q] == NONE], default=None)

    def _state(self, q, into, logw):
        terms = [self.sum[s] + LD(logw[a]) for a, s in into]
        d = len(terms)
        self.sum[q] = lse(terms)
        moved = max(self.bound[s] + U * abs(t) for (a, s), t in zip(into, terms))
        self.bound[q] = moved if d == 1 else moved + (4 * d + 4) * U + U * abs(self.sum[q])
        self.count[q] = sum(self.count[s] for _, s in into)
        self.adds[q] = max(self.adds[s] for _, s in into) + (d - 1)


class MachineSums(object):
    def __init__(self, w):
        Q, final = w.n_states, w.final
        self.n_states, self.final = Q, final
        logw = [float(x) for x in w.logw]
        src, dst = [int(x) for x in w.src], [int(x) for x in w.dst]
        exists = [x > -np.inf for x in logw]
        assert not any(np.isnan(x) or x == np.inf for x in logw)

        def reach(start, a, b):
            adj = [[] for _ in range(Q)]
            for k in range(len(a)):
                if exists[k]:
                    adj[a[k]].append(b[k])
            seen = [False] * Q
            seen[start] = True
            todo = [start]
            while todo:
                for t in adj[todo.pop()]:
                    if not seen[t]:
                        seen[t] = True
                        todo.append(t)
            return seen

        rf, rb = reach(0, src, dst), reach(final, dst, src)
        self.useful = [rf[q] and rb[q] for q in range(Q)]
        self.n_useful = sum(self.useful)
        self.arc_useful = [exists[k] and self.useful[src[k]] and self.useful[dst[k]] for k in range(len(src))]
        ua = [k for k in range(len(src)) if self.arc_useful[k]]
        self.F = Direction(Q, 0, self.useful, [(k, src[k], dst[k]) for k in ua], logw)
        self.B = Direction(Q, final, self.useful, [(k, dst[k], src[k]) for k in ua], logw)
        self.stuck = self.F.stuck  # the lowest useful state the forward peeling leaves: the refusal names it
        self.refused = self.stuck is not None
        assert self.refused == (self.B.stuck is not None)
        if self.refused:
            return
        self.alpha, self.beta, self.E, self.Eb = self.F.sum, self.B.sum, self.F.bound, self.B.bound
        self.cf, self.cb = self.F.count, self.B.count
        self.level = self.F.level
        self.levels = (self.F.levels, self.B.levels)
        self.Z, self.N = self.alpha[final], self.cf[final]
        self.ln_gamma, self.Eg = [], []
        for k in range(len(src)):
            if not self.arc_useful[k]:
                self.ln_gamma.append(NEG_INF)
                self.Eg.append(LD(0.0))
                continue
            t1 = self.alpha[src[k]] + LD(logw[k])
            t2 = t1 + self.beta[dst[k]]
            g = t2 - self.Z
            self.ln_gamma.append(g)
            self.Eg.append(self.E[src[k]] + self.Eb[dst[k]] + self.E[final] + 4 * U * max(abs(t1), abs(t2), abs(self.Z), abs(g)))

    def worst_bound(self):
        """the largest bound of any value of the case"""
        if self.refused:
            return LD(0.0)
        return max([LD(0.0)] + list(self.E) + list(self.Eb) + list(self.Eg))

    @staticmethod
    def count_bound(adds):
        """the relative error of a path count behind `adds` rounded additions"""
        k = LD(adds) * U
        return k / (1 - k)


def enumerate_paths(w, limit=10000):
    """-> [(arc ids)]: every path from state 0 that ends the first time it is in the final state, over existing arcs, by an
    iterative depth-first walk that enters only states from which the final state can be reached; None if there are more than
    `limit` (or a cycle is met: a walk longer than the states)"""
    Q = w.n_states
    back = [[] for _ in range(Q)]
    for k in range(w.n_arcs):
        if w.logw[k] > -np.inf:
            back[int(w.dst[k])].append(int(w.src[k]))
    alive, todo = {w.final}, [w.final]
    while todo:
        for s in back[todo.pop()]:
            if s not in alive:
                alive.add(s)
                todo.append(s)
    if 0 not in alive:
        return []
    out = [[] for _ in range(Q)]
    for k in range(w.n_arcs):
        if w.logw[k] > -np.inf and int(w.dst[k]) in alive:
            out[int(w.src[k])].append(k)
    paths = []
    if w.final == 0:
        return [()]
    stack = [(0, iter(out[0]))]
    path = []
    while stack:
        q, it = stack[-1]
        k = next(it, None)
        if k is None:
            stack.pop()
            if path:
                path.pop()
            continue
        t = int(w.dst[k])
        path.append(k)
        if t == w.final:
            paths.append(tuple(path))
            path.pop()
            if len(paths) > limit:
                return None
            continue
        if len(path) > Q:
            return None
        stack.append((t, iter(out[t])))
    return paths
