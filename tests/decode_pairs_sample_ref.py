"""A numpy restatement of batch pair alignment sampling (carmel_hip_decode_pairs_sample, Decoder.sample_pairs) for the pair
sampling tests, written independently of csrc/decode_pairs_sample.hip: alpha is decode_pairs_ref.planes' full planes reduced with
np.logaddexp.at, the uniform is decode_sample_ref's splitmix restatement, and the candidates of a node are read from the arc
arrays, not from the device's tables.

The rule.  alpha[i][j][q] is the forward value of node (i, j, q) of the pair (x, y), x on the matched side.  Sample s of pair l
of the call walks back from (n, m, final), step = 0.  At (i, j, q) the candidates are, in this order: "stop" (value 0.0) at
(0, 0, 0) only; if i > 0 the arcs into q whose matched symbol is x_i, in arc-id order -- an M0 arc (other symbol 0) with value
alpha[i - 1][j][src] + w, an MM arc only if j > 0 and its other symbol is y_j, with value alpha[i - 1][j - 1][src] + w; the
matched-side-epsilon arcs into q, in arc-id order -- a 00 arc with value alpha[i][j][src] + w, a 0M arc only if j > 0 and its
other symbol is y_j, with value alpha[i][j - 1][src] + w.  With Z = alpha[i][j][q], p_c = exp(value_c - Z) (0 for -inf), S = the
p_c added in order, u = uniform(seed, s, l, step), t = u S: the first candidate with p_c > 0 whose running sum exceeds t is
chosen, or the last with p_c > 0.  "Stop" ends the walk; otherwise the arc is prepended, step += 1, q = the arc's source, i -= 1
if the arc's matched symbol is not epsilon, j -= 1 if its other symbol is not.

A draw is AMBIGUOUS if some running sum other than the last lies within decode_sample_ref.AMBIGUITY (1e-6) S of t.  The margin
is the one-sided sampler's and so is its derivation: the pair sums are held to the same 1e-10 max(1, |value|)
(test_decode_pairs_host.close_enough), values <~ 1e2, which is <= 1e-8 relative in a p_c; 1e-6 leaves two orders over that."""
import numpy as np

from decode_pairs_ref import NINF, planes
from decode_sample_ref import AMBIGUITY, uniform_many


class Into(object):
    """the arcs of a decode_pairs_ref.Prepared by what a node's walk needs: (dst, matched symbol) -> matched arcs, dst ->
    matched-side-epsilon arcs; arc ids ascending, no arc of weight zero"""

    def __init__(self, P):
        self.P = P
        self.m, self.e = {}, {}
        for k in np.nonzero(P.ok)[0]:
            k = int(k)
            if P.msym[k]:
                self.m.setdefault((int(P.dst[k]), int(P.msym[k])), []).append(k)
            else:
                self.e.setdefault(int(P.dst[k]), []).append(k)

    def candidates(self, V, x, y, i, j, q):
        """-> (arc ids, -1 for "stop"; values) of node (i, j, q), in candidate order"""
        P = self.P
        arcs, vals = [], []
        if i == 0 and j == 0 and q == 0:
            arcs.append(-1)
            vals.append(0.0)
        if i > 0:
            for k in self.m.get((q, int(x[i - 1])), ()):
                if P.osym[k] == 0:
                    arcs.append(k)
                    vals.append(V[i - 1, j, P.src[k]] + P.logw[k])
                elif j > 0 and P.osym[k] == y[j - 1]:
                    arcs.append(k)
                    vals.append(V[i - 1, j - 1, P.src[k]] + P.logw[k])
        for k in self.e.get(q, ()):
            if P.osym[k] == 0:
                arcs.append(k)
                vals.append(V[i, j, P.src[k]] + P.logw[k])
            elif j > 0 and P.osym[k] == y[j - 1]:
                arcs.append(k)
                vals.append(V[i, j - 1, P.src[k]] + P.logw[k])
        return np.array(arcs, np.int64), np.array(vals, np.float64)


def into(P):
    if getattr(P, "_into", None) is None:
        P._into = Into(P)
    return P._into


def alpha(P, x, y):
    return planes(P, x, y, np.float64, np.logaddexp.at)


def sample_pair(P, x, y, l, n, seed, V=None):
    """-> None if the pair has no derivation, else (mat [n, L] int64: sample s's arc ids in path order, padded with -1;
    ambiguous [n] bool: some draw of the sample's walk was ambiguous).  l: the pair's index in the call.  The n walks run side by
    side: step t of every walk still under way is drawn at once, node by node."""
    V = alpha(P, x, y) if V is None else V
    N, M, Q = len(x), len(y), P.Q
    if not V[N, M, P.final] > NINF:
        return None
    I = into(P)
    i = np.full(n, N, np.int64)
    j = np.full(n, M, np.int64)
    q = np.full(n, P.final, np.int64)
    active = np.ones(n, bool)
    amb = np.zeros(n, bool)
    cols = []
    step = 0
    while active.any():
        assert step <= (N + M + 1) * (P.n_levels + 1)
        act = np.flatnonzero(active)
        u = uniform_many(seed, act, l, step)
        key = (i[act] * (M + 1) + j[act]) * Q + q[act]
        col = np.full(n, -1, np.int64)
        for kv in np.unique(key):
            here = key == kv
            sel, t = act[here], u[here]
            cell, qq = divmod(int(kv), Q)
            ii, jj = divmod(cell, M + 1)
            arcs, vals = I.candidates(V, x, y, ii, jj, qq)
            p = np.where(vals > NINF, np.exp(vals - V[ii, jj, qq]), 0.0)
            run = np.cumsum(p)  # (added in candidate order)
            S = run[-1]
            t = t * S
            pos = np.flatnonzero(p > 0)
            c = np.minimum(np.searchsorted(run[pos], t, side="right"), len(pos) - 1)  # the first running sum > t, or the last
            chosen = arcs[pos[c]]
            amb[sel] |= (np.abs(run[None, :-1] - t[:, None]) <= AMBIGUITY * S).any(axis=1)
            col[sel] = chosen
            stop = chosen < 0
            active[sel[stop]] = False
            mv, a = sel[~stop], chosen[~stop]
            q[mv] = P.src[a]
            i[mv] -= P.msym[a] != 0
            j[mv] -= P.osym[a] != 0
        cols.append(col)
        step += 1
    mat = np.stack(cols[::-1], axis=1)  # path order; a walk that stopped early has its -1 in front
    mat = np.take_along_axis(mat, np.argsort(mat < 0, axis=1, kind="stable"), axis=1)
    return mat, amb


def sample(P, pairs, n, seed, only=None):
    """-> per pair of the call None or sample_pair's result; `only`: the pair indices wanted (the others get None)"""
    return [sample_pair(P, x, y, l, n, seed) if only is None or l in only else None for l, (x, y) in enumerate(pairs)]
