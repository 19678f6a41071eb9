"""A numpy restatement of pair decoding (carmel --post-b, carmel_hip_decode_pairs / carmel_hip_decode_pairs_sum) for the pair
tests, written independently of csrc/decode_pairs.hip: the trellis over (matched position i, other position j, state q) kept as
full PLANES (i outer, j inner), not anti-diagonals; a cell is reduced with np.logaddexp.at / np.maximum.at over all its
candidates at once (a pairwise form, in any order), not a streaming accumulator per node; the levels of the arcs with epsilon on
both sides are decode_sum_ref.epsilon_levels' depth-first labelling, not a Kahn queue.  Every function takes a dtype: f64 is what
the tests compare the device to, longdouble what they compare f64 to.  count() is the same recursion pushed forward over Python
integers: the exact number of derivations.  enumerate_paths() is brute force: every derivation, by depth-first search.

A pair is (x, y): x spelled by the arcs' matched symbols `msym`, y by their other symbols `osym` (0 = epsilon).  An arc of weight
zero is never used.  By (matched a, other b) an arc feeds (i, j, dst) from: MM (i-1, j-1), M0 (i-1, j), 0M (i, j-1), 00 (i, j)."""
import numpy as np

from decode_sum_ref import CycleError, epsilon_levels  # noqa: F401  (CycleError: re-exported)

NINF = -np.inf


class Prepared(object):
    """the arcs of a machine by what a cell needs: matched arcs by their matched symbol, 0M arcs by their other symbol, 00 arcs
    by the 00 level (1, 2, ...) of their destination; CycleError if the 00 arcs of non-zero weight have a cycle"""

    def __init__(self, n_states, final, src, dst, msym, osym, logw):
        self.Q, self.final = int(n_states), int(final)
        self.src, self.dst = np.asarray(src).astype(np.int64), np.asarray(dst).astype(np.int64)
        self.msym, self.osym = np.asarray(msym).astype(np.int64), np.asarray(osym).astype(np.int64)
        self.logw = np.asarray(logw, np.float64)
        ids = np.arange(len(self.src))
        self.ok = self.logw > NINF
        e00 = ids[self.ok & (self.msym == 0) & (self.osym == 0)]
        self.level = epsilon_levels(self.Q, self.src, self.dst, e00)
        self.n_levels = int(self.level.max()) if self.Q else 0
        self.by_level = [e00[self.level[self.dst[e00]] == L] for L in range(1, self.n_levels + 1)]
        self.by_x = {int(x): ids[self.ok & (self.msym == x)] for x in np.unique(self.msym[self.ok & (self.msym != 0)])}
        zm = self.ok & (self.msym == 0) & (self.osym != 0)
        self.by_y = {int(y): ids[zm & (self.osym == y)] for y in np.unique(self.osym[zm])}
        self._cell = {}
        self.none = ids[:0]

    def cell_arcs(self, x, y):
        """-> (MM, M0, 0M arc ids) of a cell whose matched symbol is x and other symbol y (None: position 0 of that side)"""
        key = (x, y)
        if key not in self._cell:
            m = self.by_x.get(int(x), self.none) if x is not None else self.none
            mm = m[self.osym[m] == y] if y is not None else self.none
            zm = self.by_y.get(int(y), self.none) if y is not None else self.none
            self._cell[key] = (mm, m[self.osym[m] == 0], zm)
        return self._cell[key]


def planes(P, x, y, dtype, reduce_at):
    """-> V [(n + 1), (m + 1), Q] of `dtype`: every node's value, the candidates of a node combined by reduce_at (np.logaddexp.at:
    the sum of all derivations' weights; np.maximum.at: the best derivation's path-order sum)"""
    n, m = len(x), len(y)
    w = P.logw.astype(dtype)
    V = np.full((n + 1, m + 1, P.Q), NINF, dtype)
    V[0, 0, 0] = 0
    with np.errstate(invalid="ignore"):
        for i in range(n + 1):
            for j in range(m + 1):
                mm, m0, zm = P.cell_arcs(x[i - 1] if i else None, y[j - 1] if j else None)
                cell = V[i, j]
                if len(mm):
                    reduce_at(cell, P.dst[mm], V[i - 1, j - 1][P.src[mm]] + w[mm])
                if len(m0):
                    reduce_at(cell, P.dst[m0], V[i - 1, j][P.src[m0]] + w[m0])
                if len(zm):
                    reduce_at(cell, P.dst[zm], V[i, j - 1][P.src[zm]] + w[zm])
                for arcs in P.by_level:  # the sources of a level's arcs are of lower levels: final
                    reduce_at(cell, P.dst[arcs], cell[P.src[arcs]] + w[arcs])
    return V


def pair_sum(P, x, y, dtype=np.float64):
    """-> ln of the sum over the derivations of (x, y) of the product of their arcs' weights (-inf: none)"""
    return planes(P, x, y, dtype, np.logaddexp.at)[len(x), len(y), P.final]


def pair_best(P, x, y, dtype=np.float64):
    """-> (best path-order sum, path as arc ids or None, tied): `tied` says whether some node of the returned path had two best
    candidates.  Among equal candidates the path takes a matched arc before an epsilon arc, then the lowest arc id."""
    V = planes(P, x, y, dtype, np.maximum.at)
    w = P.logw.astype(dtype)
    n, m = len(x), len(y)
    best = V[n, m, P.final]
    if not best > NINF:
        return best, None, False
    ids = np.arange(len(P.src))
    path, tied, i, j, q = [], False, n, m, P.final
    while (i, j, q) != (0, 0, 0):
        mm, m0, zm = P.cell_arcs(x[i - 1] if i else None, y[j - 1] if j else None)
        e00 = ids[P.ok & (P.msym == 0) & (P.osym == 0) & (P.dst == q)]
        hits = []  # (epsilon arc?, arc id, source cell) of the candidates that reach the node's value exactly
        for arcs, di, dj, eps in ((mm, 1, 1, 0), (m0, 1, 0, 0), (zm, 0, 1, 1), (e00, 0, 0, 1)):
            for a in arcs[P.dst[arcs] == q]:
                if V[i - di, j - dj, P.src[a]] + w[a] == V[i, j, q]:
                    hits.append((eps, int(a), i - di, j - dj))
        assert hits, (i, j, q)
        tied |= len(hits) > 1
        _, a, i, j = min(hits)
        path.append(a)
        q = int(P.src[a])
        assert len(path) <= (n + m + 1) * (P.n_levels + 1)
    return best, path[::-1], tied


def count(P, x, y):
    """-> the number of derivations of (x, y), exactly (Python integers, pushed forward from (0, 0, start))"""
    n, m = len(x), len(y)
    outs = {}
    for a in np.nonzero(P.ok)[0]:
        outs.setdefault(int(P.src[a]), []).append((int(P.dst[a]), int(P.msym[a]), int(P.osym[a])))
    cells = {(0, 0): {0: 1}}
    for i in range(n + 1):
        for j in range(m + 1):
            cell = cells.pop((i, j), None)
            if not cell:
                continue
            xi, yj = (x[i] if i < n else None), (y[j] if j < m else None)
            for L in range(P.n_levels + 1):  # a state's count is final once every state of lower 00 level has pushed
                for q in [q for q in cell if P.level[q] == L]:
                    c = cell[q]
                    for dst, a, b in outs.get(q, ()):
                        if a == 0 and b == 0:
                            cell[dst] = cell.get(dst, 0) + c
                            continue
                        if (a != 0 and a != xi) or (b != 0 and b != yj):
                            continue
                        t = cells.setdefault((i + (a != 0), j + (b != 0)), {})
                        t[dst] = t.get(dst, 0) + c
            if (i, j) == (n, m):
                return cell.get(P.final, 0)
    return 0


class TooMany(Exception):
    pass


def enumerate_paths(P, x, y, limit=1 << 20):
    """-> every derivation of (x, y) as a list of arc ids, by depth-first search (the 00 arcs are acyclic: it ends); None if
    there are more than `limit`"""
    n, m = len(x), len(y)
    outs = {}
    for a in np.nonzero(P.ok)[0]:
        outs.setdefault(int(P.src[a]), []).append(int(a))
    found, path = [], []

    def go(q, i, j):
        if q == P.final and i == n and j == m:
            found.append(list(path))
            if len(found) > limit:
                raise TooMany()
        for a in outs.get(q, ()):
            ma, ob = int(P.msym[a]), int(P.osym[a])
            if ma and (i == n or x[i] != ma):
                continue
            if ob and (j == m or y[j] != ob):
                continue
            path.append(a)
            go(int(P.dst[a]), i + (ma != 0), j + (ob != 0))
            path.pop()

    try:
        go(0, 0, 0)
    except TooMany:
        return None
    return found


def rescore(P, x, y, path):
    """-> (the path's weight added in path order, added from the end), after checking that the path runs from the start to the
    final state, spells x and y and uses no arc of weight zero"""
    q, xs, ys, fwd = 0, [], [], 0.0
    for a in path:
        assert P.src[a] == q and P.logw[a] > NINF, (a, q)
        if P.msym[a]:
            xs.append(int(P.msym[a]))
        if P.osym[a]:
            ys.append(int(P.osym[a]))
        fwd = fwd + P.logw[a]
        q = int(P.dst[a])
    assert q == P.final and xs == [int(s) for s in x] and ys == [int(s) for s in y], (xs, ys, list(x), list(y))
    rev = 0.0
    for a in reversed(path):
        rev = P.logw[a] + rev
    return fwd, rev
