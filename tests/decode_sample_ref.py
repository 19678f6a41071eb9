"""A Python restatement of batch posterior path sampling (carmel_hip_decode_sample, Decoder.sample) for the sampling tests,
written independently of csrc/decode_sample.hip: its own splitmix restatement of the library's counter-based uniform, the forward
rows built with np.logaddexp.at as decode_sum_ref.forward builds them (all rows kept), and the candidate lists of a node read
from the arc arrays, not from the device's tables.

The rule.  alpha[i][q] is the forward value of node (i, q).  Sample s of line l of the call walks back from (n, final), step = 0.
At (i, q) the candidates are, in this order: "stop" (value 0.0) if (i, q) = (0, 0); if i > 0 the arcs into q whose matched symbol
is x_i, in arc-id order, value alpha[i - 1][src] + w; the epsilon arcs into q, in arc-id order, value alpha[i][src] + w.  With
Z = alpha[i][q], p_c = exp(value_c - Z) (0 for -inf), S = the p_c added in order, u = uniform(seed, s, l, step), t = u S: the
first candidate with p_c > 0 whose running sum exceeds t is chosen, or the last with p_c > 0.  "Stop" ends the walk; otherwise
the arc is prepended, step += 1, q = the arc's source, and i -= 1 for a matched arc.

A draw is AMBIGUOUS if some running sum other than the last lies within 1e-6 S of t: there a device whose p_c differ from numpy's
in the last bits may choose the neighbouring candidate.  The margin is derived, not measured: the sums' tests bound the device
against numpy at 1e-10 max(1, |value|) with values <~ 1e2, which is <= 1e-8 relative in a p_c; 1e-6 leaves two orders over that."""
import numpy as np

from decode_sum_ref import prepare

NINF = -np.inf
M64 = (1 << 64) - 1
AMBIGUITY = 1e-6


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def uniform(seed, it, block, step):
    """the library's counter-based uniform in [0, 1), 53 bits: a splitmix64 finaliser over (seed, iter, block, step)"""
    h = mix64((seed & M64) ^ 0xD1B54A32D192ED03)
    h = mix64(h ^ (((it & 0xFFFFFFFF) << 32) | (block & 0xFFFFFFFF)))
    h = mix64(h ^ (step & 0xFFFFFFFF))
    return (h >> 11) * (1.0 / 9007199254740992.0)


def _mix64_many(z):
    u = np.uint64
    z = z + u(0x9E3779B97F4A7C15)  # (uint64 arrays wrap)
    z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
    return z ^ (z >> u(31))


def uniform_many(seed, its, block, step):
    """uniform(seed, it, block, step) for an array of `it` (test_decode_sample_host.py compares the two)"""
    u = np.uint64
    h = u(mix64((seed & M64) ^ 0xD1B54A32D192ED03))
    h = _mix64_many(h ^ ((np.asarray(its).astype(u) << u(32)) | u(block & 0xFFFFFFFF)))
    h = _mix64_many(h ^ u(step & 0xFFFFFFFF))
    return (h >> u(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


class Model(object):
    """a machine seen from one side: `msym` the matched side's symbols (0 = epsilon); raises decode_sum_ref.CycleError"""

    def __init__(self, n_states, final, src, dst, msym, logw):
        self.Q, self.final = int(n_states), int(final)
        self.prep = prepare(n_states, src, dst, msym, logw)
        self.src, self.dst, self.logw = self.prep[:3]
        self.msym = np.asarray(msym).astype(np.int64)
        self.into_m, self.into_e = {}, {}  # (dst, symbol) / dst -> arc ids, ascending; no arc of weight zero
        for k in range(len(self.src)):
            if not self.logw[k] > NINF:
                continue
            if self.msym[k] == 0:
                self.into_e.setdefault(int(self.dst[k]), []).append(k)
            else:
                self.into_m.setdefault((int(self.dst[k]), int(self.msym[k])), []).append(k)

    def rows(self, line):
        """-> alpha [len + 1, Q]: decode_sum_ref.forward's rows, every one kept"""
        src, dst, logw, by_sym, by_level = self.prep
        A = np.full((len(line) + 1, self.Q), NINF)
        A[0, 0] = 0.0
        with np.errstate(invalid="ignore"):
            for i in range(len(line) + 1):
                row = A[i]
                if i:
                    arcs = by_sym.get(int(line[i - 1]))
                    if arcs is not None:
                        np.logaddexp.at(row, dst[arcs], A[i - 1][src[arcs]] + logw[arcs])
                for arcs in by_level:
                    np.logaddexp.at(row, dst[arcs], row[src[arcs]] + logw[arcs])
        return A

    def candidates(self, A, line, i, q):
        """-> (arc ids, -1 for "stop"; values) of node (i, q), in candidate order"""
        arcs, vals = [], []
        if i == 0 and q == 0:
            arcs.append(-1)
            vals.append(0.0)
        if i > 0:
            for k in self.into_m.get((q, int(line[i - 1])), ()):
                arcs.append(k)
                vals.append(A[i - 1, self.src[k]] + self.logw[k])
        for k in self.into_e.get(q, ()):
            arcs.append(k)
            vals.append(A[i, self.src[k]] + self.logw[k])
        return np.array(arcs, np.int64), np.array(vals, np.float64)


def sample_line(model, line, l, n, seed, A=None):
    """-> None if the line has no derivation, else (mat [n, L] int64: sample s's arc ids in path order, padded with -1;
    ambiguous [n] bool: some draw of the sample's walk was ambiguous).  l: the line's index in the call.  The n walks run side
    by side: step t of every walk still under way is drawn at once, node by node."""
    A = model.rows(line) if A is None else A
    if not A[len(line), model.final] > NINF:
        return None
    Q = model.Q
    i = np.full(n, len(line), np.int64)
    q = np.full(n, model.final, np.int64)
    active = np.ones(n, bool)
    amb = np.zeros(n, bool)
    cols = []
    step = 0
    while active.any():
        act = np.flatnonzero(active)
        u = uniform_many(seed, act, l, step)
        key = i[act] * Q + q[act]
        col = np.full(n, -1, np.int64)
        for kv in np.unique(key):
            here = key == kv
            sel, t = act[here], u[here]
            ii, qq = divmod(int(kv), Q)
            arcs, vals = model.candidates(A, line, ii, qq)
            p = np.where(vals > NINF, np.exp(vals - A[ii, qq]), 0.0)
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
            q[mv] = model.src[a]
            i[mv] -= model.msym[a] != 0
        cols.append(col)
        step += 1
    mat = np.stack(cols[::-1], axis=1)  # path order; a walk that stopped early has its -1 in front
    mat = np.take_along_axis(mat, np.argsort(mat < 0, axis=1, kind="stable"), axis=1)
    return mat, amb


def sample(model, lines, n, seed, only=None):
    """-> per line of the call None or sample_line's pair; `only`: the line indices wanted (the others get None)"""
    return [sample_line(model, line, l, n, seed) if only is None or l in only else None for l, line in enumerate(lines)]


def paths_of(mat):
    return [[int(a) for a in row if a >= 0] for row in mat]


def is_derivation(model, line, path):
    """starts in state 0, ends in the final state, spells the line on the matched side, uses no arc of weight zero"""
    q, spelt = 0, []
    for a in path:
        if model.src[a] != q or not model.logw[a] > NINF:
            return False
        if model.msym[a]:
            spelt.append(int(model.msym[a]))
        q = int(model.dst[a])
    return q == model.final and spelt == [int(x) for x in line]


def enumerate_derivations(model, line, A=None, limit=1 << 20):
    """-> [(path, ln weight added in path order)]: every derivation of the line, by recursion back from the final node over the
    nodes the forward pass reached (so nothing is explored that no derivation uses)"""
    A = model.rows(line) if A is None else A
    out = []

    def go(i, q, tail):
        assert len(out) < limit
        if i == 0 and q == 0:
            out.append(list(tail[::-1]))
        arcs, vals = model.candidates(A, line, i, q)
        for a, v in zip(arcs, vals):
            if a >= 0 and v > NINF:
                tail.append(int(a))
                go(i - (1 if model.msym[a] else 0), int(model.src[a]), tail)
                tail.pop()

    if A[len(line), model.final] > NINF:
        go(len(line), model.final, [])
    res = []
    for p in out:
        w = 0.0
        for a in p:
            w += model.logw[a]
        res.append((p, w))
    return res


def raw_line_matrix(line_paths, path_off, arcs, l):
    """the paths of line l in the flat arrays of Decoder.sample_raw -> [paths, L] int64 padded with -1, as sample_line's mat"""
    a, b = int(line_paths[l]), int(line_paths[l + 1])
    po = path_off[a:b + 1].astype(np.int64)
    lens = np.diff(po)
    L = int(lens.max()) if len(lens) else 0
    at = np.arange(L)[None, :]
    idx = np.minimum(po[:-1, None] + at, max(len(arcs) - 1, 0))
    return np.where(at < lens[:, None], arcs.astype(np.int64)[idx] if len(arcs) else -1, -1)


def frequencies(mat):
    """-> {path tuple: share of the rows}"""
    if mat.shape[1] == 0:  # (only the empty path)
        return {(): 1.0}
    rows, counts = np.unique(mat, axis=0, return_counts=True)
    return {tuple(int(a) for a in r if a >= 0): c / float(len(mat)) for r, c in zip(rows, counts)}
