"""A numpy restatement of the all-paths sum of a line (carmel -b --sum, carmel_hip_decode_sum) for the sum tests: the log-semiring
forward pass over (position, state), written independently of csrc/decode_sum.hip.  A row is reduced with np.logaddexp.at, a
pairwise log1p form, not the kernel's streaming maximum-and-scaled-sum; the epsilon levels are a longest-path labelling found
by depth-first search, not the Kahn queue of upload_tables.  count() is the same recursion over Python integers: the exact
number of derivations."""
import numpy as np

NINF = -np.inf


class CycleError(Exception):
    pass


def epsilon_levels(n_states, src, dst, eps):
    """level[q] = the number of arcs of the longest path of the arcs `eps` that ends in q; CycleError if they have a cycle"""
    preds = [[] for _ in range(n_states)]
    for k in eps:
        preds[int(dst[k])].append(int(src[k]))
    level = [-1] * n_states  # -1 unvisited, -2 on the stack
    for root in range(n_states):
        if level[root] >= 0:
            continue
        stack = [(root, 0)]
        level[root] = -2
        while stack:
            q, at = stack[-1]
            if at < len(preds[q]):
                stack[-1] = (q, at + 1)
                p = preds[q][at]
                if level[p] == -2:
                    raise CycleError("an epsilon cycle through state %d" % p)
                if level[p] == -1:
                    level[p] = -2
                    stack.append((p, 0))
            else:
                level[q] = 1 + max(level[p] for p in preds[q]) if preds[q] else 0
                stack.pop()
    return np.array(level, np.int64)


def prepare(n_states, src, dst, msym, logw):
    """-> (src, dst, logw, matched arc ids by symbol, epsilon arc ids by level 1, 2, ...) without the arcs of weight zero"""
    src, dst, msym, logw = (np.asarray(a) for a in (src, dst, msym, logw))
    src, dst, msym = src.astype(np.int64), dst.astype(np.int64), msym.astype(np.int64)
    ids = np.arange(len(src))
    ok = logw > NINF
    eps = ids[ok & (msym == 0)]
    level = epsilon_levels(n_states, src, dst, eps)
    by_level = [eps[level[dst[eps]] == L] for L in range(1, int(level.max()) + 1 if n_states else 1)]
    by_sym = {}
    for x in np.unique(msym[ok & (msym != 0)]):
        by_sym[int(x)] = ids[ok & (msym == x)]
    return src, dst, logw, by_sym, by_level


def forward(n_states, final, src, dst, msym, logw, line, prepared=None):
    """-> ln of the sum over the derivations of `line` of the product of their arcs' weights (-inf: none); `msym` the matched
    side's symbols (0 = epsilon)"""
    src, dst, logw, by_sym, by_level = prepared or prepare(n_states, src, dst, msym, logw)

    def close(row):
        for arcs in by_level:  # the sources of a level's arcs are of lower levels: final
            np.logaddexp.at(row, dst[arcs], row[src[arcs]] + logw[arcs])

    row = np.full(n_states, NINF)
    row[0] = 0.0
    with np.errstate(invalid="ignore"):
        close(row)
        for x in line:
            nxt = np.full(n_states, NINF)
            arcs = by_sym.get(int(x))
            if arcs is not None:
                np.logaddexp.at(nxt, dst[arcs], row[src[arcs]] + logw[arcs])
            close(nxt)
            row = nxt
    return float(row[final])


def count(n_states, final, src, dst, msym, logw, line, prepared=None):
    """-> the number of derivations of `line`, exactly"""
    src, dst, logw, by_sym, by_level = prepared or prepare(n_states, src, dst, msym, logw)

    def close(row):
        for arcs in by_level:
            for k in arcs:
                c = row.get(int(src[k]))
                if c:
                    row[int(dst[k])] = row.get(int(dst[k]), 0) + c

    row = {0: 1}
    close(row)
    for x in line:
        nxt = {}
        arcs = by_sym.get(int(x))
        if arcs is not None and row:
            for k in arcs:
                c = row.get(int(src[k]))
                if c:
                    nxt[int(dst[k])] = nxt.get(int(dst[k]), 0) + c
        close(nxt)
        row = nxt
    return row.get(int(final), 0)
