"""A numpy restatement of 1-best decoding (carmel -b -k 1) for the decoding tests: the (max, +) trellis over (position, state) of
csrc/decode.hip, written independently of it.  Weights add in path order from the start; a node's back-pointer is the lowest arc
id among its best candidates (the kernel then reports the path's weight added from the end: rescore).  The epsilon closure is Jacobi rounds to a fixed point (at most |Q|), not the kernel's levels."""
import gzip
import json
import os

import numpy as np

NINF = -np.inf


class CycleError(Exception):
    pass


def viterbi(n_states, final, src, dst, msym, logw, line):
    """-> (best ln weight, path as arc ids or None, tied): `msym` the matched side's symbols (0 = epsilon); `tied` says whether
    some node of the returned path had two best candidates (the path is then one of several of equal weight)"""
    src, dst, msym, logw = (np.asarray(a) for a in (src, dst, msym, logw))
    ids = np.arange(len(src))
    ok = logw > NINF
    eps = ids[ok & (msym == 0)]
    rows, bps = [], []

    def close(d, bp):
        for _ in range(n_states + 1):
            if not len(eps):
                return
            v = d[src[eps]] + logw[eps]
            o = np.lexsort((eps, -v, dst[eps]))  # per dst: the largest value, then the lowest arc id
            first = np.r_[True, dst[eps][o][1:] != dst[eps][o][:-1]]
            q, vv, aa = dst[eps][o][first], v[o][first], eps[o][first]
            better = vv > d[q]
            if not better.any():
                return
            d[q[better]] = vv[better]
            bp[q[better]] = aa[better]
        raise CycleError("best_path_has_cycle")

    d = np.full(n_states, NINF)
    d[0] = 0.0
    bp = np.full(n_states, -1, np.int64)
    close(d, bp)
    rows.append(d)
    bps.append(bp)
    for x in line:
        m = ids[ok & (msym == x) & (msym != 0)]
        nd = np.full(n_states, NINF)
        nbp = np.full(n_states, -1, np.int64)
        if len(m):
            v = d[src[m]] + logw[m]
            o = np.lexsort((m, -v, dst[m]))
            first = np.r_[True, dst[m][o][1:] != dst[m][o][:-1]]
            q, vv, aa = dst[m][o][first], v[o][first], m[o][first]
            live = vv > NINF
            nd[q[live]] = vv[live]
            nbp[q[live]] = aa[live]
        close(nd, nbp)
        d, bp = nd, nbp
        rows.append(d)
        bps.append(bp)
    best = rows[-1][final]
    if not best > NINF:
        return best, None, False
    path, tied, i, q = [], False, len(line), final
    while bps[i][q] >= 0:
        # another arc that reaches this node's value exactly is a tie
        into = ids[ok & (dst == q)]
        n_best = 0
        for a in into:
            if msym[a] == 0:
                n_best += rows[i][src[a]] + logw[a] == rows[i][q]
            elif i > 0 and msym[a] == line[i - 1]:
                n_best += rows[i - 1][src[a]] + logw[a] == rows[i][q]
        tied |= n_best > 1
        a = bps[i][q]
        path.append(a)
        if msym[a] != 0:
            i -= 1
        q = src[a]
        assert len(path) <= (len(line) + 1) * n_states
    assert i == 0 and q == 0
    return best, path[::-1], tied


def rescore(src, dst, msym, logw, line, path, final):
    """-> (the path's weight added in path order, added from the end -- what the k-best search reports), after checking that
    the path runs from the start to `final` and spells `line`"""
    q, w, spelled = 0, 0.0, []
    for a in path:
        assert src[a] == q
        w = w + logw[a]
        if msym[a] != 0:
            spelled.append(msym[a])
        q = dst[a]
    assert q == final and spelled == list(line)
    r = 0.0
    for a in path[::-1]:
        r = logw[a] + r
    return w, r


def golden_text(golden_dir, name):
    """a decoding fixture's text: tests/golden/<name>, or <name>.gz for the larger ones (make_decode_golden.py)"""
    path = os.path.join(golden_dir, name)
    if os.path.exists(path):
        return open(path).read()
    with gzip.open(path + ".gz", "rt") as f:
        return f.read()


def golden_file(golden_dir, name, tmp_dir):
    """a path the front end can read: the fixture itself, or its decompressed copy in tmp_dir"""
    path = os.path.join(golden_dir, name)
    if os.path.exists(path):
        return path
    out = os.path.join(str(tmp_dir), name)
    with open(out, "w") as f:
        f.write(golden_text(golden_dir, name))
    return out


def decode_expected(golden_dir):
    return json.loads(golden_text(golden_dir, "decode_expected.json"))
