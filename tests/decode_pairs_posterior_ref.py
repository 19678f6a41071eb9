"""A numpy restatement of the pair arc posteriors (carmel_hip_decode_pairs_posterior) for the tests, written independently of
csrc/decode_pairs_posterior.hip: forward and backward values kept as full PLANES over (i, j, q), not anti-diagonals -- the
forward is decode_pairs_ref.planes, the backward its mirror image, i and j running down; a cell is reduced with np.logaddexp.at
over all the candidates of one kind at once (a pairwise form, in any order), not a streaming accumulator per node; the edges'
posteriors are formed afterwards, a whole cell's arcs of one kind at a time, and added with np.add.at.  Every function takes a
dtype: f64 is what the tests compare the device to, longdouble what they compare f64 to.

By (matched a, other b) an arc leads from (i, j, src) to: MM (i+1, j+1), M0 (i+1, j), 0M (i, j+1), 00 (i, j); beta[i][j][q] is
the ln of the summed weight of all ways from (i, j, q) to (n, m, final); the posterior of an edge is
exp(alpha[its source node] + w + beta[its destination node] - Z)."""
import numpy as np

from decode_pairs_ref import NINF, planes


def back_planes(P, x, y, dtype):
    """-> B [(n + 1), (m + 1), Q] of `dtype`: every node's backward value"""
    n, m = len(x), len(y)
    w = P.logw.astype(dtype)
    B = np.full((n + 1, m + 1, P.Q), NINF, dtype)
    B[n, m, P.final] = 0
    with np.errstate(invalid="ignore"):
        for i in range(n, -1, -1):
            for j in range(m, -1, -1):
                mm, m0, zm = P.cell_arcs(x[i] if i < n else None, y[j] if j < m else None)
                cell = B[i, j]
                if len(mm):
                    np.logaddexp.at(cell, P.src[mm], B[i + 1, j + 1][P.dst[mm]] + w[mm])
                if len(m0):
                    np.logaddexp.at(cell, P.src[m0], B[i + 1, j][P.dst[m0]] + w[m0])
                if len(zm):
                    np.logaddexp.at(cell, P.src[zm], B[i, j + 1][P.dst[zm]] + w[zm])
                for arcs in reversed(P.by_level):  # the destinations of a level's arcs have only higher levels after them: final
                    np.logaddexp.at(cell, P.src[arcs], cell[P.dst[arcs]] + w[arcs])
    return B


def pair_posterior(P, x, y, dtype=np.float64):
    """-> (Z, counts [n_arcs]): the ln of the pair's sum of all derivations and every arc's expected number of uses over them
    (all 0 if Z = -inf)"""
    n, m = len(x), len(y)
    A = planes(P, x, y, dtype, np.logaddexp.at)
    Z = A[n, m, P.final]
    counts = np.zeros(len(P.src), dtype)
    if not Z > NINF:
        return Z, counts
    B = back_planes(P, x, y, dtype)
    w = P.logw.astype(dtype)
    e00 = np.concatenate(P.by_level) if P.by_level else P.none
    with np.errstate(invalid="ignore"):
        for i in range(n + 1):
            for j in range(m + 1):
                mm, m0, zm = P.cell_arcs(x[i] if i < n else None, y[j] if j < m else None)
                for arcs, di, dj in ((mm, 1, 1), (m0, 1, 0), (zm, 0, 1), (e00, 0, 0)):
                    if len(arcs):
                        p = np.exp(A[i, j][P.src[arcs]] + w[arcs] + B[i + di, j + dj][P.dst[arcs]] - Z)
                        np.add.at(counts, arcs, p)
    return Z, counts


def posterior(P, pairs, weights=None, dtype=np.float64):
    """-> (sums [n_pairs], counts [n_arcs]): counts = the sum over the pairs with a derivation of weights[l] (1 without weights)
    times pair_posterior's counts"""
    sums = np.full(len(pairs), NINF, dtype)
    counts = np.zeros(len(P.src), dtype)
    for l, (x, y) in enumerate(pairs):
        sums[l], c = pair_posterior(P, x, y, dtype)
        if sums[l] > NINF:
            counts += c if weights is None else dtype(weights[l]) * c
    return sums, counts
