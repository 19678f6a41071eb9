"""A numpy restatement of the batch arc posteriors (carmel_hip_decode_posterior) for the posterior tests,
written independently of csrc/decode_posterior.hip: the forward rows are decode_sum_ref.py's recursion with every row kept (its
prepare(), its pairwise np.logaddexp.at, its depth-first epsilon levels), the backward rows the same recursion over the arcs
turned round, and an arc's count the sum over its trellis edges of exp(alpha + w + beta - Z).  Everything is computed in the
`dtype` asked for -- np.float64, or np.longdouble to measure the f64 reference's own error."""
import numpy as np

from decode_sum_ref import prepare

NINF = -np.inf


def rows(n_states, final, prepared, line, dtype=np.float64):
    """-> (alpha, beta): (len + 1) x |Q| arrays of the forward and backward values of the line's trellis nodes"""
    src, dst, logw, by_sym, by_level = prepared
    w = logw.astype(dtype)
    n = len(line)
    alpha = np.full((n + 1, n_states), NINF, dtype)
    beta = np.full((n + 1, n_states), NINF, dtype)
    alpha[0, 0] = 0.0
    beta[n, final] = 0.0
    with np.errstate(invalid="ignore"):
        for i in range(n + 1):
            if i:
                arcs = by_sym.get(int(line[i - 1]))
                if arcs is not None:
                    np.logaddexp.at(alpha[i], dst[arcs], alpha[i - 1][src[arcs]] + w[arcs])
            for arcs in by_level:  # the sources of a level's arcs are of lower levels: final
                np.logaddexp.at(alpha[i], dst[arcs], alpha[i][src[arcs]] + w[arcs])
        for i in range(n, -1, -1):
            if i < n:
                arcs = by_sym.get(int(line[i]))
                if arcs is not None:
                    np.logaddexp.at(beta[i], src[arcs], beta[i + 1][dst[arcs]] + w[arcs])
            for arcs in reversed(by_level):  # the destinations of a level's arcs are final: their own arcs lead higher
                np.logaddexp.at(beta[i], src[arcs], beta[i][dst[arcs]] + w[arcs])
    return alpha, beta


def posterior(n_states, final, src, dst, msym, logw, lines, weights=None, dtype=np.float64, prepared=None):
    """-> (sums [n_lines], counts [n_arcs]) in `dtype`: every line's ln of the sum over its derivations (-inf: none), and per arc
    the sum over the lines with a derivation of weights[l] (1 without weights) times its expected number of uses"""
    prepared = prepared or prepare(n_states, src, dst, msym, logw)
    psrc, pdst, plogw, by_sym, by_level = prepared
    w = plogw.astype(dtype)
    eps = np.concatenate(by_level) if by_level else np.zeros(0, np.int64)
    sums = np.full(len(lines), NINF, dtype)
    counts = np.zeros(len(plogw), dtype)
    for l, line in enumerate(lines):
        alpha, beta = rows(n_states, final, prepared, line, dtype)
        Z = alpha[len(line), final]
        sums[l] = Z
        if not Z > NINF:
            continue
        c = dtype(1.0 if weights is None else weights[l])
        for i in range(len(line) + 1):
            if i:
                arcs = by_sym.get(int(line[i - 1]))
                if arcs is not None:
                    np.add.at(counts, arcs, c * np.exp(alpha[i - 1][psrc[arcs]] + w[arcs] + beta[i][pdst[arcs]] - Z))
            if len(eps):
                np.add.at(counts, eps, c * np.exp(alpha[i][psrc[eps]] + w[eps] + beta[i][pdst[eps]] - Z))
    return sums, counts


def net_flow(n_states, src, dst, counts):
    """-> per state, the counts of the arcs into it less the counts of the arcs out of it"""
    net = np.zeros(n_states, counts.dtype)
    np.add.at(net, np.asarray(dst, np.int64), counts)
    np.subtract.at(net, np.asarray(src, np.int64), counts)
    return net
