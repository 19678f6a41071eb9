"""A Python restatement of pair k-best decoding (carmel --post-b with -k n; carmel_hip_decode_pairs_kbest) for the pair k-best
tests, written independently of csrc/decode_pairs_kbest.hip: a dynamic programme over full PLANES (matched position i outer, other
position j inner; no anti-diagonals) that carries WHOLE paths (no back-pointers, no bisection).  Within a cell the states go in a
topological order of the arcs with epsilon on both sides (decode_kbest_ref.eps_order: a Kahn queue).  Every node keeps its best
K + 1 entries (value, arc tuple); the extra one shows whether the K-th place is tied.

A derivation of the pair (x, y) runs from state 0 to the final state, uses no arc of weight zero, and its matched symbols without
epsilons spell x, its other symbols y (decode_pairs_ref.Prepared holds the arcs).  Its value is its arcs' weights added in path
order from the start in f64.  By (matched a, other b) an arc feeds (i, j, dst) from: MM (i-1, j-1), M0 (i-1, j), 0M (i, j-1),
00 (i, j).  Candidates at a node are (arc a into it, rank r in the source node's list), ordered by value descending, arcs whose
matched symbol is not epsilon before arcs whose matched symbol is, arc id ascending, r ascending.  Node (0, 0, start) keeps its
initial list [0.0]."""
from decode_kbest_ref import eps_order


def kbest(P, x, y, K):
    """-> (values, paths, tied): the min(K, number of derivations) best derivations of the pair (x, y) under the Prepared machine
    P, best first -- their values (path-order sums) and arc-id tuples -- and whether two of the best K + 1 have equal values (then
    which paths are returned, and in which order, is decided by the tie rule alone)"""
    n, m = len(x), len(y)
    Q = P.Q
    live = [a for a in range(len(P.src)) if P.ok[a]]
    e00 = [a for a in live if P.msym[a] == 0 and P.osym[a] == 0]
    order = eps_order(Q, P.src, P.dst, e00)
    into = [[] for _ in range(Q)]  # (arc, matched symbol, other symbol), arc ids ascending
    for a in live:
        into[int(P.dst[a])].append((a, int(P.msym[a]), int(P.osym[a])))
    keep = K + 1
    empty = [[] for _ in range(Q)]
    plane = {}
    for i in range(n + 1):
        xi = int(x[i - 1]) if i else None
        for j in range(m + 1):
            yj = int(y[j - 1]) if j else None
            cell = [None] * Q
            mm = plane.get((i - 1, j - 1), empty)
            m0 = plane.get((i - 1, j), empty)
            zm = plane.get((i, j - 1), empty)
            for q in order:
                if i == 0 and j == 0 and q == 0:
                    cell[q] = [(0.0, ())]
                    continue
                cands = []
                for a, ma, ob in into[q]:
                    if ma:
                        if ma != xi:
                            continue
                        if ob:
                            if ob != yj:
                                continue
                            source = mm
                        else:
                            source = m0
                    elif ob:
                        if ob != yj:
                            continue
                        source = zm
                    else:
                        source = cell
                    w = P.logw[a]
                    for r, (v, p) in enumerate(source[int(P.src[a])]):
                        cands.append((v + w, 0 if ma else 1, a, r, p + (a,)))
                cands.sort(key=lambda c: (-c[0], c[1], c[2], c[3]))
                cell[q] = [(c[0], c[4]) for c in cands[:keep]]
            plane[(i, j)] = cell
        for j in range(m + 1):
            plane.pop((i - 2, j), None)
    ents = plane[(n, m)][P.final]
    vals = [float(v) for v, _ in ents]
    tied = len(set(vals)) < len(vals)
    return vals[:K], [p for _, p in ents[:K]], tied
