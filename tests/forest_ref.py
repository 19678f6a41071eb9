"""forest-em's E-step, Viterbi and M-step restated in extended precision, their tolerances, and the corpora they are tested on
(test_forest_ref_host.py on the CPU, test_forest_f80_gpu.py against forest_estimate_ext_kernel, forest_estimate_kernel<false> and
<true>, forest_viterbi_kernel<GCOL>, forest_mstep_kernel and the count_reduce pass).

Reference.  `reference` walks the packed arrays (node_off, label, ref, next) directly: label 0 is an OR node, anything else an
AND node carrying that rule, ref >= 0 a back-reference to a shared sub-forest, the children of node i run from i + 1 in steps
of next (forest_enum.children).  From the definitions (forest-em/forest.hpp's inside_rec and compute_norm_outside, as the
kernels' comments cite them), in the log domain, dtype = numpy's longdouble (64-bit mantissa: asserted when sweep_math_cases is
imported):
    inside(AND) = ln w[rule] + sum of inside(child)            inside(OR) = ln sum exp inside(child)
    outside(root) = -ln p                                       ln p = inside(root)
    outside(child) = ln sum over its uses of   outside(OR parent)   or   outside(AND parent) + inside(parent) - inside(child)
    posterior(AND) = exp(inside + outside)                      count[rule] = sum of the posteriors of its AND nodes
An AND parent of inside -inf passes nothing on (the 0/0 guard of forest.hpp:470); a forest of ln p = -inf has no posterior and
is counted in n_zero; the average is over the others.  Sums are log-sum-exps over ALL their terms: nothing is cut off.  The same
walk runs with dtype = float64 (test_forest_ref_host.py).  `viterbi_ref` is the max-product value, `score` the ln weight of
a returned derivation parsed against the forest, `mstep_ref` normalize.hpp:123-164 over the norm groups.

Tolerance (`Tolerance`), u = 2^-53, from what the reference run reports (`Stats`).  The kernels come in two arithmetic forms:
the log domain (forest_estimate_kernel) and mantissa x 2^exponent pairs (forest_estimate_ext_kernel).  A step is one node.
  * A step costs at most (2 A + 4) u of the stored ln value plus 4 u per term folded, A the largest |ln value| stored.
      log form: an AND node adds its children to ln w one by one, a rounded addition of values up to A each (A u per child;
        the children are steps of their own below); an OR node is the streaming log-sum-exp of d terms, within
        (4 d + 4) u + u |value| of the exact one of its inputs (sweep_math_cases.py).
      ext form: a rule's weight enters through fx_from_ln -- ln w x log2 e is one rounded product of a rounded constant
        (2 A u of the ln value), the fraction l2 - floor(l2) is exact, exp2 is within 1 ulp (2 u) --; every product is one
        rounding (u), every aligned add one rounding (u; the bits the smaller addend loses in its shift are below that);
        ln p = log(m) + e ln 2 at the end is a logarithm within 1 ulp of a value below 0.7, a rounded product and a rounded
        addition of values up to A (2 A u + 2 u).  Each fits (2 A + 4) u a step and 4 u a term.
  * Errors ADD over the children of an AND node (a product) and an OR node moves by at most the largest error of its terms.
    So L_in, "the longest chain of dependent operations" of the inside pass, is counted as 1 + the sum over the children at an
    AND node and 1 + the maximum at an OR node, a shared sub-forest once per use: the height of the forest for a spine, the size
    of the largest derivation (OR steps included) otherwise.  D_in counts the terms folded the same way.
        ln p:  E_in = (L_in (2 A + 4) + 4 D_in) u
    It bounds ln p absolutely; ln p is compared relative to max(1, |ln p|), which is no smaller.
  * outside(root) = -ln p is exact in the log form and one rounded reciprocal in the ext form: the first step of the outside
    chain.  A step down from an AND parent is (outside + inside(parent)) - inside(child): two rounded additions of values up to
    2 A (4 A u) in the log form, a product, a divide and an aligned add (3 u) in the ext form; the accumulation into the
    child's outside value is a pairwise log-add -- exp and log1p within 1 ulp each on a sum of at least 1 (4 u), the result
    rounded (A u) -- or an aligned add (u): (5 A + 4) u a step and 4 u per contribution.  L_out is the longest chain of such
    steps from the root, D_out the contributions folded along it.  What a step takes from the inside pass, the stored inside
    values of the parent and of the child, carries their error: no more than E_in for the whole chain together, as the
    sub-forests whose errors enter along one chain are the disjoint parts of one derivation.
  * The log form's pairwise add drops the smaller term beyond 36 nats (f_lwadd); the ext form and the reference drop nothing.
    A dropped term is at most e^-36 = 2.4e-16 of the sum; with c the most adds along an outside chain: c 2.4e-16.
        E_out = (L_out (5 A + 4) + 4 D_out) u + c 2.4e-16
  * A posterior is exp(inside + outside): the errors of both (E_in for the node's own inside value, E_in + E_out for what
    reached its outside value), one rounded addition of values up to A and an exponential within 1 ulp (ext: one product, one
    ldexp); an absolute error e of the argument is a relative error e of the result.  A count sums up to N non-negative
    posteriors in some order (count_reduce_kernel, or 4096 at a time with an atomic each: count_reduce_hot_kernel): N u more.
        counts:  2 E_in + E_out + (2 A + 2 + N) u
    compared relative, on the entries above 1e-200 x the total (dense_ref.compare_counts).
  * Viterbi is additions only: the value of the best derivation is ln w plus its children, each addition rounded at a value
    of at most A_v (the largest |value| of the max-product pass, which is further from 0 than the inside pass's), a maximum is
    exact and moves by at most the largest error of its terms:  L_in A_v u.
  * M-step (forest_mstep_kernel): a group's sum runs over its n terms count + prior one after the other -- each term one
    rounded addition (u), the running sum of non-negative terms within n u --, + add_k (u), the rule's own count + prior (u),
    one divide (u): the logarithm's argument is within (n + 4) u, relatively, which is that much of ln w absolutely; the
    logarithm is within 1 ulp of its result, at most 2 u |ln w|:
        ln weight:  (n + 4 + 2 A_w) u,   n the largest group, A_w the largest finite |new ln weight|
    The largest change max |exp(new) - exp(old)| takes two exponentials within 1 ulp (2 u each) of arguments off by that much,
    of values up to W = max(1, the largest old or new weight), and one rounded difference:
        max change:  W ((n + 4 + 2 A_w) u + 5 u)
CEILING = 1e-10 is a condition, not a measurement: every case's bounds must come out under it from the reference alone
(asserted in test_forest_ref_host.py); a case that does not is made smaller.  The deepest case here, 60 AND levels of weight
1e-8 (ln p about -1105, L_in 62, A 1105), comes out at 1.5e-11 for ln p and 7e-11 for the counts."""
import numpy as np

import sweep_math_cases  # noqa: F401  (asserts that numpy's longdouble has a 64-bit mantissa)
from forest_enum import children

LD = np.longdouble
U = 2.0 ** -53
CUT = 2.4e-16  # e^-36
CEILING = 1e-10
COUNT_HOT, HOT_CHUNK = 64, 4096      # count_reduce: a rule of more than 64 slots is summed in chunks of 4096
LDS_BYTES = 150 * 1024               # dynamic LDS a forest kernel may ask for (forest.hpp: F_LDS_LIMIT)
CLASS_MIN_GROUPS, CLASS_NUM, CLASS_DEN = 256, 2, 3   # a launch class ends after 256 groups, where the groups are 2/3 of its largest


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
class Stats(object):
    def __init__(self):
        self.L_in = self.D_in = self.L_out = self.D_out = self.N = self.c = 0
        self.A = 0.0


class Tolerance(object):
    def __init__(self, st):
        self.L_in, self.D_in, self.L_out, self.D_out, self.A, self.N, self.c = st.L_in, st.D_in, st.L_out, st.D_out, st.A, st.N, st.c
        self.e_in = (self.L_in * (2.0 * self.A + 4.0) + 4.0 * self.D_in) * U
        self.e_out = (self.L_out * (5.0 * self.A + 4.0) + 4.0 * self.D_out) * U + self.c * CUT
        self.lnp = self.e_in
        self.counts = 2.0 * self.e_in + self.e_out + (2.0 * self.A + 2.0 + self.N) * U

    def __repr__(self):
        return "L=%d+%d D=%d+%d A=%.4g N=%d c=%d: ln p %.3g, counts %.3g" % (
            self.L_in, self.L_out, self.D_in, self.D_out, self.A, self.N, self.c, self.lnp, self.counts)


def _lse(vals, dtype):
    m = max(vals)
    if not m > -np.inf:  # every term -inf (or a NaN among them, which then stays)
        return m if m != m else dtype(-np.inf)
    s = dtype(0)
    for v in vals:
        s = s + np.exp(v - m)
    return m + np.log(s)


def _flatten(lab, rf, nx):
    """(non-reference nodes in post-order, children per node with back-references resolved)"""
    n = len(lab)
    nodes = [i for i in range(n) if rf[i] < 0]
    order = sorted(nodes, key=lambda i: (nx[i], -i))  # the end of the subtree ascending, its start descending

    def res(c):
        while rf[c] >= 0:
            c = rf[c]
        return c
    return order, {i: [res(c) for c in children(nx, i)] for i in nodes}


class Result(object):
    """lnp per forest, counts per rule, avg over the live forests, n_zero, post[f] = {node: posterior} of the AND nodes,
    slots per rule, tol"""


def reference(node_off, label, ref, nxt, logw, dtype=LD, variant=None):
    """the E-step of the corpus under the ln weights logw.  variant (test_forest_ref_host.py's sensitivity checks): a subtly
    wrong walk -- "shared_once": a shared sub-forest used twice by one parent gets that parent's share once; "skip_first_or":
    the first child of every OR node gets nothing in the outside pass; "no_guard": without the 0/0 guard"""
    lw = np.asarray(logw, dtype)
    n_forests = len(node_off) - 1
    NEG = dtype(-np.inf)
    res = Result()
    res.lnp = np.full(n_forests, -np.inf, dtype)
    res.counts = np.zeros(len(lw), dtype)
    res.slots = np.zeros(len(lw), np.int64)
    res.post = []
    res.n_zero = 0
    st = Stats()
    lab_all, rf_all, nx_all = np.asarray(label).tolist(), np.asarray(ref).tolist(), np.asarray(nxt).tolist()
    with np.errstate(all="ignore"):
        for f in range(n_forests):
            b, e = int(node_off[f]), int(node_off[f + 1])
            lab, rf, nx = lab_all[b:e], rf_all[b:e], nx_all[b:e]
            order, kids = _flatten(lab, rf, nx)
            assert order[-1] == 0, "the root is the forest's first node"
            ins, Lin, Din = {}, {}, {}
            for i in order:
                k = kids[i]
                if lab[i]:
                    res.slots[lab[i]] += 1
                    v = lw[lab[i]]
                    for c in k:
                        v = v + ins[c]
                    Lin[i], Din[i] = 1 + sum(Lin[c] for c in k), len(k) + sum(Din[c] for c in k)
                else:
                    v = _lse([ins[c] for c in k], dtype)
                    Lin[i], Din[i] = 1 + max(Lin[c] for c in k), len(k) + max(Din[c] for c in k)
                ins[i] = v
            st.L_in, st.D_in = max(st.L_in, Lin[0]), max(st.D_in, Din[0])
            mags = [abs(float(v)) for v in ins.values()]
            lp = ins[0]
            res.lnp[f] = lp
            post = {}
            res.post.append(post)
            if not lp > -np.inf:
                res.n_zero += 1
                for i in order:
                    if lab[i]:
                        post[i] = dtype(0)
                st.A = max([st.A] + [m for m in mags if m < np.inf])
                continue
            contrib = {i: [] for i in order}
            contrib[0].append(-lp)
            Lout, Dpar, Cpar = {0: 0}, {0: 0}, {0: 0}
            for i in reversed(order):
                cs = contrib[i]
                if not cs:  # reached by no use of non-zero outside value
                    if lab[i]:
                        post[i] = dtype(0)
                    continue
                out = _lse(cs, dtype) if len(cs) > 1 else cs[0]
                live = sum(1 for v in cs if v > -np.inf)
                lo, do, co = Lout[i] + 1, Dpar[i] + len(cs), Cpar[i] + max(live - 1, 0)
                st.L_out, st.D_out, st.c = max(st.L_out, lo), max(st.D_out, do), max(st.c, co)
                mags.append(abs(float(out)))
                if lab[i]:
                    p = np.exp(ins[i] + out)
                    post[i] = p if (p == p and ins[i] > -np.inf and out > -np.inf) or variant == "no_guard" else dtype(0)
                    res.counts[lab[i]] += post[i]
                if not out > -np.inf and variant != "no_guard":
                    continue
                k = kids[i]
                if variant == "shared_once":
                    k = list(dict.fromkeys(k))
                if variant == "skip_first_or" and not lab[i]:
                    k = k[1:]
                for c in k:
                    if lab[i]:
                        if not ins[i] > -np.inf and variant != "no_guard":
                            continue  # the 0/0 guard: an AND parent of inside zero passes nothing on
                        t = out + ins[i]
                        mags.append(abs(float(t)))
                        t = t - ins[c]
                    else:
                        t = out
                    contrib[c].append(t)
                    Lout[c], Dpar[c], Cpar[c] = max(Lout.get(c, 0), lo), max(Dpar.get(c, 0), do), max(Cpar.get(c, 0), co)
            st.A = max([st.A] + [m for m in mags if m < np.inf])
    fin = np.asarray(lw, np.float64)
    fin = np.abs(fin[np.isfinite(fin)])
    st.A = max(st.A, float(fin.max()) if len(fin) else 0.0)
    st.N = int(res.slots.max())
    live = res.lnp > -np.inf
    res.avg = res.lnp[live].sum() / dtype(int(live.sum())) if live.any() else NEG
    res.tol = Tolerance(st)
    return res


def viterbi_ref(node_off, label, ref, nxt, logw, dtype=LD):
    """(the max-product ln value of every forest, its bound L_in A_v u)"""
    lw = np.asarray(logw, dtype)
    n_forests = len(node_off) - 1
    best = np.full(n_forests, -np.inf, dtype)
    lab_all, rf_all, nx_all = np.asarray(label).tolist(), np.asarray(ref).tolist(), np.asarray(nxt).tolist()
    L, A = 0, 0.0
    with np.errstate(all="ignore"):
        for f in range(n_forests):
            b, e = int(node_off[f]), int(node_off[f + 1])
            lab, rf, nx = lab_all[b:e], rf_all[b:e], nx_all[b:e]
            order, kids = _flatten(lab, rf, nx)
            val, Lin = {}, {}
            for i in order:
                k = kids[i]
                if lab[i]:
                    v = lw[lab[i]]
                    for c in k:
                        v = v + val[c]
                    Lin[i] = 1 + sum(Lin[c] for c in k)
                else:
                    v = max(val[c] for c in k)
                    Lin[i] = 1 + max(Lin[c] for c in k)
                val[i] = v
            best[f] = val[0]
            L = max(L, Lin[0])
            A = max([A] + [abs(float(v)) for v in val.values() if v > -np.inf])
    return best, L * A * U


def score(label, ref, nxt, deriv, logw, dtype=LD):
    """the ln weight of `deriv`, a pre-order list of (rule, number of children) as best_derivation returns it, parsed against
    ONE forest's arrays; None if the list is not a derivation of the forest or an arity is wrong; the best where more than one
    parse fits"""
    import sys
    sys.setrecursionlimit(max(20000, sys.getrecursionlimit()))
    lw = np.asarray(logw, dtype)
    lab, rf, nx = np.asarray(label).tolist(), np.asarray(ref).tolist(), np.asarray(nxt).tolist()
    deriv = [(int(r), int(a)) for r, a in deriv]

    def parse(i, pos):
        """{end position: best ln weight} of node i consuming deriv from pos"""
        while rf[i] >= 0:
            i = rf[i]
        kids = list(children(nx, i))
        out = {}
        if lab[i] == 0:
            for c in kids:
                for e, s in parse(c, pos).items():
                    if e not in out or out[e] < s:
                        out[e] = s
            return out
        if pos >= len(deriv) or deriv[pos] != (lab[i], len(kids)):
            return out
        ends = {pos + 1: lw[lab[i]]}
        for c in kids:
            nxt_ends = {}
            for e, s in ends.items():
                for e2, s2 in parse(c, e).items():
                    t = s + s2
                    if e2 not in nxt_ends or nxt_ends[e2] < t:
                        nxt_ends[e2] = t
            ends = nxt_ends
            if not ends:
                break
        return ends
    with np.errstate(all="ignore"):
        return parse(0, 0).get(len(deriv))


class MstepTolerance(object):
    def __init__(self, n, a_w, w_max):
        self.n, self.A_w, self.W = n, a_w, w_max
        self.lnw = (n + 4.0 + 2.0 * a_w) * U
        self.delta = w_max * (self.lnw + 5.0 * U)

    def __repr__(self):
        return "n=%d A_w=%.4g W=%.4g: ln weight %.3g, max change %.3g" % (self.n, self.A_w, self.W, self.lnw, self.delta)


def mstep_ref(counts, prior, group_off, group_rule, add_k, zero_zero, old_logw):
    """normalize.hpp:123-164 in longdouble: per group sum = the sum of count + prior; if it is positive every member becomes
    (count + prior) / (sum + add_k); else every member becomes 0 (zero_zero) or 1 / the group's size.  Rules outside every group
    keep their weight.  Returns (new ln weights, the largest |exp(new) - exp(old)| over the rules in groups, MstepTolerance)"""
    goff, grule = np.asarray(group_off, np.int64), np.asarray(group_rule, np.int64)
    sizes = np.diff(goff)
    assert (sizes > 0).all() and goff[-1] == len(grule)
    old = np.asarray(old_logw, LD)
    with np.errstate(all="ignore"):
        c = np.asarray(counts, LD)[grule] + LD(prior)
        sums = np.add.reduceat(c, goff[:-1])
        gid = np.repeat(np.arange(len(sizes)), sizes)
        live = (sums > 0)[gid]
        new = np.full(len(c), -np.inf, LD)
        pos = live & (c > 0)
        new[pos] = np.log(c[pos] / (sums + LD(add_k))[gid][pos])
        if not zero_zero:
            new[~live] = -np.log(sizes.astype(LD))[gid][~live]
        delta = np.abs(np.exp(new) - np.exp(old[grule])).max()
    out = old.copy()
    out[grule] = new
    fin = new[np.isfinite(new.astype(np.float64))]
    a_w = float(np.abs(fin).max()) if len(fin) else 0.0
    w_max = max(1.0, float(np.exp(old[grule]).max()), float(np.exp(new).max()))
    return out, delta, MstepTolerance(int(sizes.max()), a_w, w_max)


# ---------------------------------------------------------------------------------------------------------------------
# the layout, restated from carmel_hip_forests_create: groups of 64 by stream length, launch classes, the kernel of a class
# ---------------------------------------------------------------------------------------------------------------------
def estep_kind(max_nodes):
    """ext up to 100 nodes (24 B x 64 x n in LDS), log up to 150 (16 B x 64 x n), the global columns beyond"""
    if 24 * 64 * max_nodes <= LDS_BYTES:
        return "ext"
    return "log" if 16 * 64 * max_nodes <= LDS_BYTES else "gcol"


def layout(node_off, label, ref, nxt):
    """(nodes, classes): the non-reference nodes per forest, and [(first group, groups, max_nodes, kind)] per launch class --
    forests sorted by stream length (a record per non-reference node and per child), 64 to a group, a class ending after 256
    groups at the first group of at most 2/3 of its largest"""
    n_forests = len(node_off) - 1
    rf = np.asarray(ref)
    nonref = (rf < 0).astype(np.int64)
    cum = np.concatenate([[0], np.cumsum(nonref)])
    off = np.asarray(node_off, np.int64)
    nodes = cum[off[1:]] - cum[off[:-1]]
    # every node but a forest's root is the child of exactly one node, a child record each; a reference node has no header
    length = nodes + (np.diff(off) - 1)
    order = np.argsort(-length, kind="stable")
    gmax = [int(nodes[order[g:g + 64]].max()) for g in range(0, n_forests, 64)]
    classes, i = [], 0
    while i < len(gmax):
        mx, j = gmax[i], i + 1
        while j < len(gmax):
            mx = max(mx, gmax[j])
            if j - i >= CLASS_MIN_GROUPS and gmax[j] * CLASS_DEN <= mx * CLASS_NUM:
                break
            j += 1
        classes.append((i, j - i, mx, estep_kind(mx)))
        i = j
    return nodes, classes


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
BALLASTS = (100, 101, 150, 151)       # ext, log, log and gcol, each at its limit
BAL = list(range(1, 13))              # the ballast forest's rules, in three norm groups of four
ZERO_GROUP, SINGLE, NO_GROUP = [13, 14], 15, 16   # no forest uses these: an all-zero group of two, one of one, a rule in no group
E0 = 20                               # the edge forests' rules start here


def ballast(n_nodes, seed=0, rules=BAL):
    """a forest of exactly n_nodes non-reference nodes (and no reference): an OR over (rule rule rule) triples and leaves"""
    rng = np.random.default_rng(1000 + n_nodes + seed)
    m, extra = (n_nodes - 1) // 3, (n_nodes - 1) % 3
    kids = ["(%d %d %d)" % tuple(rng.choice(rules, 3)) for _ in range(m)] + ["%d" % rng.choice(rules) for _ in range(extra)]
    return "(OR %s)" % " ".join(kids)


def random_forest(rng, rules, depth):
    """a random AND/OR forest with shared sub-forests over `rules`, after test_forest_gpu.synth_forests"""
    nid, defined = [0], []

    def gen(d, top=False):
        r = rng.random()
        if not top and defined and r < 0.15:
            return "#%d" % rng.choice(defined)
        if d == 0 or (not top and r < 0.3):
            return str(rng.choice(rules))
        if r < 0.6 or top:
            body = "(OR %s)" % " ".join(gen(d - 1) for _ in range(rng.integers(2, 4)))
        else:
            body = "(%d %s)" % (rng.choice(rules), " ".join(gen(d - 1) for _ in range(rng.integers(1, 3))))
        if not top and rng.random() < 0.3:
            nid[0] += 1
            defined.append(nid[0])
            return "#%d%s" % (nid[0], body)
        return body
    return gen(depth, top=True)


def _groups_of(rules, rng, lo=2, hi=6):
    rules, out, i = list(rules), [], 0
    while i < len(rules):
        k = int(rng.integers(lo, hi))
        out.append(rules[i:i + k])
        i += k
    return out


class Case(object):
    """make() -> dict(forests = the edge forests' texts, groups = their norm groups, weights = {rule: ln weight} to override
    the random ones, expect = what the host test checks of the corpus); ballast: the corpus gets a ballast forest in front, of
    every size in BALLASTS (else it runs as it is: ballasts = (0,)); second: estimate -> maximize -> estimate; every: the
    derivations of every k-th forest are scored"""

    def __init__(self, name, make, with_ballast=True, second=False, every=1, seed=0):
        self.name, self.make, self.with_ballast, self.second, self.every, self.seed = name, make, with_ballast, second, every, seed
        self.ballasts = BALLASTS if with_ballast else (0,)
        self._built = {}

    def corpus(self, n_ballast):
        if n_ballast not in self._built:
            self._built[n_ballast] = Corpus(self, n_ballast)
        return self._built[n_ballast]


class Corpus(object):
    """the arrays (through the oracle's reader, as test_forest_gpu.make reads them), the ln weights, the oracle's handle"""

    def __init__(self, case, n_ballast):
        from oracle import binding
        d = case.make()
        self.case, self.n_ballast, self.expect = case, n_ballast, dict(d.get("expect", {}))
        forests = ([ballast(n_ballast)] if case.with_ballast else []) + list(d["forests"])
        groups = [BAL[0:4], BAL[4:8], BAL[8:12], ZERO_GROUP, [SINGLE]] + [list(g) for g in d["groups"]]
        self.ftext = "\n".join(forests) + "\n"
        self.ntext = "(" + " ".join("(" + " ".join(str(r) for r in g) + ")" for g in groups) + ")"
        self.of = of = binding.OracleForests(self.ftext, self.ntext)
        self.node_off, self.label, self.ref, self.next = of.node_off, of.label, of.ref, of.next
        self.n_rules, self.n_forests = max(of.n_rules, NO_GROUP + 1), of.n_forests
        self.group_off, self.group_rule = of.group_off, of.group_rule[:int(of.group_off[-1])]
        self.oracle_ok = self.n_rules == of.n_rules
        if "group_arrays" in d:  # norm groups too many for a text: built directly, and the oracle is left out of the M-step
            self.group_off, self.group_rule, self.n_rules = d["group_arrays"]
            self.oracle_ok = False
        lw = np.log(np.random.default_rng(77 + case.seed).uniform(0.05, 1.0, self.n_rules))
        for r, v in d.get("weights", {}).items():
            lw[r] = v
        self.logw = lw
        self.nodes, self.classes = layout(self.node_off, self.label, self.ref, self.next)
        self._ref = {}

    def arrays(self):
        return self.node_off, self.label, self.ref, self.next

    def forest(self, f):
        b, e = int(self.node_off[f]), int(self.node_off[f + 1])
        return self.label[b:e], self.ref[b:e], self.next[b:e]

    def reference(self, logw=None, dtype=LD, variant=None):
        """the reference run at the corpus's own weights is computed once and shared"""
        if logw is None and variant is None:
            if dtype not in self._ref:
                self._ref[dtype] = reference(*self.arrays(), self.logw, dtype)
            return self._ref[dtype]
        return reference(*self.arrays(), self.logw if logw is None else logw, dtype, variant)

    def oracle_forests(self, logw=None):
        self.of.set_weights(self.logw if logw is None else logw)
        return self.of


def _plain(n_total):
    def make():
        rng = np.random.default_rng(200 + n_total)
        rules = list(range(E0, E0 + 40))
        return dict(forests=[random_forest(rng, rules, 3) for _ in range(n_total - 1)], groups=_groups_of(rules[:-2], rng),
                    expect=dict(n_forests=n_total, last_group=(n_total - 1) % 64 + 1))
    return make


def _zero():
    rng = np.random.default_rng(301)
    Z1, Z2 = E0, E0 + 1
    a, b, c, d, e, f = range(E0 + 2, E0 + 8)
    rules = list(range(E0, E0 + 30))
    forests = ["(%d %d %d)" % (a, Z1, b),                                  # a whole forest dead
               "(OR (%d %d) (%d %d))" % (a, Z1, b, c),                     # an OR with one dead branch
               "(%d (OR %d %d) %d)" % (a, Z2, b, c),
               "(OR (%d (%d %d) %d) %d)" % (a, b, Z1, c, d),               # a dead AND beside a live sibling, under a live outside value
               "(OR (%d %d #1(OR %d %d)) (%d #1))" % (a, Z1, b, c, d),     # a shared sub-forest under a dead and under a live branch
               "(OR (%d #1(%d %d) %d) (%d #1 %d))" % (a, e, f, Z2, b, c),
               "(OR %d %d)" % (Z1, Z2),                                    # dead, an OR of dead leaves
               "%d" % Z1]                                                  # dead, a single leaf
    forests += [random_forest(rng, rules, 3) for _ in range(150)]
    return dict(forests=forests, groups=_groups_of(rules, rng), weights={Z1: -np.inf, Z2: -np.inf, E0 + 12: -np.inf, E0 + 20: -np.inf},
                expect=dict(min_zero=4))


SHARED_FORESTS = ["(%d #1(OR %d %d) #1)" % (E0, E0 + 1, E0 + 2),                                       # twice inside one AND
                  "(OR (%d #1(%d #2(OR %d %d) #2) #1) %d)" % (E0, E0 + 3, E0 + 1, E0 + 2, E0 + 4),     # a reference inside a referenced sub-forest
                  "(OR (%d (OR %d %d %d %d %d)) (%d #1(OR %d %d) #1))" % (E0, E0 + 3, E0 + 4, E0 + 5, E0 + 6, E0 + 7, E0 + 1, E0 + 3, E0 + 4),
                  "(%d #1(OR (%d %d) %d) #1 #2(%d #1) #2)" % (E0 + 2, E0 + 5, E0 + 6, E0 + 7, E0 + 3)]


def _shared():
    return dict(forests=SHARED_FORESTS, groups=[[E0, E0 + 1, E0 + 2], [E0 + 3, E0 + 4, E0 + 5, E0 + 6]])  # (E0 + 7: in no group)


DEEP = 40   # a spine whose later children wait on the Viterbi walk's stack: one more a level, past its 32 LDS entries
WIDE = (254, 255, 256, 300)   # the header's 8-bit child count saturates at 255: the Viterbi walk then counts the records
T1, T2, T3 = E0 + 30, E0 + 31, E0 + 32   # three rules of one weight: an OR over bit-identical sub-forests


def _wide(k, kind):
    """an OR / AND node of k children: two shared sub-forests and references to them in turn (k children, four more nodes)"""
    a, b, c, d, e = E0, E0 + 1, E0 + 2, E0 + 3, E0 + 4
    kids = ["#1(OR %d %d)" % (a, b), "#2(OR %d %d)" % (c, d)] + ["#%d" % (1 + j % 2) for j in range(k - 2)]
    return "(%s %s)" % ("OR" if kind == "or" else str(e), " ".join(kids))


def _shapes():
    rng = np.random.default_rng(302)
    rules = list(range(E0, E0 + 12))
    forests = ["%d" % (E0 + 5), "(OR %d)" % (E0 + 6), "(OR (%d %d))" % (E0 + 7, E0 + 8), "(%d (OR (OR %d)))" % (E0 + 9, E0 + 10),
               "(OR (%d %d) (%d %d) (%d %d))" % (T1, E0 + 5, T2, E0 + 5, T3, E0 + 5),
               "(OR (%d %d) (%d %d) (%d %d))" % (E0 + 6, T3, E0 + 6, T2, E0 + 6, T1)]
    deep = "(OR %d %d)" % (E0 + 7, E0 + 8)
    for _ in range(DEEP):
        deep = "(%d %s %d)" % (rng.choice(rules[5:]), deep, rng.choice(rules[5:]))
    forests.append(deep)
    forests += [_wide(k, kind) for k in WIDE for kind in ("or", "and")]
    forests += [random_forest(rng, rules, 2) for _ in range(20)] + ["%d" % rng.choice(rules) for _ in range(5)]
    # (the wide AND nodes multiply 300 values: the OR's two rules near 1/2 each keep them in range of every form)
    w = {E0: np.log(0.55), E0 + 1: np.log(0.4), E0 + 2: np.log(0.3), E0 + 3: np.log(0.65), T1: np.log(0.3), T2: np.log(0.3), T3: np.log(0.3)}
    return dict(forests=forests, groups=_groups_of(rules, rng) + [[T1, T2, T3]], weights=w, 
                expect=dict(first_best={4: [(T1, 1), (E0 + 5, 0)], 5: [(E0 + 6, 1), (T3, 0)]}, deep=6))


def _leaf_only(n_ballast=0):
    rng = np.random.default_rng(303)
    rules = list(range(E0, E0 + 9))
    return dict(forests=["%d" % rng.choice(rules) for _ in range(70)], groups=_groups_of(rules, rng),
                expect=dict(n_forests=70, max_nodes=1))


SPINE = (24, 40, 60)   # AND levels of weight about 1e-8: roots about 1e-190, 1e-320 and 1e-480


def _range():
    rng = np.random.default_rng(304)
    S = list(range(E0, E0 + 4))          # about 1e-8
    Wd = list(range(E0 + 4, E0 + 12))    # up to 4
    P, Q, X, Y, EQ = E0 + 12, E0 + 13, E0 + 14, E0 + 15, E0 + 16

    def spine(depth):
        t = "(OR %d %d)" % (X, Y)
        for _ in range(depth):
            t = "(%d %s)" % (rng.choice(S), t)
        return t
    forests = [spine(d) for d in SPINE]
    forests += [random_forest(rng, Wd, 3) for _ in range(40)]
    forests += ["(OR (%d %d) (%d %d))" % (P, X, Q, Y),                    # two derivations 1e-250 apart
                "(OR (%d #1(OR %d %d)) (%d #1))" % (P, X, Y, Q),          # ... and two uses of one sub-forest that far apart
                "(OR %s)" % " ".join([str(EQ)] * 70)]                     # a sum of 70 equal terms
    w = {r: np.log(1e-8) + np.log(rng.uniform(0.5, 1.5)) for r in S}
    w.update({r: np.log(rng.uniform(0.05, 4.0)) for r in Wd})
    w.update({P: np.log(1e-250), Q: np.log(0.5), EQ: np.log(1.0 / 70)})
    return dict(forests=forests, groups=[S, Wd[:4], Wd[4:], [P, Q], [X, Y]], weights=w,
                expect=dict(roots={0: -190, 1: -320, 2: -480}))  # (log10)


HOT = {E0: 64, E0 + 1: 65, E0 + 2: 4096, E0 + 3: 4097}


def _hot():
    rng = np.random.default_rng(305)
    pool = list(range(E0 + 4, E0 + 4 + 600))  # (600 rules over 16 644 leaves: about 28 slots each, all cold)
    forests = ["(%d %d %d)" % (h, rng.choice(pool), rng.choice(pool)) for h, k in HOT.items() for _ in range(k)]
    order = rng.permutation(len(forests))
    return dict(forests=[forests[i] for i in order], groups=[list(HOT)] + _groups_of(pool, rng, 3, 9), expect=dict(slots=HOT))


def _second():
    rng = np.random.default_rng(306)
    rules = list(range(E0, E0 + 40))
    return dict(forests=[random_forest(rng, rules, 3) for _ in range(120)], groups=_groups_of(rules[:-2], rng))


def _mstep():
    """groups of 1, 2 and 257 rules among the used ones (the all-zero groups, the group that is live only through the prior and
    the rules in no group are in every corpus: ZERO_GROUP, SINGLE, NO_GROUP)"""
    rng = np.random.default_rng(307)
    one, two, big = [E0], [E0 + 1, E0 + 2], list(range(E0 + 3, E0 + 3 + 257))
    rules = one + two + big[:40] + [E0 + 300, E0 + 301]  # (most of the large group has no count; the last two are in no group)
    return dict(forests=[random_forest(rng, rules, 3) for _ in range(100)], groups=[one, two, big])


TINY = 16385   # forests of three nodes: with four large ones 257 groups, the first 256 a class of their own


def _two_class(big_nodes):
    def make(n_ballast=0):
        rng = np.random.default_rng(308 + big_nodes)
        T, pool = E0, list(range(E0 + 1, E0 + 41))
        forests = ["(%d %d %d)" % (T, rng.choice(pool), rng.choice(pool)) for _ in range(TINY)]
        for k, at in enumerate((5, 4000, 9000, 16000)):  # (anywhere in the corpus: sorting by stream length puts them in group 0)
            forests.insert(at, ballast(big_nodes, seed=k))
        return dict(forests=forests, groups=[[T]] + _groups_of(pool, rng),
                    expect=dict(classes=[(0, 256, big_nodes, estep_kind(big_nodes)), (256, 1, 3, "ext")], slots={T: TINY}))
    return make


STRIDE_GROUPS = 4096 * 256 + 300   # singleton groups: the M-step's grid ends at 4096 x 256 threads, these take a second trip


def _stride(n_ballast=0):
    n_rules = STRIDE_GROUPS + 1
    hi = [n_rules - 1, n_rules - 2, n_rules - 150, 4096 * 256 + 1, 4096 * 256, 7]
    forests = ["(OR (%d %d) (%d %d) %d)" % (hi[0], hi[1], hi[2], hi[3], hi[4]), "(%d %d)" % (hi[5], hi[0])]
    goff, grule = np.arange(STRIDE_GROUPS + 1, dtype=np.uint64), np.arange(1, n_rules, dtype=np.uint32)
    return dict(forests=forests, groups=[], group_arrays=(goff, grule, n_rules), expect=dict(n_groups=STRIDE_GROUPS))


CASES = ([Case("plain-%d" % n, _plain(n), seed=n) for n in (1, 63, 64, 65)]
         + [Case("zero", _zero, seed=1), Case("shared", _shared, seed=2), Case("shapes", _shapes, seed=3),
            Case("range", _range, seed=4), Case("hot", _hot, seed=5), Case("second", _second, second=True, seed=6),
            Case("mstep", _mstep, seed=7),
            Case("leaf-only", _leaf_only, with_ballast=False, seed=8),
            Case("two-class-log", _two_class(120), with_ballast=False, every=257, seed=9),
            Case("two-class-gcol", _two_class(151), with_ballast=False, every=257, seed=10),
            Case("mstep-grid-stride", _stride, with_ballast=False, seed=11)])
NAMES = [c.name for c in CASES]
PARAMS = [(c.name, n) for c in CASES for n in c.ballasts]


def by_name(name):
    return CASES[NAMES.index(name)]
