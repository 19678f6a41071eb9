"""The corpus that holds csrc/compose.hip to compose_ref.py: each case the smallest shape that still reaches its edge, built
deterministically (a seed where anything is drawn).  What each case is FOR is written in Case.expect and asserted on the
reference's run report in tests/test_compose_ref_host.py, before any GPU run; tests/test_compose_abi_gpu.py then runs every
case through carmel_hip_compose.

    frontier-N        level 1 has exactly N states (N = 1, 255, 256, 257, 513: the edges of a 256-thread workgroup), state i of it
                      with i % 4 arcs, so a shifted level_off shows; all of them lead into ONE new state (many inserts of one key)
    into-one-300      300 states, two arcs each, that all discover the same destination triple
    rebuild           200 x 200 states, three arcs a state, 40 000 composite states over 399 levels of at most 200 states: the
                      hash table is rebuilt once with more than 30 000 states to reinsert, the state arrays double six times,
                      and the arcs emitted afterwards lead back into every earlier level
    sizes-T           T = 2, 3, 32: operand states of (T, T), (T+1, T), (T, T+1), (T+1, T+1), (T+1, T+2), (T+2, T+1), (0, T+1) and
                      (T+1, 0) arcs, each pair reached under filter state 0, 1 and 2; epsilons first, last, in the middle, as a
                      state's only arcs, and absent
    bucket-a / -b     a state of 1000 arcs on one join symbol (duplicates that differ in weight alone) in A / in B, indexed
                      (T = 32) and scanned (T = 1000); symbols that sort first and last in the state, buckets of one arc, symbols
                      absent between two present ones, below the first and above the last
    symtab-T          a2b a non-monotone permutation with entries 0xffffffff, symbol ids at and beyond n_a2b / n_b2a, under
                      T = 2 (both indexed paths) and T = 32 (scanned)
    no-arcs-a / -b    an operand with states and no arc at all (arrays of one unused element: valid pointers)
    state0-alone      a composition that is state 0 and nothing else
    chain-2000        2000 levels of one state
    weights           every pair of weights from a list across the exponent range, with -inf, -0.0 and denormals
    random-K          200 seeded pairs: 1 to 12 states, 0 to 40 arcs a state, 1 to 5 symbols, epsilon rate 0 to 0.6, T from
                      {0, 1, 2, 5, 32}"""
import math

import numpy as np

import compose_ref as cr

C_NONE = cr.C_NONE


class Case(object):
    def __init__(self, name, A, B, a2b, b2a, threshold, **expect):
        self.name, self.A, self.B, self.a2b, self.b2a, self.threshold, self.expect = name, A, B, list(a2b), list(b2a), threshold, expect
        self._ref = None

    def reference(self):
        """computed once a session and shared: nobody changes it"""
        if self._ref is None:
            self._ref = cr.compose(self.A, self.B, self.a2b, self.b2a, self.threshold)
        return self._ref

    def mutant(self, name):
        return cr.compose(self.A, self.B, self.a2b, self.b2a, self.threshold, mutant=name)

    def arrays(self):
        """the arguments of carmel_hip_compose after `device`: numpy arrays, never empty (an operand without arcs passes one
        unused element, as Composer::run_device does)"""
        def side(X):
            pad = (lambda v: v if v else [0])
            return [np.array(X.off, np.uint64), np.array(pad(X.inp), np.uint32), np.array(pad(X.out), np.uint32),
                    np.array(pad(X.dst), np.uint32), np.array(pad(X.logw), np.float64)]
        return side(self.A), side(self.B), np.array(self.a2b or [0], np.uint32), len(self.a2b), np.array(self.b2a or [0], np.uint32), len(self.b2a)

    def __repr__(self):
        return "Case(%s)" % self.name


def identity(n):
    return list(range(n))


def sym(i):
    return "*e*" if i == 0 else "s%d" % i


def to_text(X, final):
    """an operand in carmel's text format: numbered states, one arc a line, the weight as exp(logw) in full"""
    lines = [str(final)]
    for q in range(X.n_states):
        for k in range(X.off[q], X.off[q + 1]):
            lines.append("(%d (%d %s %s %s))" % (q, X.dst[k], sym(X.inp[k]), sym(X.out[k]), repr(math.exp(X.logw[k]))))
    return "\n".join(lines) + "\n"


# ---- frontier widths -------------------------------------------------------------------------------------------------------
def frontier(N, arcs_of=lambda i: i % 4, name=None):
    """A: 0 -k-> k for k = 1 .. N; state k has arcs_of(k) arcs on symbol 1 into N + 1, which has none.  B: 0 -k-> 1 for every k,
    1 -1-> 2.  Level 1 is {(k, 1, 0)}, N states of different arc counts; level 2 is (N + 1, 2, 0) alone."""
    A = [[(k, k, k, -0.5 * k) for k in range(1, N + 1)]]
    for k in range(1, N + 1):
        A.append([(100 + j, 1, N + 1, -0.25 * (j + 1) - k) for j in range(arcs_of(k))])
    A.append([])
    B = [[(k, 1000 + k, 1, -0.125 * k) for k in range(1, N + 1)], [(1, 7, 2, -3.0)], []]
    n_new = 1 if any(arcs_of(k) for k in range(1, N + 1)) else 0
    return Case(name or "frontier-%d" % N, cr.Flat.from_states(A), cr.Flat.from_states(B), identity(N + 1), identity(N + 1), 32,
                level_sizes=[1, N] + [1] * n_new, level1_arcs=sorted(arcs_of(k) for k in range(1, N + 1)))


# ---- a table rebuild with content ------------------------------------------------------------------------------------------
REBUILD_N = 200


def rebuild(n=REBUILD_N, seed=5):
    """Composite state (i, j), always under filter 0: symbol 1 steps A (i -> i + 1 mod n) while B loops, symbol 2 steps B while A
    loops -- the levels are the anti-diagonals i + j = d of an n x n torus, at most n states wide -- and symbol 3 sends both
    operands BACK, i -> a(i) <= i and j -> b(j) <= j, to a state of an earlier level (so the depths stay i + j).  a and b are drawn
    half of them a few states back and half with a bias towards state 0, so that the late levels, the ones expanded after the
    rebuild, reach back into every earlier level, the first ones and the ones just before the rebuild included.  Both operands are cycles (the steps wrap)."""
    rng = np.random.default_rng(seed)
    far = lambda i: int(i * rng.random() ** 3)                     # anywhere below, mostly far below
    near = lambda i: max(0, i - 1 - int(rng.integers(0, 12)))      # a few states below
    a = [far(i) if i % 2 else near(i) for i in range(n)]
    b = [near(j) if j % 2 else far(j) for j in range(n)]
    A = [[(1, 1, (i + 1) % n, -1.0), (2, 2, i, -0.5), (3, 3, a[i], -0.25 * (i % 7))] for i in range(n)]
    B = [[(1, 11, j, -2.0), (2, 12, (j + 1) % n, -0.125), (3, 13, b[j], -0.0625 * (j % 5))] for j in range(n)]
    return Case("rebuild", cr.Flat.from_states(A), cr.Flat.from_states(B), identity(4), identity(4), 32,
                n_states=n * n, levels=2 * n - 1, max_frontier=n, min_reinserted=30000, min_doublings=5)


# ---- the size comparisons at their edges -----------------------------------------------------------------------------------
EPS_PATTERNS = ("first", "last", "middle", "only", "absent")


def shape_arcs(n, pattern, sink, io, rng):
    """n arcs of a shape state: join symbols from {1, 2, 3}, epsilons (0) placed by the pattern; `io` puts the join symbol on the
    output side (A) or the input side (B).  Weights are distinct multiples of 1/8: duplicates are told apart."""
    syms = [1 + int(rng.integers(0, 3)) for _ in range(n)]
    if n:
        if pattern == "first":
            syms[0] = 0
        elif pattern == "last":
            syms[-1] = 0
        elif pattern == "middle" and n >= 3:
            syms[n // 2] = 0
            if n >= 5:
                syms[1] = 0
        elif pattern == "middle":
            syms[n - 1] = 0
        elif pattern == "only":
            syms = [0] * n
    arcs = []
    for k, s in enumerate(syms):
        other = 20 + k
        arcs.append(((other, s) if io == "out" else (s, other)) + (sink[k % len(sink)], -0.125 * (k + 1)))
    return arcs


def shapes_of(T):
    return [(T, T), (T + 1, T), (T, T + 1), (T + 1, T + 1), (T + 1, T + 2), (T + 2, T + 1), (0, T + 1), (T + 1, 0)]


def expected_path(na, nb, T):
    """the rule in words, apart from the reference's code: nothing is indexed unless the larger state has MORE than T arcs;
    A is indexed only where it has strictly more arcs than B"""
    if max(na, nb) <= T:
        return "scanned"
    return "a_indexed" if na > nb else "b_indexed"


def sizes(T, seed=11):
    """Per shape k and epsilon pattern: states P (entry), M (one epsilon arc into S) and S (the shape state) in each operand.
    (PA, PB, 0) is reached from (0, 0, 0) on a symbol of its own; from there symbol 1 leads to (SA, SB, 0), symbol 2 to
    (MA, SB, 0) whose a:*e* arc taken alone gives (SA, SB, 1), symbol 3 to (SA, MB, 0) whose *e*:c arc taken alone gives
    (SA, SB, 2).  The shape states' arcs lead into two sinks and back into state 0's successors."""
    rng = np.random.default_rng(seed + T)
    # states 1 and 2 of either operand are the sinks: a dead end, and a state with one arc into the dead end
    A, B = [[], [], [(9, 1, 1, -4.0)]], [[], [], [(1, 9, 1, -4.0)]]
    want = []
    entry = 4
    for (na, nb) in shapes_of(T):
        for pa, pb in zip(EPS_PATTERNS, EPS_PATTERNS[2:] + EPS_PATTERNS[:2]):
            PA, MA, SA = len(A), len(A) + 1, len(A) + 2
            PB, MB, SB = len(B), len(B) + 1, len(B) + 2
            A[0].append((entry, entry, PA, -1.0))
            B[0].append((entry, entry, PB, -1.0))
            entry += 1
            A += [[(31, 1, SA, -0.5), (32, 2, MA, -0.25), (33, 3, SA, -0.75)], [(34, 0, SA, -1.5)], shape_arcs(na, pa, (1, 2), "out", rng)]
            B += [[(1, 41, SB, -0.5), (2, 42, SB, -0.25), (3, 43, MB, -0.75)], [(0, 44, SB, -2.5)], shape_arcs(nb, pb, (1, 2), "in", rng)]
            want.append((SA, SB, na, nb))
    return Case("sizes-%d" % T, cr.Flat.from_states(A), cr.Flat.from_states(B), identity(entry), identity(entry), T, shapes=want)


# ---- buckets ----------------------------------------------------------------------------------------------------------------
BUCKET = 1000


def bucket(big_side, T):
    """The big state: one arc on symbol 1 (sorts first), 1000 on symbol 5 that differ in weight alone, one each on 3 and 7,
    one on 9 (sorts last) -- in file order 9, 3, the thousand, 7, 1, so list order and index order differ.  The other state asks
    for 5, 1, 9, 4 and 6 (absent between present ones), 0 (no epsilon there), 10 (above the last), 5 again, 3, 7."""
    big = [(9, -9.0), (3, -3.0)] + [(5, -0.0078125 * k) for k in range(BUCKET)] + [(7, -7.0), (1, -1.0)]
    small = [(5, -0.5), (1, -0.25), (9, -0.125), (4, -4.0), (6, -6.0), (0, -10.0), (10, -11.0), (5, -1.5), (3, -2.5), (7, -3.5), (2, -4.5)]
    if big_side == "a":
        A = [[(1, 1, 1, 0.0)], [(50 + k % 3, s, 2, w) for k, (s, w) in enumerate(big)], []]
        B = [[(1, 1, 1, 0.0)], [(s, 60 + k, 2, w) for k, (s, w) in enumerate(small)], []]
    else:
        A = [[(1, 1, 1, 0.0)], [(60 + k, s, 2, w) for k, (s, w) in enumerate(small)], []]
        B = [[(1, 1, 1, 0.0)], [(s, 50 + k % 3, 2, w) for k, (s, w) in enumerate(big)], []]
    path = "scanned" if T >= BUCKET + 4 else big_side + "_indexed"
    return Case("bucket-%s-%s" % (big_side, "scanned" if path == "scanned" else "indexed"), cr.Flat.from_states(A), cr.Flat.from_states(B),
                identity(11), identity(11), T, path=path, longest_bucket=BUCKET, n_arcs=1 + 2 * BUCKET + 4 + 1)


# ---- symbol tables ---------------------------------------------------------------------------------------------------------
A2B = [0, 4, 2, 6, 1, C_NONE, 3]   # A's output ids 0 .. 6; 7 and 8 are used by A's arcs and lie beyond the table
B2A = [0, 4, 2, 6, 1, C_NONE, 3]   # its inverse (B's input id 5 has no partner either); B's arcs use 7 and 8 as well


def symtab(T, seed=3):
    """A of states with 9, 9, 4, 4 and 0 arcs, B with 9, 4, 9, 4 and 2 -- under T = 2 nine arcs against four is A indexed, four
    against nine and the ties B indexed -- on a permutation that turns the order of A's ids round in B."""
    assert all(B2A[A2B[x]] == x for x in range(7) if A2B[x] != C_NONE)
    rng = np.random.default_rng(seed)
    na, nb = [9, 9, 4, 4, 0], [9, 4, 9, 4, 2]

    def state(q, n, io):
        """n arcs: the id without a partner (5) and one beyond the table (7) wherever there is room, the rest drawn; arc k of
        state q leads to state (q + k) % 5, so every pair of states is met"""
        syms = ([5, 7] if n >= 3 else []) + [int(x) for x in rng.permutation([1, 2, 3, 4, 6, 8])]
        syms = (syms + [int(rng.integers(0, 7)) for _ in range(n)])[:n]
        syms = [syms[k] for k in rng.permutation(n)]
        return [((30 + k, s) if io == "out" else (s, 40 + k)) + ((q + k) % 5, -0.25 * k) for k, s in enumerate(syms)]
    A = [state(q, n, "out") for q, n in enumerate(na)]
    B = [state(q, n, "in") for q, n in enumerate(nb)]
    return Case("symtab-%d" % T, cr.Flat.from_states(A), cr.Flat.from_states(B), A2B, B2A, T,
                lookups=("scanned",) if T >= 9 else ("a_indexed", "b_indexed"))


# ---- degenerate operands ---------------------------------------------------------------------------------------------------
def degenerate():
    none3 = cr.Flat.from_states([[], [], []])
    eps_b = cr.Flat.from_states([[(0, 5, 1, -1.0), (1, 6, 2, -2.0)], [(0, 7, 2, -0.5), (0, 8, 0, -0.25)], []])
    eps_a = cr.Flat.from_states([[(5, 0, 1, -1.0), (6, 1, 2, -2.0)], [(7, 0, 2, -0.5), (8, 0, 0, -0.25)], []])
    apart_a = cr.Flat.from_states([[(1, 1, 1, -1.0), (2, 2, 0, -1.0)], [(1, 1, 0, -1.0)]])
    apart_b = cr.Flat.from_states([[(3, 1, 1, -1.0), (4, 2, 0, -1.0)], [(3, 1, 0, -1.0)]])
    L = 2000
    chain = cr.Flat.from_states([[(1, 1, i + 1, -1.0)] for i in range(L - 1)] + [[]])
    loop = cr.Flat.from_states([[(1, 2, 0, -0.5)]])
    return [Case("no-arcs-a", none3, eps_b, identity(2), identity(2), 32, n_states=4),   # (0,0,0) -> (0,1,2) -> (0,2,2), (0,0,2)
            Case("no-arcs-b", eps_a, none3, identity(2), identity(2), 2, n_states=4),
            Case("no-arcs-both", none3, none3, identity(2), identity(2), 0, n_states=1, n_arcs=0),
            Case("state0-alone", apart_a, apart_b, identity(5), identity(5), 1, n_states=1, n_arcs=0),  # B's input 3, 4 never leave A
            Case("chain-2000", chain, loop, identity(2), identity(2), 32, levels=L, max_frontier=1)]


# ---- weights ---------------------------------------------------------------------------------------------------------------
WEIGHTS = [0.0, -0.0, -1.0, -1e-300, -5e-324, -2.2250738585072014e-308, -1e300, -1.7976931348623157e308, float("-inf"), 1e300,
           1.7976931348623157e308, 2.0 ** -1074, -0.1, -744.4400719213812, 709.782712893384]


def weights():
    """every pair from WEIGHTS, one f64 addition each: sums that are exact, that round, that underflow to a denormal, that overflow to
    an infinity, -inf on one side and on both, -0.0 + -0.0 = -0.0 and -0.0 + 0.0 = 0.0.  No +inf on the way in, so no NaN."""
    A = [[(1, 1, 1, 0.0)], [(10 + k, 1, 2, w) for k, w in enumerate(WEIGHTS)], []]
    B = [[(1, 1, 1, -0.0)], [(1, 10 + k, 2, w) for k, w in enumerate(WEIGHTS)], []]
    return Case("weights", cr.Flat.from_states(A), cr.Flat.from_states(B), identity(2), identity(2), 5, n_arcs=1 + len(WEIGHTS) ** 2)


# ---- random ----------------------------------------------------------------------------------------------------------------
N_RANDOM = 200


def random_operand(rng, n_states, max_arcs, n_sym, p_eps, io, weights=None, p_empty=0.2):
    states = []
    for _ in range(n_states):
        n = int(rng.integers(0, max_arcs + 1)) if rng.random() >= p_empty else 0
        st = []
        for _ in range(n):
            join = 0 if rng.random() < p_eps else int(rng.integers(1, n_sym + 1))
            other = 0 if rng.random() < p_eps else int(rng.integers(1, n_sym + 1))
            w = float(rng.choice(weights)) if weights is not None else -float(rng.integers(0, 64)) / 8
            st.append(((other, join) if io == "out" else (join, other)) + (int(rng.integers(0, n_states)), w))
        states.append(st)
    return cr.Flat.from_states(states)


def random_case(seed):
    rng = np.random.default_rng(1000 + seed)
    n_sym = int(rng.integers(1, 6))
    p_eps = float(rng.choice([0.0, 0.1, 0.3, 0.6]))
    max_arcs = int(rng.choice([2, 5, 12, 40]))
    A = random_operand(rng, int(rng.integers(1, 13)), max_arcs, n_sym, p_eps, "out")
    B = random_operand(rng, int(rng.integers(1, 13)), max_arcs, n_sym, p_eps, "in")
    perm = [0] + [int(x) + 1 for x in rng.permutation(n_sym)]
    inv = [0] * (n_sym + 1)
    for x, y in enumerate(perm):
        inv[y] = x
    return Case("random-%d" % seed, A, B, perm, inv, int(rng.choice([0, 1, 2, 5, 32])))


_CASES = None


def cases():
    """every case but the random ones, built once"""
    global _CASES
    if _CASES is None:
        _CASES = ([frontier(N) for N in (1, 255, 256, 257, 513)] + [frontier(300, lambda i: 2, "into-one-300"), rebuild()] +
                  [sizes(T) for T in (2, 3, 32)] +
                  [bucket("a", 32), bucket("b", 32), bucket("a", BUCKET + 4), bucket("b", BUCKET + 4)] + [symtab(2), symtab(32)] +
                  degenerate() + [weights()])
    return _CASES


_RANDOM = None


def random_cases():
    global _RANDOM
    if _RANDOM is None:
        _RANDOM = [random_case(s) for s in range(N_RANDOM)]
    return _RANDOM


def by_name(name):
    return next(c for c in cases() if c.name == name)


NAMES = ["frontier-1", "frontier-255", "frontier-256", "frontier-257", "frontier-513", "into-one-300", "rebuild", "sizes-2", "sizes-3",
         "sizes-32", "bucket-a-indexed", "bucket-b-indexed", "bucket-a-scanned", "bucket-b-scanned", "symtab-2", "symtab-32", "no-arcs-a",
         "no-arcs-b", "no-arcs-both", "state0-alone", "chain-2000", "weights"]
