"""A plain sequential product construction: the reference that csrc/compose.hip (carmel_hip_compose) is held to.

It takes the flat arrays of the C ABI -- per operand the CSR arrays off / in / out / dst / logw, the two symbol tables a2b and
b2a, the index threshold (carmel -T) -- and keeps no index structure: for every composite state the matching arcs are found by
scanning the other state's arc list, and then put in the emission order that the header comments of compose.hip and
host/compose.hpp state:

  composite state (qa, qb, f), na and nb arcs leaving qa and qb, big = max(na, nb), "A bigger" = na > nb (a tie goes to B):
    big > T and not A bigger  "B indexed": A's arcs in list order; per arc the matching arcs of B NEWEST FIRST (descending position)
    big > T and A bigger      "A indexed": B's arcs in list order; per arc the matching arcs of A newest first
    otherwise                 "scanned":   A's arcs in list order; per arc the matching arcs of B in LIST order
  where A is walked (B indexed, scanned), per arc a:x of A
    x = *e* (id 0):  a:*e* alone -> (qa', qb, 1) unless f = 2;  then, if f = 0, with every *e*:c of B -> (qa', qb', 0)
    otherwise:       with every a2b[x]:c of B -> (qa', qb', 0); no match where x >= n_a2b or a2b[x] = 0xffffffff
  and after A's arcs, unless f = 1, every *e*:c of B alone -> (qa, qb', 2), in the order B's matches come in;
  where B is walked (A indexed) the same with the sides exchanged: *e*:c of B alone first (unless f = 1), then with A's
  a:*e* arcs (if f = 0); after B's arcs, unless f = 2, A's a:*e* arcs alone, newest first.
  An arc's weight is logw_a + logw_b (one f64 addition), ka / kb the position of the operand arc WITHIN ITS STATE, 0xffffffff
  for the side that took no arc.

Composite states are discovered level by level (the device's frontier); the temporary ids the device hands out within a level
follow the order in which its atomics land, so everything here is keyed by the triple (qa, qb, f), never by an id.

compose() also gives an account of the run (Report): what the device must have gone through -- levels, frontier sizes, which of
the three code paths ran under which filter state, bucket lengths, failed symbol lookups, and where the hash table is rebuilt
(compose.hip: capacity 2^16 at the start; before a level is emitted, 2 * (n_states + level_arcs) > capacity makes a new table of
the next sufficient power of two, into which the n_states states known so far are reinserted) and how far the state arrays
grow (1024 entries, doubled until n_states + level_arcs fit).

renumber() applies what Composer::run_device does to the device's output: composite states numbered in the order a LIFO work
list discovers them, every state's arcs reversed at the end -- the composed transducer as the front end prints it.

MUTANTS names deliberate mistakes; compose(..., mutant=name) makes one.  tests/test_compose_ref_host.py shows that the corpus
(compose_cases.py) tells every one of them from the reference."""
import struct

C_NONE = 0xffffffff
PATHS = ("b_indexed", "a_indexed", "scanned")
MUTANTS = ("bucket_order", "big_ge_threshold", "tie_to_a", "a_alone_under_filter_2", "filter_after_both", "ka_from_operand_start")


class Flat(object):
    """one operand: CSR over states, arcs in list order.  Plain Python lists."""

    def __init__(self, off, inp, out, dst, logw):
        self.off, self.inp, self.out, self.dst, self.logw = list(off), list(inp), list(out), list(dst), list(logw)
        self.n_states = len(self.off) - 1
        assert self.off[0] == 0 and self.off[-1] == len(self.inp) == len(self.out) == len(self.dst) == len(self.logw)
        assert all(a <= b for a, b in zip(self.off, self.off[1:])) and all(0 <= d < self.n_states for d in self.dst)

    @classmethod
    def from_states(cls, states):
        """states: per state a list of (in, out, dst, logw)"""
        off, arcs = [0], []
        for st in states:
            arcs.extend(st)
            off.append(len(arcs))
        return cls(off, [a[0] for a in arcs], [a[1] for a in arcs], [a[2] for a in arcs], [float(a[3]) for a in arcs])

    def n_arcs(self, q):
        return self.off[q + 1] - self.off[q]


class Report(object):
    def __init__(self):
        self.level_sizes = []          # composite states per level
        self.level_arcs = []           # arcs per level
        self.paths = {(p, f): 0 for p in PATHS for f in range(3)}  # composite states by code path and filter state
        self.longest_bucket = 0        # the most matches one lookup returned
        self.none_lookups = {p: 0 for p in PATHS}   # by code path: lookups of a symbol whose table entry is 0xffffffff
        self.range_lookups = {p: 0 for p in PATHS}  # ... and of a symbol id at or beyond the table's length
        self.rebuilds = []             # (states reinserted, arcs emitted before the level, new table capacity)
        self.state_capacity = 1024     # of the device's state arrays at the end
        self.table_capacity = 1 << 16

    @property
    def levels(self):
        return len(self.level_sizes)

    @property
    def doublings(self):
        return (self.state_capacity // 1024).bit_length() - 1

    def timing_line(self):
        """the line carmel_hip_compose prints under the timing option"""
        return "timing: compose levels=%d max_frontier=%d rebuilds=%d reinserted=%s state_capacity=%d table_capacity=%d" % (
            self.levels, max(self.level_sizes), len(self.rebuilds), ",".join(str(r[0]) for r in self.rebuilds) or "-",
            self.state_capacity, self.table_capacity)


class Result(object):
    def __init__(self):
        self.arcs = {}    # triple -> [(in, out, destination triple, logw, ka, kb)] in emission order
        self.depth = {}   # triple -> BFS depth
        self.report = Report()

    @property
    def n_states(self):
        return len(self.arcs)

    @property
    def n_arcs(self):
        return sum(len(v) for v in self.arcs.values())


def bits(x):
    """the bit pattern of an f64: -0.0 is not 0.0, and a weight is compared exactly"""
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def expand(A, B, a2b, b2a, T, qa, qb, f, report=None, mutant=None):
    """the arcs leaving composite state (qa, qb, f), in emission order"""
    a0, b0 = A.off[qa], B.off[qb]
    na, nb = A.n_arcs(qa), B.n_arcs(qb)
    a_bigger = na >= nb if mutant == "tie_to_a" else na > nb
    big = na if a_bigger else nb
    indexed = big >= T if mutant == "big_ge_threshold" else big > T
    path = "scanned" if not indexed else "a_indexed" if a_bigger else "b_indexed"
    if report is not None:
        report.paths[(path, f)] += 1
    newest_first = indexed and mutant != "bucket_order"
    ka_base = a0 if mutant == "ka_from_operand_start" else 0
    out = []

    def matches(X, x0, nx, side, sym):
        """positions within the state of X's arcs whose join symbol is sym: a scan, then the order of the path"""
        found = [k for k in range(nx) if side[x0 + k] == sym]
        if report is not None:
            report.longest_bucket = max(report.longest_bucket, len(found))
        return found[::-1] if newest_first else found

    def translate(table, sym):
        if sym >= len(table):
            if report is not None:
                report.range_lookups[path] += 1
            return C_NONE
        if table[sym] == C_NONE and report is not None:
            report.none_lookups[path] += 1
        return table[sym]

    def both(ka, kb):
        out.append((A.inp[a0 + ka], B.out[b0 + kb], (A.dst[a0 + ka], B.dst[b0 + kb], f if mutant == "filter_after_both" else 0),
                    A.logw[a0 + ka] + B.logw[b0 + kb], ka + ka_base, kb))

    def a_alone(ka):
        out.append((A.inp[a0 + ka], 0, (A.dst[a0 + ka], qb, 1), A.logw[a0 + ka], ka + ka_base, C_NONE))

    def b_alone(kb):
        out.append((0, B.out[b0 + kb], (qa, B.dst[b0 + kb], 2), B.logw[b0 + kb], C_NONE, kb))

    if path != "a_indexed":
        for ka in range(na):
            o = A.out[a0 + ka]
            if o == 0:
                if f != 2 or mutant == "a_alone_under_filter_2":
                    a_alone(ka)
                if f == 0:
                    for kb in matches(B, b0, nb, B.inp, 0):
                        both(ka, kb)
            else:
                m = translate(a2b, o)
                if m != C_NONE:
                    for kb in matches(B, b0, nb, B.inp, m):
                        both(ka, kb)
        if f != 1:
            for kb in matches(B, b0, nb, B.inp, 0):
                b_alone(kb)
    else:
        for kb in range(nb):
            i = B.inp[b0 + kb]
            if i == 0:
                if f != 1:
                    b_alone(kb)
                if f == 0:
                    for ka in matches(A, a0, na, A.out, 0):
                        both(ka, kb)
            else:
                m = translate(b2a, i)
                if m != C_NONE:
                    for ka in matches(A, a0, na, A.out, m):
                        both(ka, kb)
        if f != 2 or mutant == "a_alone_under_filter_2":
            for ka in matches(A, a0, na, A.out, 0):
                a_alone(ka)
    return out


def compose(A, B, a2b, b2a, threshold, mutant=None):
    a2b, b2a = list(a2b), list(b2a)
    assert A.n_states and B.n_states
    R = Result()
    rep = R.report
    frontier = [(0, 0, 0)]
    R.depth[(0, 0, 0)] = 0
    n_states, n_arcs, depth = 1, 0, 0
    while frontier:
        nxt, level_arcs = [], 0
        for t in frontier:
            arcs = expand(A, B, a2b, b2a, threshold, t[0], t[1], t[2], rep, mutant)
            R.arcs[t] = arcs
            level_arcs += len(arcs)
            for a in arcs:
                if a[2] not in R.depth:
                    R.depth[a[2]] = depth + 1
                    nxt.append(a[2])
        rep.level_sizes.append(len(frontier))
        rep.level_arcs.append(level_arcs)
        # what the device does between the count pass and the emit pass of this level
        max_states = n_states + level_arcs
        while rep.state_capacity < max_states:
            rep.state_capacity *= 2
        if 2 * max_states > rep.table_capacity:
            while rep.table_capacity < 2 * max_states:
                rep.table_capacity *= 2
            rep.rebuilds.append((n_states, n_arcs, rep.table_capacity))
        n_states += len(nxt)
        n_arcs += level_arcs
        frontier = nxt
        depth += 1
    return R


def renumber(R, final=None):
    """Composer::run_device's pass over the device's output: state numbers from a LIFO work list (the start state is 0; a
    state popped from the list has its arcs walked in emission order, and every destination not seen before gets the next
    number and is pushed), then every state's arcs reversed.  Returns (states, number of every triple): states[n] is the list
    of (in, out, destination number, logw, ka, kb).  With final = (qa, qb) the locked *e*:*e* arcs that join several final
    states (one per filter state reached, in filter order, added before the reversal) are modelled too; the second value is
    then followed by the final state's number, None where no final state is reached."""
    num = {(0, 0, 0): 0}
    states = [[]]
    work = [(0, 0, 0)]
    while work:
        t = work.pop()
        cur = num[t]
        for (i, o, d, w, ka, kb) in R.arcs[t]:
            if d not in num:
                num[d] = len(states)
                states.append([])
                work.append(d)
            states[cur].append((i, o, num[d], w, ka, kb))
    fin = None
    if final is not None:
        found = [num[(final[0], final[1], f)] for f in range(3) if (final[0], final[1], f) in num]
        if len(found) == 1:
            fin = found[0]
        elif found:
            fin = len(states)
            states.append([])
            for s in found:
                states[s].append((0, 0, fin, 0.0, C_NONE, C_NONE))
    states = [st[::-1] for st in states]
    return (states, num) if final is None else (states, num, fin)
