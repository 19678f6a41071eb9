"""CPU: the reference of the device composition (compose_ref.py) and its corpus (compose_cases.py), held before any GPU run.

  * Anchor.  The host composer (csrc/host/compose.hpp, Composer::run) is held to the oracle elsewhere; here the reference, after
    renumber() -- run_device's LIFO numbering and arc reversal --, must give the front end's host composition arc for arc and in
    order, for 60 random operand pairs at -T 2 and -T 32.  Twice: `carmel -HJ -q -d` prints the composition as composed (every
    state, dead ends included), and `carmel -HJ -q` prints it reduced, with a reduced first operand -- the reduction
    (Transducer::prune_useless) is restated in prune() below.  The *e*:*e* arcs that join several final states are MODELLED
    (renumber(final=...)), not left aside.  At -T 32 the oracle's composition must be the same arcs once more.
  * Intended properties.  Every case of the corpus reaches the edge it was built for, by the reference's run report.
  * Mutants.  Six deliberate mistakes in the reference; for each at least one case of the corpus gives another result."""
import math
import os
import subprocess

import numpy as np
import pytest

import compose_cases as cc
import compose_ref as cr
from conftest import ROOT

CLI = os.path.join(ROOT, "carmel_amd", "bin", "carmel")
LN2 = math.log(2.0)
N_ANCHOR = 60


sym, to_text = cc.sym, cc.to_text


def parse(text):
    """(final, {state: [(in, out, dest, weight)]}) of a composition printed with -HJ"""
    lines = [l for l in text.split("\n") if l.strip()]
    arcs = {}
    for l in lines[1:]:
        t = l.replace("(", " ").replace(")", " ").split()
        assert len(t) in (4, 5), l
        arcs.setdefault(int(t[0]), []).append((t[2], t[3], int(t[1]), float(t[4].rstrip("!")) if len(t) == 5 else 1.0))  # (a joining arc is locked: 1!)
    return int(lines[0]), arcs


def prune(states, final):
    """Transducer::prune_useless: keep the states on a path from state 0 to the final state, in order; drop *e*:*e* self loops.
    states[s] = [(in, out, dest, ...)].  None where nothing is left."""
    n = len(states)
    rev = [[] for _ in range(n)]
    for s in range(n):
        for a in states[s]:
            rev[a[2]].append(s)

    def reach(start, step):
        seen, work = {start}, [start]
        while work:
            for d in step(work.pop()):
                if d not in seen:
                    seen.add(d)
                    work.append(d)
        return seen
    f, b = reach(0, lambda s: [a[2] for a in states[s]]), reach(final, lambda s: rev[s])
    if final not in f or 0 not in b:
        return None
    keep = [s for s in range(n) if s in f and s in b]
    remap = {s: k for k, s in enumerate(keep)}
    out = []
    for s in keep:
        out.append([a[:2] + (remap[a[2]],) + a[3:] for a in states[s]
                    if a[2] in remap and not (a[0] == 0 and a[1] == 0 and remap[a[2]] == remap[s])])
    return out, remap[final]


def as_printed(states):
    return {s: [(sym(a[0]), sym(a[1]), a[2], 2.0 ** round(a[3] / LN2)) for a in st] for s, st in enumerate(states) if st}


def anchor_pair(seed):
    rng = np.random.default_rng(77 + seed)
    n_sym = int(rng.integers(2, 4))
    w = [0.0, math.log(0.5), math.log(0.25), math.log(0.125)]
    p_eps = float(rng.uniform(0, 0.5))
    for _ in range(100):  # (the last state is the final one and must be named by an arc, or the loader does not know it)
        A = cc.random_operand(rng, int(rng.integers(2, 7)), 5, n_sym, p_eps, "out", w, p_empty=0.05)
        B = cc.random_operand(rng, int(rng.integers(2, 7)), 5, n_sym, p_eps, "in", w, p_empty=0.05)
        if all(X.n_arcs(X.n_states - 1) or (X.n_states - 1) in X.dst for X in (A, B)) and A.n_arcs(0) and B.n_arcs(0):
            return A, B, n_sym
    raise AssertionError("no operand pair drawn")


def states_of(X):
    return [[(X.inp[k], X.out[k], X.dst[k], X.logw[k]) for k in range(X.off[q], X.off[q + 1])] for q in range(X.n_states)]


def carmel(args):
    p = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    return p.returncode, p.stdout, p.stderr


def test_reference_is_the_host_composition(oracle, tmp_path):
    compared = {"as composed": 0, "reduced": 0, "oracle": 0, "empty": 0}
    for seed in range(4 * N_ANCHOR):
        if compared["as composed"] >= 2 * N_ANCHOR:  # N_ANCHOR pairs whose composition reaches a final state, at both thresholds
            break
        A, B, n_sym = anchor_pair(seed)
        fa, fb = A.n_states - 1, B.n_states - 1
        ta, tb = to_text(A, fa), to_text(B, fb)
        pa, pb = str(tmp_path / "a.fst"), str(tmp_path / "b.fst")
        open(pa, "w").write(ta)
        open(pb, "w").write(tb)
        ident = cc.identity(n_sym + 1)
        if cr.renumber(cr.compose(A, B, ident, ident, 32), final=(fa, fb))[2] is None:
            if compared["empty"] >= 20:  # compositions that reach no final state: the first ten pairs show that the front end agrees
                continue
        for T in (2, 32):
            # as composed: -d keeps the operands and the result as they are
            states, num, fin = cr.renumber(cr.compose(A, B, ident, ident, T), final=(fa, fb))
            rc, out, err = carmel(["-HJ", "-q", "-d", "-T", str(T), pa, pb])
            assert (rc == 0) == (fin is not None), (seed, T, err)
            if rc == 0:
                got_fin, got = parse(out)
                assert got_fin == fin and got == as_printed(states), (seed, T)
                compared["as composed"] += 1
            else:
                compared["empty"] += 1
            # reduced: carmel -HJ -q -T t a b reduces its first operand, composes, reduces the result
            rc, out, err = carmel(["-HJ", "-q", "-T", str(T), pa, pb])
            pr = prune(states_of(A), fa)
            want = None
            if pr is not None:
                A2 = cr.Flat.from_states(pr[0])
                states, num, fin = cr.renumber(cr.compose(A2, B, ident, ident, T), final=(pr[1], fb))
                want = prune(states, fin) if fin is not None else None
            assert (rc == 0) == (want is not None), (seed, T, err)
            if rc == 0:
                got_fin, got = parse(out)
                assert got_fin == want[1] and got == as_printed(want[0]), (seed, T)
                compared["reduced"] += 1
                if T == 32:
                    o_fin, o_arcs = parse(oracle.OracleCascade([ta, tb], remember=False).composed().write(full=True, onearc=True))
                    assert o_fin == want[1] and o_arcs == as_printed(want[0]), (seed, T)
                    compared["oracle"] += 1
    print("anchor: compared", compared)
    assert compared["as composed"] == compared["reduced"] == 2 * N_ANCHOR and compared["oracle"] == N_ANCHOR


def test_renumbering_by_hand():
    """0 -> x, y; x -> w; y -> z, x: numbers are given at discovery (x 1, y 2), but the work list is LIFO: y is popped before x,
    so z is 3 and w is 4 (a queue would give w 3).  Arcs come out reversed."""
    R = cr.Result()
    s0, x, y, z, w = (0, 0, 0), (1, 1, 0), (2, 2, 0), (3, 3, 0), (4, 4, 1)
    R.arcs = {s0: [(1, 1, x, -1.0, 0, 0), (2, 2, y, -2.0, 1, 1)], x: [(3, 3, w, -3.0, 0, cr.C_NONE)],
              y: [(4, 4, z, -4.0, 0, 0), (5, 5, x, -5.0, 1, 1)], z: [], w: []}
    states, num = cr.renumber(R)
    assert num == {s0: 0, x: 1, y: 2, z: 3, w: 4}
    assert states == [[(2, 2, 2, -2.0, 1, 1), (1, 1, 1, -1.0, 0, 0)], [(3, 3, 4, -3.0, 0, cr.C_NONE)],
                      [(5, 5, 1, -5.0, 1, 1), (4, 4, 3, -4.0, 0, 0)], [], []]
    assert cr.renumber(R, final=(3, 3))[2] == 3 and cr.renumber(R, final=(4, 4))[2] == 4 and cr.renumber(R, final=(9, 9))[2] is None
    R.arcs[z] = [(0, 7, (3, 3, 2), -1.0, cr.C_NONE, 0)]
    R.arcs[(3, 3, 2)] = []
    states, num, fin = cr.renumber(R, final=(3, 3))  # two final states: a new one, joined by locked *e*:*e* arcs
    assert fin == 6 and states[3][0] == (0, 0, 6, 0.0, cr.C_NONE, cr.C_NONE) and states[num[(3, 3, 2)]] == [(0, 0, 6, 0.0, cr.C_NONE, cr.C_NONE)]


# ---- the corpus reaches what it was built for ------------------------------------------------------------------------------
def test_case_names():
    assert [c.name for c in cc.cases()] == cc.NAMES and len(cc.random_cases()) == cc.N_RANDOM


@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_frontier_cases(N):
    c = cc.by_name("frontier-%d" % N)
    R = c.reference()
    assert R.report.level_sizes == c.expect["level_sizes"] and R.report.level_sizes[1] == N
    level1 = [t for t, d in R.depth.items() if d == 1]
    assert sorted(len(R.arcs[t]) for t in level1) == c.expect["level1_arcs"]
    if N >= 4:
        assert {len(R.arcs[t]) for t in level1} == {0, 1, 2, 3}
        assert len({a[2] for t in level1 for a in R.arcs[t]}) == 1  # one new state, found by every thread of the level at once


def test_into_one_case():
    R = cc.by_name("into-one-300").reference()
    level1 = [t for t, d in R.depth.items() if d == 1]
    assert len(level1) == 300 and {a[2] for t in level1 for a in R.arcs[t]} == {(301, 2, 0)} and R.depth[(301, 2, 0)] == 2


def test_rebuild_case():
    c = cc.by_name("rebuild")
    R = c.reference()
    rep = R.report
    assert R.n_states == c.expect["n_states"] > 33000 and rep.levels == c.expect["levels"]
    assert max(rep.level_sizes) == c.expect["max_frontier"] <= 256  # many narrow levels
    assert len(rep.rebuilds) >= 1 and max(r[0] for r in rep.rebuilds) >= c.expect["min_reinserted"]
    assert rep.doublings >= c.expect["min_doublings"] and rep.state_capacity >= 1024 << 5
    # after the (last) rebuild, arcs lead back into states of EVERY earlier level
    n_at = rep.rebuilds[-1][0]
    level_at = next(d for d in range(rep.levels) if sum(rep.level_sizes[:d + 1]) >= n_at)  # the level being emitted at the rebuild
    hit = {R.depth[a[2]] for t, arcs in R.arcs.items() if R.depth[t] >= level_at for a in arcs}
    assert set(range(level_at)) <= hit, sorted(set(range(level_at)) - hit)
    # ... through cycles in both operands: the steps that wrap are among them
    n = cc.REBUILD_N
    assert any(t[0] == n - 1 and a[2][0] == 0 for t, arcs in R.arcs.items() if R.depth[t] >= level_at for a in arcs)
    assert any(t[1] == n - 1 and a[2][1] == 0 for t, arcs in R.arcs.items() if R.depth[t] >= level_at for a in arcs)
    print("rebuild case:", rep.timing_line(), "| rebuilds (states, arcs before, capacity):", rep.rebuilds)


@pytest.mark.parametrize("T", [2, 3, 32])
def test_size_cases(T):
    c = cc.by_name("sizes-%d" % T)
    R = c.reference()
    assert len(c.expect["shapes"]) == 8 * len(cc.EPS_PATTERNS)
    seen = set()
    for (sa, sb, na, nb) in c.expect["shapes"]:
        assert (c.A.n_arcs(sa), c.B.n_arcs(sb)) == (na, nb)
        for f in range(3):
            assert (sa, sb, f) in R.arcs, (na, nb, f)  # every shape under every filter state
        seen.add((na, nb))
        # the path the state takes, recomputed apart from the reference: an indexed walk shows in the order of the duplicates
        path = cc.expected_path(na, nb, T)
        arcs = R.arcs[(sa, sb, 0)]
        ka, kb = [a[4] for a in arcs if a[5] != cr.C_NONE and a[4] != cr.C_NONE], [a[5] for a in arcs if a[5] != cr.C_NONE and a[4] != cr.C_NONE]
        if path == "a_indexed":
            assert kb == sorted(kb)  # B walked in list order
        else:
            assert ka == sorted(ka)  # A walked in list order
    assert seen == set(cc.shapes_of(T))
    assert all(R.report.paths[(p, f)] > 0 for p in cr.PATHS for f in range(3)), R.report.paths
    # epsilons first, last, in the middle, the only arcs, absent -- on A's output side and on B's input side
    for X, side, col in ((c.A, c.A.out, 0), (c.B, c.B.inp, 1)):
        pats = set()
        for shape in c.expect["shapes"]:
            q = shape[col]
            s = side[X.off[q]:X.off[q + 1]]
            if len(s) >= 2:
                pats.add("only" if not any(s) else "absent" if all(s) else
                         "first" if s[0] == 0 and all(s[1:]) else "last" if s[-1] == 0 and all(s[:-1]) else "middle" if s[0] and s[-1] else "mixed")
        assert {"only", "absent", "first", "last"} <= pats and (T < 3 or "middle" in pats), pats


@pytest.mark.parametrize("name", ["bucket-a-indexed", "bucket-b-indexed", "bucket-a-scanned", "bucket-b-scanned"])
def test_bucket_cases(name):
    c = cc.by_name(name)
    R = c.reference()
    path = c.expect["path"]
    assert sum(v for (p, f), v in R.report.paths.items() if p == path) >= 1
    assert R.n_arcs == c.expect["n_arcs"]
    big = (1, 1, 0)
    arcs = R.arcs[big]
    assert max(c.A.n_arcs(1), c.B.n_arcs(1)) == cc.BUCKET + 4
    side = 4 if name.startswith("bucket-a") else 5   # ka or kb: the position in the big state
    # the thousand duplicates come once per asking arc (symbol 5 is asked for twice), in one run each
    runs = [[a[side] for a in arcs if a[5 if side == 4 else 4] == k and 2 <= a[side] < 2 + cc.BUCKET] for k in (0, 7)]
    for run in runs:
        assert len(run) == cc.BUCKET
        if path == "scanned":
            assert run == sorted(run)  # list order
        else:
            assert run == sorted(run, reverse=True)  # newest first
    if name != "bucket-a-scanned":  # (scanned with A the big state: A is walked, the buckets are B's, of two arcs)
        assert R.report.longest_bucket == cc.BUCKET
    # symbols that sort first (1) and last (9) in the big state are found, 4, 6, 10 and 2 are not
    other = 5 if side == 4 else 4
    asked = {a[other] for a in arcs if a[side] != cr.C_NONE}
    assert asked == {0, 1, 2, 7, 8, 9}, asked  # positions in the small state of the arcs on 5, 1, 9, 5, 3, 7


@pytest.mark.parametrize("T", [2, 32])
def test_symbol_table_cases(T):
    c = cc.by_name("symtab-%d" % T)
    rep = c.reference().report
    for p in c.expect["lookups"]:
        assert rep.none_lookups[p] > 0 and rep.range_lookups[p] > 0, (p, rep.none_lookups, rep.range_lookups)
        assert sum(rep.paths[(p, f)] for f in range(3)) > 0
    mapped = [x for x in c.a2b[1:] if x != cr.C_NONE]
    assert mapped != sorted(mapped) and cr.C_NONE in c.a2b and cr.C_NONE in c.b2a
    assert max(c.A.out) >= len(c.a2b) and max(c.B.inp) >= len(c.b2a)
    assert c.reference().n_arcs > 20


def test_degenerate_and_weight_cases():
    for name in ("no-arcs-a", "no-arcs-b", "no-arcs-both", "state0-alone", "chain-2000", "weights"):
        c = cc.by_name(name)
        R = c.reference()
        for key, want in c.expect.items():
            got = {"n_states": R.n_states, "n_arcs": R.n_arcs, "levels": R.report.levels, "max_frontier": max(R.report.level_sizes)}[key]
            assert got == want, (name, key, got, want)
    assert cc.by_name("no-arcs-a").A.off == [0, 0, 0, 0] and cc.by_name("no-arcs-b").B.off == [0, 0, 0, 0]
    assert all(len(v) for side in cc.by_name("no-arcs-both").arrays()[:2] for v in side)  # valid pointers all the same
    R = cc.by_name("state0-alone").reference()
    assert list(R.arcs) == [(0, 0, 0)]
    dead = [t for t, arcs in cc.by_name("sizes-2").reference().arcs.items() if not arcs]
    assert dead  # dead-end states
    W = [a[3] for a in cc.by_name("weights").reference().arcs[(1, 1, 0)]]
    assert not any(math.isnan(w) for w in W)
    pats = {cr.bits(w) for w in W}
    assert {cr.bits(0.0), cr.bits(-0.0), cr.bits(float("-inf")), cr.bits(float("inf"))} <= pats
    assert any(w != 0 and abs(w) < 2.2250738585072014e-308 for w in W)  # a denormal sum


def test_random_cases_spread():
    cs = cc.random_cases()
    assert {c.threshold for c in cs} == {0, 1, 2, 5, 32}
    assert min(c.A.n_states for c in cs) == 1 and max(c.A.n_states for c in cs) == 12
    assert max(max(c.A.n_arcs(q) for q in range(c.A.n_states)) for c in cs) >= 35
    tot = {k: 0 for k in cr.Report().paths}
    for c in cs:
        for k, v in c.reference().report.paths.items():
            tot[k] += v
    assert all(v > 0 for v in tot.values()), tot
    assert sum(1 for c in cs if c.reference().n_states == 1) >= 1 and max(c.reference().n_states for c in cs) > 100


# ---- mutants ---------------------------------------------------------------------------------------------------------------
def same(R, M):
    if set(R.arcs) != set(M.arcs):
        return False
    return all([a[:3] + (cr.bits(a[3]),) + a[4:] for a in R.arcs[t]] == [a[:3] + (cr.bits(a[3]),) + a[4:] for a in M.arcs[t]] for t in R.arcs)


@pytest.mark.parametrize("mutant", cr.MUTANTS)
def test_the_corpus_tells_the_mutant_apart(mutant):
    small = [c for c in cc.cases() if c.name not in ("rebuild", "chain-2000")]
    told = [c.name for c in small if not same(c.reference(), c.mutant(mutant))]
    told_random = sum(1 for c in cc.random_cases() if not same(c.reference(), c.mutant(mutant)))
    print("mutant %-24s told apart by %s and %d of the %d random cases" % (mutant, told, told_random, cc.N_RANDOM))
    assert told, "no built case tells %s from the reference: the corpus has a hole" % mutant
    assert told_random
