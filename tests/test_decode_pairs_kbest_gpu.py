"""GPU: batch pair k-best alignments (carmel_hip_decode_pairs_kbest, csrc/decode_pairs_kbest.hip) against the path-carrying
reference of decode_pairs_kbest_ref.py on the workload of decode_pairs_kbest_cases.py (both proved on the CPU by
test_decode_pairs_kbest_host.py), rank 0 against carmel_hip_decode_pairs, the 0M loop that the one-sided k-best refuses, the same
bytes across tiers, chunks and runs, K = 1024 by hand, the reduction to the one-sided k-best, edge cases and argument errors, and
the front end's --pair-kbest=N on the epron-jpron fixture."""
import itertools
import os
import re

import numpy as np
import pytest

from decode_pairs_cases import pairs_for
from decode_pairs_kbest_cases import CASES, LDS_DOUBLES, case, reference
from decode_pairs_kbest_ref import kbest
from decode_pairs_ref import Prepared, count, rescore
from test_decode_gpu import lines_for, random_machine, run
from test_decode_kbest_gpu import printed_ln
from test_decode_pairs_gpu import TOKEN, identity_machine

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -5
EXACT = {}  # case -> pairs whose paths were compared with the reference's, path for path


def check_pairs(P, pairs, K, ref, counts, weights, paths):
    """everything the device returns for `pairs` against the reference's (values, paths, tied) per pair: min(K, count) paths,
    pairwise distinct derivations of the pair, their path-order values the reference's bit for bit and in order, the reported
    weights the arcs added from the end, and the reference's very paths where it is untied; -> pairs compared path for path"""
    n_exact = 0
    for l, (x, y) in enumerate(pairs):
        vals, rpaths, tied = ref[l]
        got = [tuple(int(a) for a in p) for p in paths[l]]
        assert len(got) == len(weights[l]) == min(K, counts[l]) == len(vals), (l, x, y, len(got), counts[l])
        assert len(set(got)) == len(got), (l, x, y)
        fwds = []
        for p, wt in zip(got, weights[l]):
            fwd, rev = rescore(P, x, y, list(p))  # (asserts: start to final, spells x and y, no arc of weight zero)
            assert rev == wt, (l, x, y, p, rev, wt)
            fwds.append(float(fwd))
        assert fwds == vals, (l, x, y, fwds, vals)
        if not tied:
            assert got == rpaths, (l, x, y)
            n_exact += len(got) > 0
    return n_exact


def split(pairs):
    return [x for x, _ in pairs], [y for _, y in pairs]


@pytest.mark.parametrize("seed,tie", CASES)
def test_random_machines_against_the_reference(seed, tie):
    from carmel_amd.decode import Decoder
    c = case(seed, tie)
    xs, ys = split(c["pairs"])
    d = Decoder(c["w"], side=c["side"])
    weights, paths = d.decode_pairs_kbest(xs, ys, c["K"])
    d.close()
    EXACT[(seed, tie)] = check_pairs(c["P"], c["pairs"], c["K"], reference(seed, tie), c["count"], weights, paths)
    print("seed %d tie %d K %d: %d of %d pairs path for path, largest diagonals %d doubles (LDS holds %d)"
          % (seed, tie, c["K"], EXACT[(seed, tie)], len(xs), c["diag"], LDS_DOUBLES))


def test_exact_comparisons_were_made():
    """over the cases that ran (seed 2 if none did): some pair was compared path for path"""
    if not EXACT:
        test_random_machines_against_the_reference(2, False)
    print("%d pairs compared path for path over %d cases" % (sum(EXACT.values()), len(EXACT)))
    assert sum(EXACT.values()) > 0


@pytest.mark.parametrize("K", [1, 2, 5])
def test_rank_0_is_decode_pairs(K):
    from carmel_amd.decode import Decoder
    n_with = 0
    for seed in range(8):
        c = case(seed)
        xs, ys = split(c["pairs"])
        d = Decoder(c["w"], side=c["side"])
        best, paths1 = d.decode_pairs(xs, ys)
        weights, paths = d.decode_pairs_kbest(xs, ys, K)
        for l in range(len(xs)):
            if np.isneginf(best[l]):
                assert len(weights[l]) == 0 and len(paths[l]) == 0 and c["count"][l] == 0, (seed, l)
                continue
            assert weights[l][0] == best[l] and list(paths[l][0]) == list(paths1[l]), (seed, l)
            assert len(paths[l]) == min(K, c["count"][l]), (seed, l)
            n_with += 1
        best2, paths2 = d.decode_pairs(xs, ys)  # the entry points alternate on one handle
        d.close()
        assert best2.tobytes() == best.tobytes() and [list(p) for p in paths2] == [list(p) for p in paths1]
    assert n_with >= 30


def test_an_insertion_loop_is_accepted_and_a_00_cycle_refused():
    from carmel_amd._capi import CarmelHipError
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    # test_epsilon_cycle_is_refused_for_k_above_1's machine as a pair machine, its epsilon arcs now insertions *e*:c:
    # 0 -a:a-> 1, 1 -b:b-> 3, 1 -e:c-> 2, 1 -e:c-> 1 (a 0M self-loop), 2 -e:c-> 1
    lw = np.log([1.0, 0.5, 0.5, 0.25, 0.5])
    w = Wfst(4, 3, [0, 1, 1, 1, 2], [1, 3, 2, 1, 1], [1, 2, 0, 0, 0], [1, 2, 3, 3, 3], lw)
    d = Decoder(w)
    with pytest.raises(CarmelHipError, match="cycle") as e:
        d.decode_kbest([[1, 2]], 2)  # an epsilon cycle of the matched side
    assert e.value.code == ERR_UNSUPPORTED
    for K in (2, 3):
        ws, ps = d.decode_pairs_kbest([[1, 2]], [[1, 3, 3, 2]], K)
        assert [list(p) for p in ps[0]] == [[0, 2, 4, 1], [0, 3, 3, 1]], ps
        assert list(ws[0]) == [lw[0] + (lw[2] + (lw[4] + (lw[1] + 0.0))), lw[0] + (lw[3] + (lw[3] + (lw[1] + 0.0)))]
    ws, ps = d.decode_pairs_kbest([[1, 2]], [[1, 3, 2]], 4)  # the loop once: one alignment
    assert [list(p) for p in ps[0]] == [[0, 3, 1]]
    d.close()
    # the machine itself: a 00 cycle 1 -> 2 -> 1, refused for every K, naming it; the handle still decodes
    w = Wfst(4, 3, [0, 1, 1, 2], [1, 3, 2, 1], [1, 2, 0, 0], [1, 2, 0, 0], np.log([1.0, 0.5, 0.5, 0.5]))
    d = Decoder(w)
    for K in (1, 2):
        with pytest.raises(CarmelHipError, match="cycle") as e:
            d.decode_pairs_kbest([[1, 2]], [[1, 2]], K)
        assert e.value.code == ERR_UNSUPPORTED and ("1 -> 2 -> 1" in str(e.value) or "2 -> 1 -> 2" in str(e.value))
    best, paths = d.decode([[1, 2]])
    assert best[0] == np.log(0.5) and list(paths[0]) == [0, 1]
    d.close()


@pytest.mark.parametrize("seed", [3, 4, 5, 9])
def test_tiers_chunks_and_runs_give_the_same_bytes(hipopt, seed):
    from carmel_amd.decode import Decoder
    c = case(seed)
    assert c["K"] >= 5 and not c["wide"] and c["diag"] <= LDS_DOUBLES  # (a dense seed of the LDS tier)
    xs, ys = split(c["pairs"])
    d = Decoder(c["w"], side=c["side"])
    got = []
    # two runs, small chunks, every pair alone, the global tier
    for key, value in ((None, None), (None, None), ("decode_chunk_bytes", "4096"), ("decode_chunk_bytes", "1"), ("decode_lds", "0")):
        if key:
            hipopt.set(key, value)
        line_paths, logw, path_off, arcs = d.decode_pairs_kbest_raw(xs, ys, c["K"])
        got.append((line_paths.tobytes(), logw.tobytes(), path_off.tobytes(), arcs.tobytes()))
        weights, paths = d._per_line(len(xs), line_paths, logw, path_off, arcs)
        check_pairs(c["P"], c["pairs"], c["K"], reference(seed), c["count"], weights, paths)
        if key:
            hipopt.unset(key)
    d.close()
    assert len(np.frombuffer(got[0][1])) >= 10
    assert all(g == got[0] for g in got[1:])


def test_k_1024_by_hand():
    from carmel_amd._capi import CarmelHipError
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    lw = np.log([0.5, 0.3, 0.2])
    w = Wfst(1, 0, [0, 0, 0], [0, 0, 0], [1, 1, 1], [2, 2, 2], lw)  # one state, three parallel arcs a:b
    P = Prepared(1, 0, w.src, w.dst, w.isym, w.osym, w.logw)
    x, y = [1] * 7, [2] * 7
    assert 3 * (7 + 1) * 1 * 1024 > LDS_DOUBLES  # the diagonals are beyond LDS
    every = []
    for p in itertools.product(range(3), repeat=7):
        v = 0.0
        for a in p:
            v = v + lw[a]
        every.append(float(v))
    assert len(every) == 3 ** 7 == count(P, x, y)
    every.sort(reverse=True)
    d = Decoder(w)
    weights, paths = d.decode_pairs_kbest([x], [y], 1024)
    assert len(paths[0]) == 1024 and len({tuple(int(a) for a in p) for p in paths[0]}) == 1024
    fwds = []
    for p, wt in zip(paths[0], weights[0]):
        fwd, rev = rescore(P, x, y, [int(a) for a in p])
        assert rev == wt
        fwds.append(float(fwd))
    assert fwds == every[:1024]
    for K in (0, 1025):
        with pytest.raises(CarmelHipError, match="k must be") as e:
            d.decode_pairs_kbest([x], [y], K)
        assert e.value.code == ERR_ARG
    d.close()


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("other_epsilon", [False, True])
def test_pairs_reduce_to_the_one_sided_kbest(other_epsilon, K):
    """osym = isym on pairs (x, x), or an other side of epsilons on pairs (x, []): carmel_hip_decode_kbest's weights and paths"""
    from carmel_amd.decode import Decoder
    Q = 37
    rng = np.random.default_rng(31 + Q)
    w = identity_machine(rng, Q, 4, other_epsilon)
    lines = lines_for(rng, w, 0, 4, 12) + [x for x, _ in pairs_for(rng, w, 0, 4, 15)[3:]]
    other = [[] for _ in lines] if other_epsilon else lines
    d = Decoder(w)
    ws1, ps1 = d.decode_kbest(lines, K)
    ws2, ps2 = d.decode_pairs_kbest(lines, other, K)
    d.close()
    assert sum(len(x) > 0 for x in ws1) >= 3 and (K == 1 or max(len(x) for x in ws1) > 1)
    assert [x.tobytes() for x in ws2] == [x.tobytes() for x in ws1]
    assert [[list(p) for p in l] for l in ps2] == [[list(p) for p in l] for l in ps1]


def test_edge_cases():
    from carmel_amd._capi import lib, ptr, u32, u64
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    lw = np.log([0.5, 0.3, 0.2])
    # one state, start = final, a loop of each class but 00: 0 -a:e-> 0, 0 -e:b-> 0, 0 -a:b-> 0 (and one of weight zero)
    w = Wfst(1, 0, [0, 0, 0, 0], [0, 0, 0, 0], [1, 0, 1, 1], [0, 2, 2, 2], [lw[0], lw[1], lw[2], -np.inf])
    P = Prepared(1, 0, w.src, w.dst, w.isym, w.osym, w.logw)
    d = Decoder(w)
    line_paths, logw, path_off, arcs = d.decode_pairs_kbest_raw([], [], 3)  # no pairs
    assert list(line_paths) == [0] and len(logw) == 0 and list(path_off) == [0] and len(arcs) == 0
    pairs = [([], []), ([1], []), ([], [2]), ([1], [2]), ([1], [2] * 5), ([1] * 5, [2]), ([1], [3]), ([3], [2]), ([0], [2])]
    xs, ys = split(pairs)
    counts = [count(P, x, y) for x, y in pairs]
    assert counts == [1, 1, 1, 3, 11, 11, 0, 0, 0]
    for K in (1, 4, 16):
        weights, paths = d.decode_pairs_kbest(xs, ys, K)
        assert d.last_ms() >= 0
        assert list(weights[0]) == [0.0] and [list(p) for p in paths[0]] == [[]]  # the pair ([], []): the empty path alone
        assert [len(p) for p in paths] == [min(K, k) for k in counts]  # fewer derivations than K: exactly that many
        check_pairs(P, pairs, K, [kbest(P, x, y, K) for x, y in pairs], counts, weights, paths)
    # ([1], [2]) by hand: the MM arc, then the two equal paths: the one that ENDS in the matched arc a:e before the one that ends
    # in the epsilon arc e:b
    weights, paths = d.decode_pairs_kbest([[1]], [[2]], 3)
    assert [list(p) for p in paths[0]] == [[2], [1, 0], [0, 1]]
    # bad offsets on either side and a null line_paths are refused; the handle is as good as new
    off, sym, bad = u64([0, 1]), u32([1]), u64([1, 0])
    lp = np.zeros(2, np.uint64)
    F = lib.carmel_hip_decode_pairs_kbest
    for args in ((None, 2, 1, ptr(off), ptr(sym), ptr(off), ptr(sym)), (d._h, 2, 1, None, ptr(sym), ptr(off), ptr(sym)),
                 (d._h, 2, 1, ptr(off), ptr(sym), None, ptr(sym)), (d._h, 2, 1, ptr(off), None, ptr(off), ptr(sym)),
                 (d._h, 2, 1, ptr(off), ptr(sym), ptr(off), None), (d._h, 2, 1, ptr(bad), ptr(sym), ptr(off), ptr(sym)),
                 (d._h, 2, 1, ptr(off), ptr(sym), ptr(bad), ptr(sym)), (d._h, 2, 1 << 32, ptr(off), ptr(sym), ptr(off), ptr(sym))):
        assert F(*args, ptr(lp)) == ERR_ARG, args
    assert F(d._h, 2, 1, ptr(off), ptr(sym), ptr(off), ptr(sym), None) == ERR_ARG
    assert b"carmel_hip_decode_pairs_kbest" in lib.carmel_hip_last_error()
    weights, paths = d.decode_pairs_kbest([[1]], [[2]], 2)
    assert [list(p) for p in paths[0]] == [[2], [1, 0]]
    d.close()


def test_more_than_64_nodes_on_a_diagonal():
    from carmel_amd.decode import Decoder
    rng = np.random.default_rng(77)
    w = random_machine(rng, 90, 3, 500, p_eps=0.3, cyclic=False)
    pairs = [p for p in pairs_for(rng, w, 0, 3, 12) if min(len(p[0]), len(p[1])) >= 1]
    P = Prepared(w.n_states, w.final, w.src, w.dst, w.isym, w.osym, w.logw)
    K = 3
    xs, ys = split(pairs)
    d = Decoder(w)
    weights, paths = d.decode_pairs_kbest(xs, ys, K)
    d.close()
    counts = [count(P, x, y) for x, y in pairs]
    check_pairs(P, pairs, K, [kbest(P, x, y, K) for x, y in pairs], counts, weights, paths)
    assert sum(k > 0 for k in counts) >= 4


def test_front_end_pair_kbest_on_the_epron_jpron_pairs(golden_dir, tmp_path):
    fst, data = os.path.join(golden_dir, "epron-jpron.fst"), os.path.join(golden_dir, "epron-jpron.data")
    rows = open(data).read().split("\n")[:-1]
    ins, outs = rows[0::2], rows[1::2]
    E, J = tmp_path / "E", tmp_path / "J"
    A1, A3, A0 = tmp_path / "A1", tmp_path / "A3", tmp_path / "A0"
    E.write_text("".join(l + "\n" for l in ins))
    J.write_text("".join(l + "\n" for l in outs))
    rc0, out0, err0 = run(["-qbIEk", "1", "--pair-lines=%s" % J, "--pair-alignments=%s" % A0, str(E), fst])
    rc3, out3, err3 = run(["-qbIE", "--pair-kbest=3", "--pair-lines=%s" % J, "--pair-alignments=%s" % A3, str(E), fst])
    rc1, out1, err1 = run(["-qbIE", "--pair-kbest=1", "--pair-lines=%s" % J, "--pair-alignments=%s" % A1, str(E), fst])
    assert rc0 == 0 and rc3 == 0 and rc1 == 0, err3 + err1
    one, three = out0.split("\n")[:-1], out3.split("\n")[:-1]
    assert len(one) == len(ins) and len(three) == 3 * len(ins)
    assert three[0::3] == one and err3 == err0
    # --pair-kbest=1 is plain --pair-lines -k 1 to the byte
    assert out1 == out0 and err1 == err0 and A1.read_bytes() == A0.read_bytes()
    aligned = A3.read_text().split("\n")[:-1]
    assert len(aligned) == 3 * len(ins) and aligned[0::3] == A0.read_text().split("\n")[:-1]
    n_three = 0
    for l, (x, y) in enumerate(zip(ins, outs)):
        ranks = [a for a in aligned[3 * l:3 * l + 3] if a]
        printed = [p for p in three[3 * l:3 * l + 3] if p != "0"]
        assert len(ranks) == len(printed) >= 1 and len(set(ranks)) == len(ranks), (l, ranks)
        assert aligned[3 * l:3 * l + len(ranks)] == ranks  # (missing ranks are the LAST lines of the pair)
        n_three += len(ranks) == 3
        for line in ranks:  # every alignment spells the pair's two lines
            toks = [re.match(TOKEN + "$", t).groups() for t in line.split(" ")]
            assert [a for a, _ in toks if a != "*e*"] == x.split() and [b for _, b in toks if b != "*e*"] == y.split(), line
        ws = [printed_ln(p.split()[-1]) for p in printed]
        # (what is printed is the path's arcs added in path order, the value the lists are ordered by: non-increasing as printed)
        assert all(a >= b for a, b in zip(ws, ws[1:])), (l, ws)
        assert all(p.startswith(x + " ") for p in printed), (l, printed)
    assert n_three >= 1
    rct, _, errt = run(["-qbIE", "--pair-kbest=3", "--pair-lines=%s" % J, str(E), fst], env={"CARMEL_TIMING": "1"})
    assert rct == 0 and "timing: pairs kbest " in errt
