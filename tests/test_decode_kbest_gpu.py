"""GPU: batch k-best decoding (carmel_hip_decode_kbest, carmel --kbest=N; csrc/decode_kbest.hip) -- random machines against the
path-carrying Python reference of decode_kbest_ref.py (inputs and reference results: decode_kbest_cases.py), the memory tiers
and chunking, K = 1 against the 1-best decoder, the edge cases, and the front end on the tutorial's cluster machines."""
import math

import numpy as np
import pytest

from decode_kbest_cases import BIG, SEEDS, TIER_SEEDS, case
from decode_ref import decode_expected, golden_file, rescore
from test_decode_gpu import lines_for, random_machine, run
from test_decode_host import noe

pytestmark = pytest.mark.gpu


def decode_case(c):
    """-> per side (weights, paths) of the case's lines"""
    from carmel_amd.decode import Decoder
    out = []
    for side, lines, msym, ref in c["sides"]:
        d = Decoder(c["w"], side=side)
        out.append(d.decode_kbest(lines, c["K"]))
        d.close()
    return out


def check_case(c, results):
    w, n_exact = c["w"], 0
    for (side, lines, msym, ref), (weights, paths) in zip(c["sides"], results):
        assert len(weights) == len(paths) == len(lines)
        for line, (vals, rpaths, tied), ws, ps in zip(lines, ref, weights, paths):
            assert len(ps) == len(ws) == len(vals), (line, len(ps), len(vals))
            scores = [rescore(w.src, w.dst, msym, w.logw, line, [int(a) for a in p], w.final) for p in ps]  # (checks each path)
            assert [s[0] for s in scores] == vals, (line, [s[0] for s in scores], vals)  # bit for bit, in order
            assert [s[1] for s in scores] == list(ws), (line, scores, ws)  # the reported weight: added from the end
            assert len(set(tuple(int(a) for a in p) for p in ps)) == len(ps), line
            if not tied:
                assert [tuple(int(a) for a in p) for p in ps] == rpaths, line
                n_exact += 1
    return n_exact


def same(a, b):
    return all(x[0][l].tobytes() == y[0][l].tobytes() and len(x[1][l]) == len(y[1][l]) and
               all(np.array_equal(p, q) for p, q in zip(x[1][l], y[1][l]))
               for x, y in zip(a, b) for l in range(len(x[0])))


@pytest.mark.parametrize("seed", SEEDS)
def test_random_machines_against_the_reference(seed):
    c = case(seed)
    check_case(c, decode_case(c))


def test_global_tier_by_size():
    c = case(BIG)
    assert c["w"].n_states * c["K"] > 4096
    assert check_case(c, decode_case(c))


@pytest.mark.parametrize("seed", TIER_SEEDS)
def test_tiers_and_chunks_agree(hipopt, seed):
    c = case(seed)
    a = decode_case(c)
    check_case(c, a)
    assert same(a, decode_case(c))  # two runs
    hipopt.set("decode_chunk_bytes", "4096")
    b = decode_case(c)
    assert same(a, b)
    hipopt.set("decode_lds", "0")
    g = decode_case(c)
    check_case(c, g)
    assert same(a, g)


@pytest.mark.parametrize("seed", range(8))
def test_rank_0_is_the_1best_path(seed):
    """decode_kbest(lines, 1) is decode(lines) -- on cyclic epsilon subgraphs too -- and for K >= 2 rank 0 is decode's path"""
    from carmel_amd.decode import Decoder
    rng = np.random.default_rng(300 + seed)
    cyclic = seed % 2 == 1
    Q, V = int(rng.integers(2, 41)), int(rng.integers(2, 7))
    w = random_machine(rng, Q, V, int(rng.integers(Q, 4 * Q + 20)), p_eps=0.2, cyclic=cyclic)
    for side in (0, 1):
        lines = lines_for(rng, w, side, V, 12)
        d = Decoder(w, side=side)
        best, paths = d.decode(lines)
        for K in (1,) if cyclic else (1, 2, 5):
            ws, ps = d.decode_kbest(lines, K)
            for l in range(len(lines)):
                if np.isneginf(best[l]):
                    assert len(ws[l]) == 0 and len(ps[l]) == 0
                    continue
                assert (K > 1 or len(ws[l]) == 1) and ws[l][0] == best[l] and np.array_equal(ps[l][0], paths[l]), (K, l)
        again = d.decode(lines)  # the two entries alternate on one handle
        assert again[0].tobytes() == best.tobytes() and all(np.array_equal(x, y) for x, y in zip(again[1], paths))
        d.close()


def test_every_line_alone_in_its_chunk_and_no_lines(hipopt):
    """a budget below every line's cost (each line goes alone) returns the bytes of the default budget, from all three entries;
    an empty list of lines returns empty results"""
    from carmel_amd.decode import Decoder
    rng = np.random.default_rng(77)
    w = random_machine(rng, 40, 5, 160, p_eps=0.2, cyclic=False)
    lines = lines_for(rng, w, 0, 5, 12)
    d = Decoder(w)

    def everything(ls):
        best, paths = d.decode(ls)
        raw = d.decode_kbest_raw(ls, 3)
        return [best.tobytes()] + [p.tobytes() for p in paths] + [a.tobytes() for a in raw] + [d.sum(ls).tobytes()]

    def nothing():
        best, paths = d.decode([])
        assert len(best) == 0 and paths == []
        assert d.decode_kbest([], 3) == ([], [])
        line_paths, logw, path_off, arcs = d.decode_kbest_raw([], 3)
        assert list(line_paths) == [0] and len(logw) == 0 and list(path_off) == [0] and len(arcs) == 0
        assert len(d.sum([])) == 0

    try:
        a = everything(lines)
        assert any(len(p) for p in a[1:13])  # some line has a path
        nothing()
        hipopt.set("decode_chunk_bytes", "1")
        assert everything(lines) == a
        nothing()
    finally:
        d.close()


def test_epsilon_cycle_is_refused_for_k_above_1():
    from carmel_amd._capi import CarmelHipError
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    # 0 -a-> 1, 1 -eps-> 2, 2 -eps-> 1, 1 -b-> 3: a cycle of weight 1/4
    w = Wfst(4, 3, [0, 1, 1, 2], [1, 3, 2, 1], [1, 2, 0, 0], [1, 2, 0, 0], np.log([1.0, 0.5, 0.5, 0.5]))
    d = Decoder(w)
    with pytest.raises(CarmelHipError, match="cycle") as e:
        d.decode_kbest([[1, 2]], 2)
    assert e.value.code == -5  # CARMEL_HIP_ERR_UNSUPPORTED
    best, paths = d.decode([[1, 2]])  # the handle stays usable
    assert best[0] == np.log(1.0) + (np.log(0.5) + 0.0) and list(paths[0]) == [0, 1]
    ws, ps = d.decode_kbest([[1, 2]], 1)
    assert list(ws[0]) == [best[0]] and list(ps[0][0]) == [0, 1]
    d.close()


def test_edge_cases():
    from carmel_amd._capi import CarmelHipError
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    # 0 -1-> 1 (two parallel arcs), 1 -2-> 2, 0 -eps-> 2 (the empty line), 0 -1-> 2
    w = Wfst(3, 2, [0, 0, 0, 0, 1], [1, 1, 2, 2, 2], [1, 1, 0, 1, 2], [1, 1, 0, 1, 2], np.log([0.5, 0.25, 0.125, 0.5, 0.5]))
    d = Decoder(w)
    for K in (0, 1025):
        with pytest.raises(CarmelHipError, match="k must be"):
            d.decode_kbest([[1, 2]], K)
    ws, ps = d.decode_kbest([[1, 2], [2], [], [1], [9]], 4)
    assert [list(p) for p in ps[0]] == [[0, 4], [1, 4]]  # fewer than K derivations: exactly that many
    assert list(ws[0]) == [np.log(0.5) + (np.log(0.5) + 0.0), np.log(0.25) + (np.log(0.5) + 0.0)]
    assert len(ps[1]) == 0 and len(ws[1]) == 0  # none
    assert [list(p) for p in ps[2]] == [[2]] and list(ws[2]) == [np.log(0.125)]  # the empty line
    assert [list(p) for p in ps[3]] == [[3]]
    assert len(ps[4]) == 0  # a symbol no arc carries
    assert d.last_ms() >= 0
    d.close()


def printed_ln(tok):
    return float(tok[2:]) if tok.startswith("e^") else float(tok[:-2]) if tok.endswith("ln") else math.log(float(tok))


def test_front_end_kbest_on_the_cluster_machines(golden_dir, tmp_path):
    gold = decode_expected(golden_dir)["cluster"]
    members = [golden_file(golden_dir, m, tmp_path) for m in ("cat.fsa.trained.noe", "spellout.fst.trained")]
    lines = noe(golden_dir, gold["data"])[:50] + ["no_such_symbol"]
    text = "".join(l + "\n" for l in lines)
    for form in ("-qbsriWIE", "-qbsriIE"):
        rc1, out1, err1 = run([form + "k", "1"] + members, stdin=text)
        rc3, out3, err3 = run([form, "--kbest=3"] + members, stdin=text)
        assert rc1 == 0 and rc3 == 0, err3
        one, three = out1.split("\n")[:-1], out3.split("\n")[:-1]
        assert len(one) == len(lines) and len(three) == 3 * len(lines)
        assert three[0::3] == one
        assert err3 == err1
        fill = "" if "W" in form else "0"
        assert three[-3:] == [fill] * 3  # the unknown symbol: three fill lines
        if "W" not in form:
            n_several = 0
            for l in range(len(lines) - 1):
                ws = [printed_ln(x.split()[-1]) for x in three[3 * l:3 * l + 3] if x != "0"]
                assert ws and all(a >= b for a, b in zip(ws, ws[1:])), (l, ws)
                n_several += len(ws) > 1
            assert n_several
