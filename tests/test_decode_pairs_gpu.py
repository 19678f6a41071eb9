"""GPU: batch pair decoding (carmel_hip_decode_pairs / carmel_hip_decode_pairs_sum, Decoder.decode_pairs / sum_pairs, carmel -b
--pair-lines=FILE; csrc/decode_pairs.hip) -- random machines against the numpy planes of decode_pairs_ref.py (workload:
decode_pairs_cases.py, what it contains and why the reference is right: test_decode_pairs_host.py), the reductions to the
one-sided decoders bit for bit, exact edge cases, the memory tiers and chunking, cycles, the trainer's per-pair probabilities as
an independent device route, argument errors, and the front end on the epron-jpron fixture."""
import re

import numpy as np
import pytest

from decode_pairs_cases import SEEDS, case, pairs_for
from decode_pairs_ref import Prepared, count, pair_best, pair_sum, rescore
from test_decode_gpu import lines_for, random_machine, run
from test_decode_kbest_gpu import printed_ln
from test_decode_pairs_host import close_enough  # (RTOL = 1e-10 of max(1, |ref|): derived there)

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -5


def check_pairs(P, pairs, best, paths, sums, ref_sum=None, ref_best=None):
    """everything the device returns for `pairs` against the reference: the has-derivation set, the sums within RTOL, every path a
    derivation of its pair whose path-order sum is the reference's best value bit for bit, the reported weight the path's arcs
    added from the end, the path itself where the reference's best is untied; -> (pairs with a derivation, untied ones, the
    worst relative error of a sum)"""
    n_with = n_untied = 0
    worst = 0.0
    for l, (x, y) in enumerate(pairs):
        rs = ref_sum[l] if ref_sum is not None else pair_sum(P, x, y)
        rb, rp, tied = ref_best[l] if ref_best is not None else pair_best(P, x, y)
        print("pair %d: n %d m %d sum %r ref %r best %r ref %r" % (l, len(x), len(y), sums[l], rs, best[l], rb))
        if rp is None:
            assert np.isneginf(rs) and np.isneginf(sums[l]) and np.isneginf(best[l]) and len(paths[l]) == 0, (l, x, y)
            continue
        n_with += 1
        assert close_enough(sums[l], rs), (l, x, y, sums[l], rs)
        worst = max(worst, abs(sums[l] - rs) / max(1.0, abs(rs)))
        fwd, rev = rescore(P, x, y, [int(a) for a in paths[l]])
        assert fwd == rb and rev == best[l], (l, x, y, fwd, rb, rev, best[l])
        if not tied:
            assert [int(a) for a in paths[l]] == rp, (l, x, y)
            n_untied += 1
    return n_with, n_untied, worst


@pytest.mark.parametrize("seed", SEEDS)
def test_random_machines_against_numpy(hipopt, seed):
    from carmel_amd._capi import CarmelHipError
    from carmel_amd.decode import Decoder
    c = case(seed)
    if c["lds_off"]:
        hipopt.set("decode_lds", "0")  # a small machine in the global tier
    xs, ys = [x for x, _ in c["pairs"]], [y for _, y in c["pairs"]]
    d = Decoder(c["w"], side=c["side"])
    if c["P"] is None:  # the 00 arcs have a cycle: refused by both, and the handle stays usable
        for call in (d.decode_pairs, d.sum_pairs):
            with pytest.raises(CarmelHipError, match="cycle") as e:
                call(xs, ys)
            assert e.value.code == ERR_UNSUPPORTED
        best, _ = d.decode(xs)
        assert best.shape == (len(xs),)
        d.close()
        return
    best, paths = d.decode_pairs(xs, ys)
    sums = d.sum_pairs(xs, ys)
    d.close()
    assert sums.dtype == np.float64 and sums.shape == best.shape == (len(xs),)
    n_with, _, worst = check_pairs(c["P"], c["pairs"], best, paths, sums, c["sum"], c["best"])
    print("seed %d: %d of %d pairs with a derivation, worst relative error of a sum %.3g" % (seed, n_with, len(xs), worst))


def identity_machine(rng, Q, V, other_epsilon):
    """an acyclic random machine whose other side repeats its matched side, or is all epsilon"""
    from carmel_amd.model import Wfst
    w = random_machine(rng, Q, V, 4 * Q, p_eps=0.2, cyclic=False)
    return Wfst(w.n_states, w.final, w.src, w.dst, w.isym, np.zeros_like(w.isym) if other_epsilon else w.isym.copy(), w.logw)


@pytest.mark.parametrize("other_epsilon", [False, True])
@pytest.mark.parametrize("Q", [37, 4200])
def test_pairs_reduce_to_the_one_sided_decoders(Q, other_epsilon):
    """osym = isym on pairs (x, x), or an other side of epsilons on pairs (x, []): carmel_hip_decode's bests and paths and
    carmel_hip_decode_sum's sums, bit for bit"""
    from carmel_amd.decode import Decoder
    rng = np.random.default_rng(31 + Q)
    w = identity_machine(rng, Q, 4, other_epsilon)
    n = 24 if Q < 4096 else 6
    # lines_for's short walks hardly ever end in the final state of a large machine: half the lines are walks that stop there
    lines = lines_for(rng, w, 0, 4, n // 2) + [x for x, _ in pairs_for(rng, w, 0, 4, n // 2 + 3)[3:]]
    d = Decoder(w)
    best, paths = d.decode(lines)
    sums = d.sum(lines)
    other = [[] for _ in lines] if other_epsilon else lines
    pbest, ppaths = d.decode_pairs(lines, other)
    psums = d.sum_pairs(lines, other)
    d.close()
    assert np.isfinite(best).sum() >= 3
    assert pbest.tobytes() == best.tobytes() and psums.tobytes() == sums.tobytes()
    assert [list(p) for p in ppaths] == [list(p) for p in paths]


def decode_all(w, pairs, side=0):
    from carmel_amd.decode import Decoder
    d = Decoder(w, side=side)
    xs, ys = [x for x, _ in pairs], [y for _, y in pairs]
    best, paths = d.decode_pairs(xs, ys)
    sums = d.sum_pairs(xs, ys)
    d.close()
    return best, paths, sums


def test_edge_cases():
    from carmel_amd.model import Wfst
    lw = np.log([0.5, 0.3, 0.2])
    # one state, start = final, a loop of each class but 00: 0 -a:e-> 0, 0 -e:b-> 0, 0 -a:b-> 0 (and one of weight zero)
    w = Wfst(1, 0, [0, 0, 0, 0], [0, 0, 0, 0], [1, 0, 1, 1], [0, 2, 2, 2], [lw[0], lw[1], lw[2], -np.inf])
    P = Prepared(1, 0, w.src, w.dst, w.isym, w.osym, w.logw)
    pairs = [([], []), ([1], []), ([], [2]), ([1], [2] * 5), ([1] * 5, [2]), ([1], [2]), ([1], [3]), ([3], [2]), ([0], [2])]
    best, paths, sums = decode_all(w, pairs)
    assert best[0] == 0.0 and sums[0] == 0.0 and len(paths[0]) == 0  # final = start, the empty pair
    assert best[1] == lw[0] and list(paths[1]) == [0] and sums[1] == lw[0]  # m = 0
    assert best[2] == lw[1] and list(paths[2]) == [1] and sums[2] == lw[1]  # n = 0
    assert count(P, *pairs[3]) == 6 + 5 and count(P, *pairs[4]) == 6 + 5  # (1, 5) and (5, 1)
    assert list(paths[5]) == [2] and close_enough(sums[5], np.logaddexp(lw[2], np.logaddexp(lw[0] + lw[1], lw[1] + lw[0])))
    check_pairs(P, pairs, best, paths, sums)
    # all four arc classes at one node, state 2 of (1, 1): 0 -a:b-> 1, 0 -a:e-> 1, 0 -e:b-> 1, 0 -e:e-> 1, the same from 1 to 2
    cls_i, cls_o = [1, 1, 0, 0], [2, 0, 2, 0]
    w = Wfst(3, 2, [0] * 4 + [1] * 4, [1] * 4 + [2] * 4, cls_i * 2, cls_o * 2, np.log(np.linspace(0.2, 0.9, 8)))
    P = Prepared(3, 2, w.src, w.dst, w.isym, w.osym, w.logw)
    pairs = [([1], [2]), ([], []), ([1], []), ([], [2]), ([1, 1], [2, 2]), ([1, 1], [2]), ([1], [2, 2]), ([1, 1, 1], [2])]
    best, paths, sums = decode_all(w, pairs)
    assert [count(P, x, y) for x, y in pairs[:4]] == [4, 1, 2, 2]  # MM.00, 00.MM, M0.0M, 0M.M0; 00.00; ...
    assert list(paths[1]) == [3, 7] and best[1] == w.logw[3] + (w.logw[7] + 0.0)
    assert np.isneginf(best[7]) and np.isneginf(sums[7])
    assert check_pairs(P, pairs, best, paths, sums)[0] == 7
    # the same pairs from the other side
    best1, paths1, sums1 = decode_all(w, [(y, x) for x, y in pairs], side=1)
    assert best1.tobytes() == best.tobytes() and [list(p) for p in paths1] == [list(p) for p in paths]
    check_pairs(Prepared(3, 2, w.src, w.dst, w.osym, w.isym, w.logw), [(y, x) for x, y in pairs], best1, paths1, sums1)
    # ties: among equal matched arcs the lowest id; a matched arc beats an equal epsilon arc, whatever the ids
    h = np.log(0.5)
    w = Wfst(3, 1, [0, 0, 0, 0, 2], [2, 1, 1, 1, 1], [1, 1, 1, 1, 0], [0, 2, 2, 2, 2], [h, -np.inf, h, h, 0.0])
    best, paths, sums = decode_all(w, [([1], [2])])
    assert list(paths[0]) == [2] and best[0] == h  # not [0, 4] (an equal epsilon arc), not [1] (weight zero), not [3]
    assert close_enough(sums[0], np.log(1.5))


def test_more_than_64_nodes_on_a_diagonal():
    rng = np.random.default_rng(77)
    w = random_machine(rng, 90, 3, 500, p_eps=0.3, cyclic=False)
    pairs = [p for p in pairs_for(rng, w, 0, 3, 12) if min(len(p[0]), len(p[1])) >= 1]
    P = Prepared(w.n_states, w.final, w.src, w.dst, w.isym, w.osym, w.logw)
    best, paths, sums = decode_all(w, pairs)
    assert check_pairs(P, pairs, best, paths, sums)[0] >= 4


def tier_machine(Q_total):
    """681 live states (and unreachable ones up to Q_total), the final state among the live ones"""
    from carmel_amd.model import Wfst
    w = random_machine(np.random.default_rng(5), 681, 3, 2500, p_eps=0.3, cyclic=False)
    return Wfst(Q_total, w.final, w.src, w.dst, w.isym, w.osym, w.logw)


def test_tiers_give_the_same_bytes(hipopt):
    """3 (min(n, m) + 1) |Q| doubles: |Q| = 682 with min(n, m) = 3 is 8184, the last that fits the LDS tier; |Q| = 683 is 8196;
    a longer pair in the call, decode_lds=0 and |Q| > 4096 put the same pairs into the global tier"""
    from carmel_amd.decode import Decoder
    w = tier_machine(682)
    rng = np.random.default_rng(6)
    pairs = [p for p in pairs_for(rng, w, 0, 3, 40) if min(len(p[0]), len(p[1])) <= 3][:8]
    longer = [p for p in pairs_for(rng, w, 0, 3, 40) if min(len(p[0]), len(p[1])) >= 4][:1]
    assert max(min(len(x), len(y)) for x, y in pairs) == 3 and longer
    P = Prepared(w.n_states, w.final, w.src, w.dst, w.isym, w.osym, w.logw)
    xs, ys = [x for x, _ in pairs], [y for _, y in pairs]
    results = []

    def one(machine, extra=()):
        d = Decoder(machine)
        b, p = d.decode_pairs(xs + [x for x, _ in extra], ys + [y for _, y in extra])
        s = d.sum_pairs(xs + [x for x, _ in extra], ys + [y for _, y in extra])
        d.close()
        n = len(xs)
        results.append((b[:n].tobytes(), s[:n].tobytes(), [list(q) for q in p[:n]]))
        return b[:n], p[:n], s[:n]

    b, p, s = one(w)  # 8184 doubles: LDS
    assert check_pairs(P, pairs, b, p, s)[0] >= 3
    one(tier_machine(683))  # 8196 doubles: global
    one(w, longer)  # the call's longest pair decides
    one(tier_machine(4200))
    hipopt.set("decode_lds", "0")
    one(w)
    assert all(r == results[0] for r in results[1:])


def test_chunks_and_runs_give_the_same_bytes(hipopt):
    from carmel_amd.decode import Decoder
    rng = np.random.default_rng(8)
    w = random_machine(rng, 30, 4, 150, p_eps=0.3, cyclic=False)
    pairs = pairs_for(rng, w, 0, 4, 60)
    xs, ys = [x for x, _ in pairs], [y for _, y in pairs]
    d = Decoder(w)
    got = []
    for chunk in (None, None, "4096"):
        hipopt.set("decode_chunk_bytes", chunk)
        b, p = d.decode_pairs(xs, ys)
        got.append((b.tobytes(), d.sum_pairs(xs, ys).tobytes(), [list(q) for q in p]))
    hipopt.unset("decode_chunk_bytes")
    d.close()
    assert np.isfinite(np.frombuffer(got[0][0])).sum() >= 20
    assert got[0] == got[1] == got[2]


def test_cycles():
    from carmel_amd._capi import CarmelHipError
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    # a 00 cycle 1 -> 2 -> 1: refused by both calls, naming it; the handle still decodes
    w = Wfst(4, 3, [0, 1, 1, 2], [1, 3, 2, 1], [1, 2, 0, 0], [1, 2, 0, 0], np.log([1.0, 0.5, 0.5, 0.5]))
    d = Decoder(w)
    for call in (d.decode_pairs, d.sum_pairs):
        with pytest.raises(CarmelHipError, match="cycle") as e:
            call([[1, 2]], [[1, 2]])
        assert e.value.code == ERR_UNSUPPORTED and ("1 -> 2 -> 1" in str(e.value) or "2 -> 1 -> 2" in str(e.value))
    best, paths = d.decode([[1, 2]])
    assert best[0] == np.log(0.5) and list(paths[0]) == [0, 1]
    new = w.logw.copy()
    new[3] = -np.inf  # an arc of weight zero is no arc: no cycle any more
    d.set_weights(new)
    assert d.sum_pairs([[1, 2]], [[1, 2]])[0] == np.log(0.5)
    d.close()
    # an insertion loop: 0 -a:b/w-> 1, 1 -e:c/0.5-> 1: an epsilon cycle of the input side, none of the pair trellis
    lw, half = np.log(0.3), np.log(0.5)
    w = Wfst(2, 1, [0, 1], [1, 1], [1, 0], [2, 3], [lw, half])
    d = Decoder(w)
    best, paths = d.decode_pairs([[1]], [[2, 3, 3]])
    assert list(paths[0]) == [0, 1, 1] and best[0] == lw + (half + (half + 0.0))
    assert d.sum_pairs([[1]], [[2, 3, 3]])[0] == (0.0 + lw + half) + half
    with pytest.raises(CarmelHipError, match="cycle") as e:
        d.sum([[1]])
    assert e.value.code == ERR_UNSUPPORTED
    d.close()


@pytest.mark.parametrize("seed", [1, 2, 4])
def test_the_trainer_gives_the_same_pair_probabilities(seed):
    """the same machine and pairs through carmel_hip_estimate (a derivation lattice per pair): an independent device route"""
    from carmel_amd.decode import Decoder
    from carmel_amd.model import NORM_NONE, Corpus
    from carmel_amd.trainer import HipForwardBackward
    c = case(seed)
    assert c["P"] is not None
    pairs = c["pairs"]
    corpus = Corpus.from_lists([(y, x) if c["side"] else (x, y) for x, y in pairs])
    fb = HipForwardBackward(c["w"], corpus, norm_group=NORM_NONE, normalize_first=False)
    fb.estimate(per_pair=True)
    has, lp = fb.has_deriv.astype(bool), fb.pair_logprob.copy()
    fb.close()
    d = Decoder(c["w"], side=c["side"])
    sums = d.sum_pairs([x for x, _ in pairs], [y for _, y in pairs])
    d.close()
    assert np.array_equal(has, np.isfinite(sums)) and has.sum() >= 4
    for got, ref in zip(sums[has], lp[has]):
        assert close_enough(got, ref), (got, ref)


def test_argument_errors_and_set_weights():
    from carmel_amd._capi import lib, ptr, u32, u64
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    lw = np.log([0.5, 0.25])
    w = Wfst(2, 1, [0, 0], [1, 1], [1, 1], [2, 2], lw)
    d = Decoder(w)
    off, sym, bad = u64([0, 1]), u32([1]), u64([1, 0])
    out, poff = np.zeros(1), np.zeros(2, np.uint64)
    P, S = lib.carmel_hip_decode_pairs, lib.carmel_hip_decode_pairs_sum
    for args in ((None, 1, ptr(off), ptr(sym), ptr(off), ptr(sym)), (d._h, 1, None, ptr(sym), ptr(off), ptr(sym)),
                 (d._h, 1, ptr(off), ptr(sym), None, ptr(sym)), (d._h, 1, ptr(off), None, ptr(off), ptr(sym)),
                 (d._h, 1, ptr(off), ptr(sym), ptr(off), None), (d._h, 1, ptr(bad), ptr(sym), ptr(off), ptr(sym)),
                 (d._h, 1, ptr(off), ptr(sym), ptr(bad), ptr(sym)), (d._h, 1 << 32, ptr(off), ptr(sym), ptr(off), ptr(sym))):
        assert P(*args, ptr(out), ptr(poff)) == ERR_ARG, args
        assert S(*args, ptr(out)) == ERR_ARG, args
    assert P(d._h, 1, ptr(off), ptr(sym), ptr(off), ptr(sym), None, ptr(poff)) == ERR_ARG
    assert P(d._h, 1, ptr(off), ptr(sym), ptr(off), ptr(sym), ptr(out), None) == ERR_ARG
    assert S(d._h, 1, ptr(off), ptr(sym), ptr(off), ptr(sym), None) == ERR_ARG
    assert b"carmel_hip_decode_pairs_sum" in lib.carmel_hip_last_error()
    best, paths = d.decode_pairs([[1]], [[2]])  # the handle is as good as new
    assert best[0] == lw[0] and list(paths[0]) == [0]
    assert close_enough(d.sum_pairs([[1]], [[2]])[0], np.log(0.75))
    assert d.last_ms() >= 0
    assert d.decode([[1]])[0][0] == lw[0]  # the entries alternate on one handle
    d.set_weights([-np.inf, np.log(0.125)])
    best, paths = d.decode_pairs([[1]], [[2]])
    assert best[0] == np.log(0.125) and list(paths[0]) == [1]
    assert d.sum_pairs([[1]], [[2]])[0] == np.log(0.125)
    d.close()


PPX = r"product of probs=(\S+), probability=2\^(\S+)"
TOKEN = r'(\*e\*|"[^"]*"):(\*e\*|"[^"]*")'


def test_front_end_on_the_epron_jpron_pairs(oracle, golden_dir, tmp_path):
    import os
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    fst, data = os.path.join(golden_dir, "epron-jpron.fst"), os.path.join(golden_dir, "epron-jpron.data")
    rows = open(data).read().split("\n")[:-1]
    ins, outs = rows[0::2], rows[1::2]
    E, J, A = tmp_path / "E", tmp_path / "J", tmp_path / "A"
    E.write_text("".join(l + "\n" for l in ins))
    J.write_text("".join(l + "\n" for l in outs))
    rc, out, err = run(["-qbIEk", "1", "--sum-paths", "--pair-lines=%s" % J, "--pair-alignments=%s" % A, str(E), fst],
                       env={"CARMEL_TIMING": "1"})
    assert rc == 0, err
    assert "timing: pairs " in err
    printed = out.split("\n")[:-1]  # one line per pair: -I of a pair's path spells the line again, and its weight follows
    assert len(printed) == len(ins) and all(p.startswith(x + " ") for p, x in zip(printed, ins)), out
    aligned = A.read_text().split("\n")[:-1]
    assert len(aligned) == len(ins)
    for line, x, y in zip(aligned, ins, outs):
        toks = [re.match(TOKEN + "$", t).groups() for t in line.split(" ")]
        assert [a for a, _ in toks if a != "*e*"] == x.split() and [b for _, b in toks if b != "*e*"] == y.split(), line
    # the same pairs through the Python interface, on the oracle's reading of the files
    ow = oracle.OracleWfst.parse(open(fst).read())
    w, cp = ow.arrays(), oracle.OracleCorpus.parse(ow, open(data).read()).arrays()
    line = lambda side, l: [int(s) for s in cp[side + "_sym"][int(cp[side + "_off"][l]):int(cp[side + "_off"][l + 1])]]
    xs, ys = [line("in", l) for l in range(len(ins))], [line("out", l) for l in range(len(ins))]
    d = Decoder(Wfst(w["n_states"], w["final"], w["src"], w["dst"], w["isym"], w["osym"], w["logw"]))
    best, _ = d.decode_pairs(xs, ys)
    sums = d.sum_pairs(xs, ys)
    d.close()
    assert np.isfinite(best).all() and np.isfinite(sums).all()
    rep = [l for l in err.split("\n") if l and not l.startswith("timing:")]
    assert "Derivations found for all %d inputs." % len(ins) in rep
    vit = [re.match(r"Viterbi \(best path\) " + PPX, l) for l in rep if l.startswith("Viterbi")]
    tot = [re.match(r"Sum \(all paths\) " + PPX, l) for l in rep if l.startswith("Sum (all paths)")]
    assert len(vit) == 1 and len(tot) == 1 and vit[0] and tot[0], rep
    total_best = total_sum = 0.0
    for b, s in zip(best, sums):
        total_best, total_sum = total_best + b, total_sum + s
    print("Viterbi %s python %r; Sum %s python %r" % (vit[0].group(1), total_best, tot[0].group(1), total_sum))
    assert close_enough(printed_ln(vit[0].group(1)), total_best) and close_enough(printed_ln(tot[0].group(1)), total_sum)
    # carmel -S on the same pairs: the trainer's forward pass
    rcs, _, errs = run(["-S", data, fst])
    assert rcs == 0, errs
    scored = re.search(r"-S corpus product of probs=(\S+),", errs)
    assert scored, errs
    assert close_enough(printed_ln(tot[0].group(1)), printed_ln(scored.group(1))), (tot[0].group(1), scored.group(1))
    # what goes to stdout does not depend on --sum-paths
    rc2, out2, err2 = run(["-qbIEk", "1", "--pair-lines=%s" % J, str(E), fst])
    assert rc2 == 0 and out2 == out and "Sum (all paths)" not in err2
