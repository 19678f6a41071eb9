"""GPU: batch all-paths sums (carmel_hip_decode_sum, Decoder.sum, carmel -b --sum-paths; csrc/decode_sum.hip) -- random machines
against the numpy forward pass of decode_sum_ref.py (workload: decode_sum_cases.py, what it contains: test_decode_sum_host.py),
the same lines against the k-best decoder's paths, exact small cases, the memory tiers and chunking, and the front end's report
on the tutorial's cipher and cluster machines."""
import re

import numpy as np
import pytest

from decode_ref import decode_expected, golden_file
from decode_sum_cases import SEEDS, case, cross_checked
from decode_sum_ref import forward, prepare
from test_decode_gpu import check_random, lines_for, random_machine, run
from test_decode_host import noe
from test_decode_kbest_gpu import printed_ln

pytestmark = pytest.mark.gpu

# the relative 1e-10 of the tagging decode test (test_decode_gpu.py): one rounding of a value of magnitude <= ~1e2 per trellis
# step (<= 1.4e-14) and a few ulp per Lse read-out, over at most (14 + 1) x 6 dependent steps: below 1e-11
RTOL = 1e-10


def close_enough(got, ref):
    return abs(got - ref) <= RTOL * max(1.0, abs(ref))


@pytest.mark.parametrize("seed", SEEDS)
def test_random_machines_against_numpy(hipopt, seed):
    from carmel_amd._capi import CarmelHipError
    from carmel_amd.decode import Decoder
    c = case(seed)
    w = c["w"]
    if c["lds_off"]:
        hipopt.set("decode_lds", "0")  # a small machine in the global tier
    for side, lines, ref, counts, _ in c["sides"]:
        d = Decoder(w, side=side)
        if ref is None:  # the epsilon arcs of this side have a cycle
            with pytest.raises(CarmelHipError, match="cycle") as e:
                d.sum(lines)
            assert e.value.code == -5  # CARMEL_HIP_ERR_UNSUPPORTED
            best, paths = d.decode(lines)  # the handle stays usable
            check_random(w, side, lines, best, paths)
            d.close()
            continue
        got = d.sum(lines)
        d.close()
        assert got.dtype == np.float64 and got.shape == (len(lines),)
        for l, (g, r) in enumerate(zip(got, ref)):
            if np.isneginf(r):
                assert np.isneginf(g), (side, lines[l], g)
            else:
                assert close_enough(g, r), (side, lines[l], g, r, counts[l])


@pytest.mark.parametrize("seed", SEEDS)
def test_sum_equals_the_logsumexp_of_all_kbest_paths(hipopt, seed):
    """every line of 1 .. 1024 derivations: the 1024 best paths are all of them"""
    from carmel_amd.decode import Decoder
    c = case(seed)
    if c["lds_off"]:
        hipopt.set("decode_lds", "0")
    for side, lines, ref, counts, take in cross_checked(c):
        if not take:
            continue
        some = [lines[l] for l in take]
        d = Decoder(c["w"], side=side)
        got = d.sum(some)
        ws, _ = d.decode_kbest(some, 1024)
        d.close()
        for l, g, v in zip(take, got, ws):
            assert len(v) == counts[l], (side, lines[l], len(v), counts[l])
            lse = np.logaddexp.reduce(np.sort(v))
            assert close_enough(g, lse), (side, lines[l], g, lse)
            if counts[l] >= 2:
                assert g > v[0], (side, lines[l], g, v[0])


def test_the_cross_check_takes_enough_lines():
    """(which lines take part is a property of the inputs: test_decode_sum_host.py proves the same number without a device)"""
    n = sum(counts[l] >= 2 for seed in SEEDS for _, _, _, counts, take in cross_checked(case(seed)) for l in take)
    assert n >= 550, n


def test_exact_cases():
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    # test_set_weights_and_fill_lines' machine (0 -1-> 1, 0 -1-> 2, 1 -2-> 2) with a second 0 -1-> 1
    lw = np.log([0.5, 0.25, 0.125, 0.5])
    w = Wfst(3, 2, [0, 0, 0, 1], [1, 2, 1, 2], [1, 1, 1, 2], [3, 4, 3, 5], lw)
    d = Decoder(w)
    lines = [[1, 2], [1], [2], [], [9]]
    s = d.sum(lines)
    two = np.logaddexp(lw[0] + lw[3], lw[2] + lw[3])
    assert close_enough(s[0], two) and s[0] > lw[0] + lw[3]
    assert s[1] == 0.0 + lw[1]  # one derivation: no exp, no log
    assert np.isneginf(s[2]) and np.isneginf(s[3]) and np.isneginf(s[4])
    assert d.last_ms() >= 0
    best, paths = d.decode(lines)  # the entries alternate on one handle
    assert best[0] == lw[0] + (lw[3] + 0.0) and list(paths[0]) == [0, 3]
    ws, _ = d.decode_kbest(lines, 4)
    assert len(ws[0]) == 2
    assert d.sum(lines).tobytes() == s.tobytes()
    new = lw.copy()
    new[2] = -np.inf  # a weight of zero removes the second path: the first one's weights, added in path order
    new[3] = np.log(0.3)
    d.set_weights(new)
    s2 = d.sum(lines)
    assert s2[0] == (0.0 + new[0]) + new[3] and s2[0] != s[0]
    new[0] = -np.inf
    d.set_weights(new)
    assert np.isneginf(d.sum(lines)[0])
    d.close()
    # the empty line, and an epsilon arc into a state that matched arcs enter too: 0 -eps-> 1, 0 -1-> 1, 1 -1-> 1, final 1
    lw = np.log([0.5, 0.25, 0.125])
    w = Wfst(2, 1, [0, 0, 1], [1, 1, 1], [0, 1, 1], [0, 1, 1], lw)
    d = Decoder(w)
    s = d.sum([[], [1]])
    assert s[0] == 0.0 + lw[0]
    assert close_enough(s[1], np.logaddexp(lw[1], lw[0] + lw[2]))
    d.close()


def test_sums_are_deterministic(hipopt):
    """two runs, two chunkings of the batch and the two memory tiers give the same bytes"""
    from carmel_amd.decode import Decoder
    rng = np.random.default_rng(7)
    w = random_machine(rng, 40, 5, 160, p_eps=0.2, cyclic=False)
    lines = lines_for(rng, w, 0, 5, 300)
    d = Decoder(w)
    a = d.sum(lines)
    assert np.isfinite(a).sum() >= 30
    again = d.sum(lines)
    hipopt.set("decode_chunk_bytes", "4096")
    chunked = d.sum(lines)
    hipopt.unset("decode_chunk_bytes")
    hipopt.set("decode_lds", "0")
    glob = d.sum(lines)
    d.close()
    assert a.tobytes() == again.tobytes() == chunked.tobytes() == glob.tobytes()


PPX = (r"product of probs=(\S+), probability=2\^(\S+) per-input-symbol-perplexity\(N=(\d+)\)=2\^(\S+) "
       r"per-line-perplexity\(N=(\d+)\)=2\^(\S+?)")


@pytest.mark.parametrize("name,members", [("cluster", ["cat.fsa.trained.noe", "spellout.fst.trained"]),
                                          ("cipher", ["cipher.wfsa.noe", "cipher.fst.trained"])])
def test_front_end_sum_on_the_tutorial_machines(oracle, golden_dir, tmp_path, name, members):
    gold = decode_expected(golden_dir)[name]
    members = [golden_file(golden_dir, m, tmp_path) for m in members]
    lines = noe(golden_dir, gold["data"])
    text = "".join(l + "\n" for l in lines)
    # the numpy forward on the oracle's composition, the lines on its output side (-r), added in line order
    oc = oracle.OracleCascade([open(m).read() for m in members], remember=False)
    w = oc.composed().arrays()
    cp = oc.corpus("".join("\n%s\n" % l for l in lines + ["no_such_symbol"])).arrays()
    prep = prepare(w["n_states"], w["src"], w["dst"], w["osym"], w["logw"])
    ref = [forward(w["n_states"], w["final"], w["src"], w["dst"], w["osym"], w["logw"],
                   cp["out_sym"][int(cp["out_off"][l]):int(cp["out_off"][l + 1])], prep) for l in range(len(lines) + 1)]
    assert all(r > -np.inf for r in ref[:-1]) and ref[-1] == -np.inf
    total = 0.0
    for r in ref[:-1]:
        total += r
    for form in (["-qbsriWIEk", "1"], ["-qbsriWIE", "--kbest=3"]):
        rc0, out0, err0 = run(form + members, stdin=text)
        rc, out, err = run(form + ["--sum-paths"] + members, stdin=text)
        assert rc0 == 0 and rc == 0, err
        assert out == out0
        rep0, rep = [l for l in err0.split("\n") if l], [l for l in err.split("\n") if l]
        assert len(rep0) == 2 and len(rep) == 5, rep
        assert rep[2:4] == rep0 == [gold["derivations"], gold["viterbi"]]
        vit = re.match(r"Viterbi \(best path\) " + PPX + "$", rep[3])
        tot = re.match(r"Sum \(all paths\) " + PPX + "$", rep[4])
        pre = re.match(PPX + "$", rep[1])
        assert vit and tot and pre, rep
        assert rep[0] == "Derivations found for all %d  inputs." % len(lines)
        assert tot.group(3) == vit.group(3) and tot.group(5) == vit.group(5) == str(len(lines))
        got = printed_ln(tot.group(1))
        assert abs(got - total) <= RTOL * abs(total), (got, total)
        assert got >= printed_ln(vit.group(1))
        assert pre.groups() == tot.groups()
        n_sym = int(tot.group(3))
        assert float(tot.group(2)) == float("%.6g" % (got / 0.6931471805599453))
        assert float(tot.group(4)) == float("%.6g" % (-got / n_sym / 0.6931471805599453))
        assert float(tot.group(6)) == float("%.6g" % (-got / len(lines) / 0.6931471805599453))
    # a line without a derivation: D < n and the "excluding" tail; -timing shows the sum call
    some = lines[:5] + ["no_such_symbol"]
    rc, out, err = run(["-qbsriWIEk", "1", "--sum-paths"] + members, stdin="".join(l + "\n" for l in some), env={"CARMEL_TIMING": "1"})
    assert rc == 0, err
    rep = [l for l in err.split("\n") if l and not l.startswith("timing:")]
    assert "timing: sum " in err and "timing: decode " in err
    assert rep[0] == "Derivations found for all 5  inputs." and rep[2] == "No derivations found for 1 of 6 inputs."
    tail = ", excluding 1 0 probabilities (i.e. real ppx is infinite)."
    assert rep[3].endswith(tail) and rep[4].endswith(tail) and not rep[1].endswith(tail)
    tot = re.match(r"Sum \(all paths\) " + PPX + re.escape(tail) + "$", rep[4])
    assert tot and tot.group(5) == "5", rep[4]
    part = 0.0
    for r in ref[:5]:
        part += r
    assert abs(printed_ln(tot.group(1)) - part) <= RTOL * abs(part)


def test_front_end_refuses_the_sum_over_an_epsilon_cycle(tmp_path):
    """as --kbest over a cycle: the library's error, no output"""
    m = tmp_path / "loop.fst"
    m.write_text("F\n(S (A a x 0.5))\n(A (B *e* *e* 0.5))\n(B (A *e* *e* 0.5))\n(A (F b y 0.5))\n")
    rc1, out1, err1 = run(["-qbsriWIEk", "1", str(m)], stdin="x y\n")
    assert rc1 == 0 and out1 == "a b\n", err1
    rc, out, err = run(["-qbsriWIEk", "1", "--sum-paths", str(m)], stdin="x y\n")
    assert rc != 0 and out == ""
    assert "carmel_hip_decode_sum" in err and "cycle" in err
