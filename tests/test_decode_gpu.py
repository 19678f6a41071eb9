"""GPU: batch 1-best decoding (carmel -b -k 1; csrc/decode.hip) -- the tutorial's three decode runs against the reference's
recorded output (commands.trace), and random machines against the numpy trellis of tests/decode_ref.py."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from decode_ref import CycleError, decode_expected, golden_file, rescore, viterbi
from test_decode_host import noe

CLI = os.path.join(ROOT, "carmel_amd", "bin", "carmel")
pytestmark = pytest.mark.gpu


def run(args, stdin="", env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([CLI] + list(args), input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       env=e, timeout=1200)
    return p.returncode, p.stdout, p.stderr


def tie_weights(oracle, members, lines, ours, theirs):
    """the weights of two printed -I paths (input strings) of the same output line, each the best over the composed machine's
    paths that spell both strings (an independent numpy Viterbi on the oracle's composition): equal bit for bit = a tie"""
    oc = oracle.OracleCascade([open(m).read() for m in members], remember=False)
    w = oc.composed().arrays()
    out = []
    for line, a, b in zip(lines, ours, theirs):
        res = []
        for inp in (a, b):
            c = oc.corpus("%s\n%s\n" % (inp, line)).arrays()
            isym, osym = c["in_sym"], c["out_sym"]
            # pair symbols: an arc matches (isym_k, osym_k) on the machine's (in, out); the machines here are epsilon-free
            assert len(isym) == len(osym) and not (w["isym"] == 0).any() and not (w["osym"] == 0).any()
            code = w["isym"].astype(np.int64) * (1 << 32) + w["osym"]
            keys = {k: j + 1 for j, k in enumerate(sorted(set(code.tolist())))}
            msym = np.array([keys[k] for k in code.tolist()], np.int64)
            seq = [keys.get(int(i) * (1 << 32) + int(o), -1) for i, o in zip(isym, osym)]
            best, path, _ = viterbi(w["n_states"], w["final"], w["src"], w["dst"], msym, w["logw"], seq)
            res.append(rescore(w["src"], w["dst"], msym, w["logw"], seq, path, w["final"])[1] if path else best)
        out.append(res)
    return out


def check_tutorial(oracle, golden_dir, name, members, tmp_path):
    gold = decode_expected(golden_dir)[name]
    lines = noe(golden_dir, gold["data"])
    rc, out, err = run(["-qbsriWIEk", "1"] + members, stdin="".join(l + "\n" for l in lines))
    assert rc == 0, err
    got = out.split("\n")[:-1]
    assert len(got) == len(gold["paths"])
    diff = [k for k, (a, b) in enumerate(zip(got, gold["paths"])) if a != b]
    if diff:  # every differing line must be a tie, shown on the oracle's composition
        ws = tie_weights(oracle, members, [lines[k] for k in diff], [got[k] for k in diff], [gold["paths"][k] for k in diff])
        for k, (a, b) in zip(diff, ws):
            assert a == b and a > -np.inf, (name, k + 1, got[k], gold["paths"][k], a, b)
    summary = [l for l in err.split("\n") if l]
    return got, summary, gold, diff


@pytest.mark.parametrize("name,members", [("cluster", ["cat.fsa.trained.noe", "spellout.fst.trained"]),
                                          ("cipher", ["cipher.wfsa.noe", "cipher.fst.trained"])])
def test_tutorial_decode_matches_the_reference(oracle, golden_dir, tmp_path, name, members):
    got, summary, gold, diff = check_tutorial(oracle, golden_dir, name, [golden_file(golden_dir, m, tmp_path) for m in members],
                                              tmp_path)
    assert summary == [gold["derivations"], gold["viterbi"]], (summary, diff)


def test_tagging_decode_after_our_em(oracle, golden_dir, tmp_path):
    """the tagging decode used the EM run's tagging.fst.trained (commands:19-22), which the tutorial directory no longer holds:
    train it with the pinned EM run, then decode with the reference's tagging.fsa.trained.noe"""
    g = lambda n: os.path.join(golden_dir, n)
    rc, out, err = run(["--train-cascade", "-HJ", g("tagging.data"), g("tagging.fsa"), g("tagging.fst")],
                       env={"CARMEL_TRAINED_DIR": str(tmp_path)})
    assert rc == 0, err
    members = [golden_file(golden_dir, "tagging.fsa.trained.noe", tmp_path), str(tmp_path / "tagging.fst.trained")]
    got, summary, gold, diff = check_tutorial(oracle, golden_dir, "tagging", members, tmp_path)
    assert summary[0] == gold["derivations"]
    ours = float(summary[1].split("probs=e^")[1].split(",")[0])
    ref = float(gold["viterbi"].split("probs=e^")[1].split(",")[0])
    assert abs(ours - ref) <= 1e-10 * abs(ref), (summary[1], gold["viterbi"])
    print("tagging: %d of 1005 lines differ (ties); summary %s" % (len(diff), "exact" if summary[1] == gold["viterbi"] else summary[1]))


def random_machine(rng, Q, V, n_arcs, p_eps, cyclic, p_zero=0.03):
    src = np.sort(rng.integers(0, Q, n_arcs)).astype(np.uint32)
    dst = rng.integers(0, Q, n_arcs).astype(np.uint32)
    isym = rng.integers(1, V + 1, n_arcs).astype(np.uint32)
    osym = rng.integers(1, V + 1, n_arcs).astype(np.uint32)
    logw = np.log(rng.uniform(0.01, 1.0, n_arcs))
    logw[rng.uniform(size=n_arcs) < p_zero] = -np.inf
    for side_sym in (isym, osym):
        e = rng.uniform(size=n_arcs) < p_eps
        side_sym[e] = 0
    if not cyclic:  # epsilon arcs (on either side) only go forward in state order
        for side_sym in (isym, osym):
            e = side_sym == 0
            bad = e & (dst <= src)
            side_sym[bad] = rng.integers(1, V + 1, int(bad.sum()))
    else:
        k = rng.integers(0, n_arcs)
        isym[k] = osym[k] = 0
        dst[k] = src[k]  # an epsilon self-loop of weight <= 1
    # a spine 0 -> 1 -> ... -> Q-1 so that the final state is reachable
    sp = min(Q - 1, 12)
    hops = np.linspace(0, Q - 1, sp + 1).astype(np.uint32)
    src = np.concatenate([src, hops[:-1]])
    dst = np.concatenate([dst, hops[1:]])
    isym = np.concatenate([isym, rng.integers(1, V + 1, sp)]).astype(np.uint32)
    osym = np.concatenate([osym, rng.integers(1, V + 1, sp)]).astype(np.uint32)
    logw = np.concatenate([logw, np.log(rng.uniform(0.01, 1.0, sp))])
    o = np.argsort(src, kind="stable")
    from carmel_amd.model import Wfst
    return Wfst(Q, Q - 1, src[o], dst[o], isym[o], osym[o], logw[o])


def lines_for(rng, w, side, V, n):
    msym = w.osym if side else w.isym
    out = [[], [V + 7]]  # the empty line; a symbol no arc carries
    while len(out) < n:
        if rng.uniform() < 0.6:  # a random walk's string: often has a derivation
            q, s = 0, []
            for _ in range(rng.integers(1, 14)):
                k = np.nonzero(w.src == q)[0]
                if not len(k):
                    break
                a = rng.choice(k)
                if msym[a]:
                    s.append(int(msym[a]))
                q = w.dst[a]
            out.append(s)
        else:
            out.append([int(x) for x in rng.integers(1, V + 1, rng.integers(0, 9))])
    return out


def check_random(w, side, lines, dec_best, dec_paths):
    msym = (w.osym if side else w.isym).astype(np.int64)
    n_unique = 0
    for line, b, p in zip(lines, dec_best, dec_paths):
        rb, rp, tied = viterbi(w.n_states, w.final, w.src, w.dst, msym, w.logw, line)
        if rp is None:
            assert np.isneginf(b) and len(p) == 0, (line, b)
            continue
        fwd, rev = rescore(w.src, w.dst, msym, w.logw, line, p, w.final)
        assert fwd == rb and rev == b, (line, fwd, rb, rev, b)  # a best path; its weight added from the end
        if not tied:
            assert list(p) == rp, (line, list(p), rp)
            n_unique += 1
    return n_unique


@pytest.mark.parametrize("seed", range(100))
def test_random_machines_against_numpy(hipopt, seed):
    from carmel_amd.decode import Decoder
    rng = np.random.default_rng(seed)
    Q = int(rng.integers(2, 60)) if seed % 10 else int(rng.integers(4100, 4400))  # every tenth: beyond the LDS tier
    if seed % 10 == 5:
        hipopt.set("decode_lds", "0")  # a small machine in the global tier
    V = int(rng.integers(2, 9))
    w = random_machine(rng, Q, V, int(rng.integers(Q, 4 * Q + 20)), p_eps=0.2, cyclic=seed % 3 == 0)
    for side in (0, 1):
        lines = lines_for(rng, w, side, V, 24 if Q < 4096 else 6)
        d = Decoder(w, side=side)
        best, paths = d.decode(lines)
        d.close()
        check_random(w, side, lines, best, paths)


def test_improving_epsilon_cycle_is_an_error():
    from carmel_amd.decode import Decoder
    from carmel_amd._capi import CarmelHipError
    from carmel_amd.model import Wfst
    # 0 -a-> 1, 1 -eps/2-> 2, 2 -eps/1-> 1, 1 -b-> 3: the cycle 1 -> 2 -> 1 has weight 2
    w = Wfst(4, 3, [0, 1, 1, 2], [1, 3, 2, 1], [1, 2, 0, 0], [1, 2, 0, 0], np.log([1.0, 0.5, 2.0, 1.0]))
    with pytest.raises(CycleError):
        viterbi(4, 3, w.src, w.dst, w.isym, w.logw, [1, 2])
    d = Decoder(w)
    with pytest.raises(CarmelHipError, match="best_path_has_cycle"):
        d.decode([[1, 2]])
    d.close()


def test_decoding_is_deterministic(hipopt, golden_dir, tmp_path):
    """two runs, and two chunkings of the batch (one chunk; chunks of a few lines), give the same bytes"""
    args = ["-qbsriIEk", "1", golden_file(golden_dir, "cipher.wfsa.noe", tmp_path), os.path.join(golden_dir, "cipher.fst.trained")]
    text = "".join(l + "\n" for l in noe(golden_dir, "cipher.data.noe")) * 3
    outs = [run(args, stdin=text) for _ in range(2)]
    outs.append(run(args, stdin=text, env={"CARMEL_HIP_DECODE_CHUNK_BYTES": "200000"}))
    assert all(o[0] == 0 for o in outs), outs[0][2]
    assert outs[0] == outs[1] == outs[2]
    from carmel_amd.decode import Decoder
    rng = np.random.default_rng(7)
    w = random_machine(rng, 40, 5, 160, p_eps=0.2, cyclic=False)
    lines = lines_for(rng, w, 0, 5, 300)
    d = Decoder(w)
    a = d.decode(lines)
    hipopt.set("decode_chunk_bytes", "4096")
    b = d.decode(lines)
    d.close()
    assert a[0].tobytes() == b[0].tobytes() and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def test_set_weights_and_fill_lines(golden_dir, tmp_path):
    """carmel_hip_decoder_set_weights takes new weights; a line without derivation prints print_kbest's fill line"""
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    w = Wfst(3, 2, [0, 0, 1], [1, 2, 2], [1, 1, 2], [3, 4, 5], np.log([0.5, 0.25, 0.5]))
    d = Decoder(w)
    best, paths = d.decode([[1, 2], [1], [2]])
    assert best[0] == np.log(0.5) + (np.log(0.5) + 0.0) and list(paths[0]) == [0, 2]
    assert best[1] == np.log(0.25) and list(paths[1]) == [1]
    assert np.isneginf(best[2]) and len(paths[2]) == 0
    d.set_weights([np.log(0.5), np.log(0.25), -np.inf])
    best, paths = d.decode([[1, 2]])
    assert np.isneginf(best[0])
    assert d.last_ms() >= 0
    d.close()
    rc, out, err = run(["-qbsriIEk", "1", golden_file(golden_dir, "cipher.wfsa.noe", tmp_path),
                        os.path.join(golden_dir, "cipher.fst.trained")], stdin="no_such_symbol\n\n")
    assert rc == 0, err
    assert out.split("\n")[0] == "0"
    assert "No derivations found for" in err and "excluding" in err
