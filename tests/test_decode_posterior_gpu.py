"""GPU: batch arc posteriors (carmel_hip_decode_posterior, Decoder.posterior, carmel -b --posterior-counts=FILE;
csrc/decode_posterior.hip) -- random machines against the reference of decode_posterior_ref.py (workload and reference:
decode_posterior_cases.py, what they contain: test_decode_posterior_host.py), exact small cases, lane striding, contended
atomics, the memory tiers and chunking, line weights, errors, and the front end on the tutorial's cluster machines.

Tolerance.  The device's counts against the f64 reference: |device - reference| <= TOL max(1, reference), TOL = 16 E floored at
1e-12.  E_REF below is a constant copied from profiles/measurement_log_decode_posterior.md: the largest discrepancy of the f64
reference against the same reference in longdouble over the random workload (test_decode_posterior_host.py measures it again
and holds it to the logged figure) -- the reference's own error, never the device's.  The factor 16 covers the device's exp and log
differing from libm in the last ulps, and the atomics' order over at most (lines x positions) terms.  The sums are compared bit
for bit with Decoder.sum everywhere."""
import os
import re

import numpy as np
import pytest

from decode_posterior_cases import SEEDS, case, reference
from decode_posterior_ref import net_flow, posterior
from decode_ref import decode_expected, golden_file
from test_decode_gpu import check_random, lines_for, random_machine, run
from test_decode_host import noe

pytestmark = pytest.mark.gpu

E_REF = 5.33e-15  # copied from profiles/measurement_log_decode_posterior.md
TOL = max(16 * E_REF, 1e-12)


def close(got, want):
    """-> the largest |got - want| / max(1, want), asserted within TOL"""
    err = float((np.abs(got - want) / np.maximum(1.0, want)).max()) if len(want) else 0.0
    assert err <= TOL, (err, int((np.abs(got - want) / np.maximum(1.0, want)).argmax()))
    return err


def checked(w, lines, side=0, weights=None, d=None):
    """the device's posterior of the lines: sums bit-equal to Decoder.sum, counts within TOL of the reference; -> (sums, counts)"""
    from carmel_amd.decode import Decoder
    own = d is None
    d = d or Decoder(w, side=side)
    sums, counts = d.posterior(lines, weights)
    assert sums.tobytes() == d.sum(lines).tobytes()
    if own:
        d.close()
    msym = (w.osym if side else w.isym).astype(np.int64)
    rs, rc = posterior(w.n_states, w.final, w.src, w.dst, msym, w.logw, lines, weights)
    assert np.array_equal(sums > -np.inf, rs > -np.inf)
    np.testing.assert_allclose(sums[rs > -np.inf], rs[rs > -np.inf], rtol=0, atol=1e-9)
    close(counts, rc)
    return sums, counts


@pytest.mark.parametrize("seed", SEEDS)
def test_random_machines_against_the_reference(hipopt, seed):
    from carmel_amd._capi import CarmelHipError
    from carmel_amd.decode import Decoder
    c = case(seed)
    w = c["w"]
    if c["lds_off"]:
        hipopt.set("decode_lds", "0")  # a small machine in the global tier
    ref_of = {side: (sums, counts) for side, _, _, sums, counts in reference(seed)}
    worst = 0.0
    for side, lines, ref, _, _ in c["sides"]:
        d = Decoder(w, side=side)
        if ref is None:  # the epsilon arcs of this side have a cycle
            with pytest.raises(CarmelHipError, match="cycle") as e:
                d.posterior(lines)
            assert e.value.code == -5  # CARMEL_HIP_ERR_UNSUPPORTED
            best, paths = d.decode(lines)  # the handle stays usable
            check_random(w, side, lines, best, paths)
            d.close()
            continue
        sums, counts = d.posterior(lines)
        assert sums.tobytes() == d.sum(lines).tobytes()
        d.close()
        rs, rc = ref_of[side]
        assert np.array_equal(sums > -np.inf, rs > -np.inf)
        worst = max(worst, close(counts, rc))
    print("seed %d: worst |device - reference| / max(1, count): %.3g (TOL %.3g)" % (seed, worst, TOL))


def test_exact_cases():
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    # the empty line with an epsilon-only derivation, an epsilon arc into a state that matched arcs enter too:
    # 0 -eps-> 1, 0 -1-> 1, 1 -1-> 1, final 1
    lw = np.log([0.5, 0.25, 0.125])
    w = Wfst(2, 1, [0, 0, 1], [1, 1, 1], [0, 1, 1], [0, 1, 1], lw)
    sums, counts = checked(w, [[]])
    assert sums[0] == lw[0] and counts.tolist() == [1.0, 0.0, 0.0]
    sums, counts = checked(w, [[1]])  # 0.25 against 0.5 x 0.125
    np.testing.assert_allclose(counts, [0.2, 0.8, 0.2], rtol=0, atol=TOL)
    # the empty line without a derivation, no derivation, an unknown symbol: they add nothing to a batch
    w = Wfst(3, 2, [0, 0, 0, 1], [1, 2, 1, 2], [1, 1, 1, 2], [3, 4, 3, 5], np.log([0.5, 0.25, 0.125, 0.5]))
    sums, counts = checked(w, [[], [2], [9], [1, 9]])
    assert np.isneginf(sums).all() and not counts.any()
    _, alone = checked(w, [[1, 2], [1]])
    sums, mixed = checked(w, [[], [1, 2], [2], [9], [1], [1, 9]])
    assert np.isneginf(sums[[0, 2, 3, 5]]).all() and close(mixed, alone) <= TOL
    np.testing.assert_allclose(alone, [0.8, 1.0, 0.2, 1.0], rtol=0, atol=TOL)  # [1] has a single derivation: arc 1 counts 1
    # final_state == 0 with the empty line: Z = 0 and all counts 0
    w0 = Wfst(2, 0, [0, 1], [1, 0], [1, 1], [1, 1], np.log([0.5, 0.5]))
    sums, counts = checked(w0, [[]])
    assert sums[0] == 0.0 and not counts.any()
    sums, counts = checked(w0, [[1, 1], [], [1]])
    assert np.isneginf(sums[2]) and counts.tolist() == [1.0, 1.0]
    # a self-loop used at several positions of one line: 0 -1-> 0 twice (arcs 0, 1), 0 -2-> 1, final 1
    lw = np.log([0.5, 0.25, 0.125])
    w = Wfst(2, 1, [0, 0, 0], [0, 0, 1], [1, 1, 2], [1, 1, 2], lw)
    sums, counts = checked(w, [[1, 1, 1, 2]])
    np.testing.assert_allclose(counts, [2.0, 1.0, 1.0], rtol=0, atol=TOL)
    new = lw.copy()
    new[1] = -np.inf  # set_weights: one loop left, a single derivation; the second call sees it
    d = Decoder(w)
    d.posterior([[1, 1, 1, 2]])
    d.set_weights(new)
    sums, counts = d.posterior([[1, 1, 1, 2]])
    assert sums[0] == d.sum([[1, 1, 1, 2]])[0] and close(counts, np.array([3.0, 0.0, 1.0])) <= TOL
    # the entries alternate on one handle
    best, paths = d.decode([[1, 2]])
    assert list(paths[0]) == [0, 2]
    _, again = d.posterior([[1, 1, 1, 2]])
    _, spaths = d.sample([[1, 2]], 3, seed=1)
    assert all(list(p) == [0, 2] for p in spaths[0])
    _, third = d.posterior([[1, 1, 1, 2]])
    assert close(again, counts) <= TOL and close(third, counts) <= TOL and d.last_ms() >= 0
    d.close()


def test_epsilon_levels_and_both_kinds_of_arc():
    """three epsilon levels 0 -> 1 -> 2 -> 3 (final), every state entered and left by matched and epsilon arcs: an epsilon arc out of
    start in row 0, one into final in row n"""
    from carmel_amd.model import Wfst
    src = [0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3]
    dst = [1, 2, 0, 3, 2, 1, 3, 3, 3, 0, 3, 1]
    sym = [0, 1, 1, 0, 0, 1, 2, 0, 1, 2, 1, 2]
    rng = np.random.default_rng(3)
    w = Wfst(4, 3, src, dst, sym, sym, np.log(rng.uniform(0.1, 1.0, len(src))))
    lines = [[], [1], [2], [1, 1], [1, 2, 1], [2, 2, 1, 1, 2], [1] * 12, [3]]
    sums, counts = checked(w, lines)
    assert (sums[:7] > -np.inf).all() and np.isneginf(sums[7]) and (counts > 0).all()
    net = net_flow(4, np.array(src), np.array(dst), counts)
    assert abs(net[3] - 7) <= 1e-9 and abs(net[0] + 7) <= 1e-9 and np.abs(net[1:3]).max() <= 1e-9


def test_lane_striding():
    """more than 64 source segments of one symbol, with and without epsilon arcs out of them (70 entries in one level)"""
    from carmel_amd.model import Wfst
    n = 70
    s, r, u, t = range(1, n + 1), range(n + 1, 2 * n + 1), 2 * n + 1, 2 * n + 2
    src = [0] * n + [0] * n + list(s) + list(s) + list(r) + [u]
    dst = list(s) + list(r) + [t] * n + [u] * n + [t] * n + [t]
    sym = [1] * (2 * n) + [2] * n + [0] * n + [2] * n + [2]
    o = np.argsort(src, kind="stable")
    rng = np.random.default_rng(4)
    w = Wfst(2 * n + 3, t, np.array(src)[o], np.array(dst)[o], np.array(sym)[o], np.array(sym)[o], np.log(rng.uniform(0.1, 1.0, len(src))))
    sums, counts = checked(w, [[1, 2], [1], [1, 2, 2]])
    assert sums[0] > -np.inf and np.isneginf(sums[1:]).all() and (counts > 0).all() and abs(counts.sum() - 2.0 - counts[w.isym == 0].sum()) <= 1e-9


def test_contended_atomics_and_chunks(hipopt):
    """2 000 copies of one line count 2 000 times one copy; every line alone in its chunk, and the global tier: the same sums bit
    for bit, the counts within tolerance of the one-chunk call"""
    from carmel_amd.decode import Decoder
    rng = np.random.default_rng(7)
    w = random_machine(rng, 40, 5, 160, p_eps=0.2, cyclic=False)
    lines = lines_for(rng, w, 0, 5, 300)
    d = Decoder(w)
    sums, counts = checked(w, lines, d=d)
    assert int((sums > -np.inf).sum()) >= 30
    l = int(np.argmax([len(x) if z > -np.inf else -1 for x, z in zip(lines, sums)]))  # the longest line with a derivation
    _, one = d.posterior([lines[l]])
    many_sums, many = d.posterior([lines[l]] * 2000)
    assert (many_sums == sums[l]).all() and one.sum() >= 1.0
    close(many, 2000 * one)
    zs, zc = d.posterior([])  # zero lines: all counts 0
    assert len(zs) == 0 and len(zc) == w.n_arcs and not zc.any()
    hipopt.set("decode_chunk_bytes", "1")
    s1, c1 = d.posterior(lines)
    hipopt.unset("decode_chunk_bytes")
    hipopt.set("decode_lds", "0")
    s2, c2 = d.posterior(lines)
    d.close()
    assert s1.tobytes() == sums.tobytes() and s2.tobytes() == sums.tobytes()
    close(c1, counts)
    close(c2, counts)


@pytest.mark.parametrize("seed", [1, 5, 10])  # the LDS tier, decode_lds=0, beyond 4096 states
def test_line_weights_against_the_reference(hipopt, seed):
    from carmel_amd.decode import Decoder
    c = case(seed)
    if c["lds_off"]:
        hipopt.set("decode_lds", "0")
    for side, lines, wt, rs, rc in reference(seed, weighted=True):
        assert (wt == 0).any() and (wt % 1 != 0).any()
        d = Decoder(c["w"], side=side)
        sums, counts = d.posterior(lines, wt)
        assert sums.tobytes() == d.sum(lines).tobytes()  # a weight of 0 is legal: the line's sum is still reported
        d.close()
        close(counts, rc)


def test_errors_leave_the_outputs_alone():
    from carmel_amd._capi import CarmelHipError, f64, lib, ptr, u32, u64
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    # an epsilon-cyclic machine: 0 -1-> 1, 1 -eps-> 2, 1 -2-> 3, 2 -eps-> 1
    w = Wfst(4, 3, [0, 1, 1, 2], [1, 2, 3, 1], [1, 0, 2, 0], [1, 0, 2, 0], np.log([0.5, 0.5, 0.5, 0.5]))
    d = Decoder(w)
    off, sym = u64([0, 2]), u32([1, 2])
    sums, counts = np.full(1, 7.5), np.full(4, 7.5)
    rc = lib.carmel_hip_decode_posterior(d._h, 1, ptr(off), ptr(sym), None, ptr(sums), ptr(counts))
    assert rc == -5 and (sums == 7.5).all() and (counts == 7.5).all()  # CARMEL_HIP_ERR_UNSUPPORTED, nothing written
    with pytest.raises(CarmelHipError, match="cycle"):
        d.posterior([[1, 2]])
    best, _ = d.decode([[1, 2]])  # the handle stays usable
    assert best[0] == np.log(0.5) + np.log(0.5)
    d.close()
    w = Wfst(2, 1, [0], [1], [1], [1], np.log([0.5]))
    d = Decoder(w)
    for bad in (-1.0, np.nan, np.inf):
        sums, counts = np.full(2, 7.5), np.full(1, 7.5)
        rc = lib.carmel_hip_decode_posterior(d._h, 2, ptr(u64([0, 1, 2])), ptr(u32([1, 1])), ptr(f64([1.0, bad])), ptr(sums), ptr(counts))
        assert rc == -1 and (sums == 7.5).all() and (counts == 7.5).all(), bad  # CARMEL_HIP_ERR_ARG
    assert lib.carmel_hip_decode_posterior(d._h, 1, ptr(u64([0, 1])), ptr(u32([1])), None, None, None) == -1
    assert lib.carmel_hip_decode_posterior(d._h, 1, ptr(u64([1, 0])), ptr(u32([1])), None, None, ptr(counts)) == -1  # bad offsets
    counts = np.full(1, 7.5)
    assert lib.carmel_hip_decode_posterior(d._h, 2, ptr(u64([0, 1, 2])), ptr(u32([1, 1])), ptr(f64([0.0, 2.5])), None, ptr(counts)) == 0
    assert counts[0] == 2.5  # (a null sum_logw is legal)
    d.close()


ARC = re.compile(r'^\((\S+) \((\S+) (\S+) (\S+) ([^\s!)]+)(!\d*)?\)\)$')


def test_front_end_posterior_counts_on_the_cluster_machines(golden_dir, tmp_path):
    gold = decode_expected(golden_dir)["cluster"]
    members = [golden_file(golden_dir, m, tmp_path) for m in ("cat.fsa.trained.noe", "spellout.fst.trained")]
    lines = noe(golden_dir, gold["data"])[:6]
    text = "".join(l + "\n" for l in lines + ["no_such_symbol"])
    n_with, length = len(lines), sum(len(l.split()) for l in lines)
    counts_file = str(tmp_path / "counts.fst")
    form = ["-qbsriWIEk", "1", "-HJ"]
    rc0, out0, err0 = run(form + members, stdin=text)
    rc, out, err = run(form + ["--posterior-counts=" + counts_file] + members, stdin=text)
    assert rc0 == 0 and rc == 0, err
    assert out == out0 and err == err0  # nothing on stdout or stderr changes
    assert "No derivations found for 1 of %d inputs." % (n_with + 1) in err
    rows = open(counts_file).read().split("\n")
    final, arcs = rows[0], [ARC.match(r) for r in rows[1:] if r]
    assert len(arcs) >= 10 and all(arcs), [r for r, m in zip(rows[1:], arcs) if not m][:3]  # FILE parses, an arc a line
    c = np.array([float(m.group(5)) for m in arcs])  # (a count of 0 is written as the weight 0)
    matched = np.array([m.group(4) != "*e*" for m in arcs])  # -r: the lines are on the output side
    tol = 1e-9 * max(1.0, c.sum())  # (15 significant digits a count)
    assert (c >= 0).all() and (c == 0).any() and abs(c[matched].sum() - length) <= tol, (c[matched].sum(), length)
    net = {}
    for m, x in zip(arcs, c):
        net[m.group(1)] = net.get(m.group(1), 0.0) - x
        net[m.group(2)] = net.get(m.group(2), 0.0) + x
    into_final, rest = net.pop(final), sorted(net.values())
    assert all(abs(x) <= tol for x in rest[1:]), rest[:3]  # flow is conserved at every state but final and one other: start
    assert abs(into_final + rest[0]) <= tol  # what final gains, start loses
    assert abs(into_final - n_with) <= tol or abs(into_final) <= tol  # (nothing, if the composition's start state is its final state)
    # with the other decoders and --sum-paths: their stdout unchanged, the same counts file
    for other in (["-qbsriWIE", "--kbest=2", "-HJ"], ["-qbsriWIE", "--sample-paths=2", "-R", "7", "-HJ", "--sum-paths"]):
        rca, outa, erra = run(other + members, stdin=text)
        rcb, outb, errb = run(other + ["--posterior-counts=" + counts_file + "2"] + members, stdin=text, env={"CARMEL_TIMING": "1"})
        assert rca == 0 and rcb == 0 and outa == outb and "timing: posterior " in errb
        assert [l for l in errb.split("\n") if not l.startswith("timing:")] == erra.split("\n")
        again = np.array([float(ARC.match(r).group(5)) for r in open(counts_file + "2").read().split("\n")[1:] if r])
        assert np.abs(again - c).max() <= tol
