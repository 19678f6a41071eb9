"""GPU: forest-em's E-step, Viterbi and M-step kernels against their f80 restatement (forest_ref.py), at the tolerances that
module derives from the reference run itself -- under 1e-10 for every case here, where test_forest_gpu.py compares the same
kernels with the f64 oracle at 1e-8 to 1e-10 and atol 1e-12.  Each case keeps that oracle comparison at its old tolerances: the
f80 run is a reference for precision, the oracle for structure.

Kernels.  forest_estimate_ext_kernel (a launch class of at most 100 nodes a forest), forest_estimate_kernel<false> (101 to 150)
and <true> (more), count_reduce_kernel / count_reduce_hot_kernel behind them, forest_viterbi_kernel<false> and <true> (up to
150 nodes, and more), forest_mstep_kernel.  The E-step kernel is chosen per launch class by its largest forest, so every edge
corpus runs behind a ballast forest of exactly 100, 101, 150 and 151 nodes: ext, log, log and gcol, each at its limit (the
root's row is the last row of LDS at 100 and at 150).  Each test asserts from the library's own description of its classes
(`timing: forest class first= count= max_nodes= estep=`) that the intended kernel was given the corpus.
Cases (forest_ref.CASES): plain (groups of 1, 63, 64 and 65 forests), zero (rules at -inf: dead forests, dead branches, the
0/0 guard), shared (a sub-forest used twice under one AND node, references inside referenced sub-forests), shapes (leaf-only
forests, an OR of one child, OR and AND nodes of 254, 255, 256 and 300 children, a spine whose pending children outgrow the
Viterbi walk's 32 LDS stack entries, an OR over bit-identical sub-forests), range (roots near 1e-190, 1e-320 and 1e-480, weights
up to 4, derivations 1e-250 apart, a sum of 70 equal terms), hot (rules of exactly 64, 65, 4096 and 4097 posterior slots), second
(estimate -> maximize -> estimate, against the f80 run at the weights the handle then reports), mstep (groups of 1, 2 and 257
rules); without a ballast: leaf-only (maxlen = 1), two-class-log and two-class-gcol (16 385 forests of three nodes and four of
120 / 151: a log or gcol class of 256 groups and an ext class, one rule of 16 385 slots), mstep-grid-stride (4096 x 256 + 300
singleton groups: the M-step's second trip).

What is compared (dense_ref.compare_lnp / compare_counts): ln p relative to max(1, |ln p|), -inf where the reference has -inf;
counts relative, on the entries above 1e-200 x the total, exact zeros where the reference has them; n_zero; the average (the
ln p bound plus the sum's own roundings: six shuffle adds, an atomic add a group, a divide).  Viterbi: the value within
L_in A_v u of viterbi_ref, every returned derivation a derivation of its forest whose f80 weight is the best within that bound,
the FIRST of bit-identical alternatives.  M-step over prior_count 0 / 0.01 x add_k 0 / 0.5 x zero_zerocounts, from the device's
own counts (so the E-step's rounding stays out of it): ln weights, -inf where the reference has -inf, rules outside every group
bit for bit, the returned largest change.

Measured, observed error / bound, the largest over the cases of a kernel (MI355X):
    forest_estimate_ext_kernel      ln p 0.18 (leaf-only, whose bound is 1e-15)   counts 0.030   errors up to 1.4e-15
    forest_estimate_kernel<false>   ln p 0.011 (zero)                             counts 0.006   errors up to 5e-15 (shapes)
    forest_estimate_kernel<true>    ln p 0.009 (zero)                             counts 0.006   errors up to 5e-15 (shapes)
    forest_viterbi_kernel<false>    value 0.09, <true> 0.065; every returned derivation's f80 weight IS the best
    forest_mstep_kernel             ln weight 0.39 (range), largest change 0.07
Every bound is under 1e-10 (the largest: range, 1.5e-11 for ln p and 6.9e-11 for the counts, where the observed errors are
1.4e-15) and every observed error under its bound.  The bounds are worst cases over a chain in which every rounding falls the
same way; that they still see a subtly wrong kernel -- a shared sub-forest's outside value added once, an OR's first child
skipped, the 0/0 guard gone, a weight off by 1e-12 -- is checked on the f64 walk in test_forest_ref_host.py.  No kernel
defect came out of these cases.

NOT covered, on purpose:
  * the samplers (forest_sample_kernel, forest_sample_multi_kernel, forest_exact.hip) and forest_gibbs_kernel: draws, not sums;
    test_forest_gpu.py and test_bench_workloads_gpu.py hold them to the oracle's chain and to the enumerated distribution.
  * forests beyond 2^20 nodes (refused by carmel_hip_forests_create) and anything near that size: a test of seconds cannot
    build one.
  * classes of 256 or more groups of LARGE forests (the two-class corpora have 256 groups, 252 of whose forests are tiny
    ones): 16 384 forests of 100 nodes and more are the benchmark's size, not a test's.
  * the ext kernel's exponent beyond the range of an int (2^31 halvings); roots that a plain double cannot hold, 1e-320 and
    1e-480, are covered in all three kernels."""
import re

import numpy as np
import pytest

import dense_ref as dr
import forest_ref as fr

pytestmark = pytest.mark.gpu

U = fr.U


def _classes(c, layout):
    """the library's launch classes are the ones recomputed from the corpus, each with the E-step kernel it is meant to get"""
    got = [(int(a), int(b), int(n), k) for a, b, n, k in
           re.findall(r"timing:\s+forest class first=(\d+) count=(\d+) max_nodes=(\d+) estep=(\w+)", layout)]
    assert got == c.classes, (got, c.classes)
    if c.case.with_ballast:
        assert [k for _, _, _, k in got] == [dict(zip(fr.BALLASTS, ("ext", "log", "log", "gcol")))[c.n_ballast]]
    return "+".join("%s(%d)" % (k, n) for _, _, n, k in got)


def _estep(c, hf, logw, kinds, what):
    avg = hf.estimate(per_forest=True)
    lnp, counts = hf.per_forest_logprob.copy(), hf.counts(0.0)
    ref = c.reference(None if logw is c.logw else logw)
    tol = ref.tol
    assert tol.lnp < fr.CEILING and tol.counts < fr.CEILING
    e_lnp, e_counts = dr.compare_lnp(lnp, ref.lnp), dr.compare_counts(counts, ref.counts)
    print("f80 %-18s %-20s %-6s %s | observed ln p %.3g (%.4f of the bound), counts %.3g (%.4f)" % (
        c.case.name, kinds, what, tol, e_lnp, e_lnp / tol.lnp, e_counts, e_counts / tol.counts))
    assert e_lnp <= tol.lnp, "ln p: error %.3g above the bound %.3g" % (e_lnp, tol.lnp)
    assert e_counts <= tol.counts, "counts: relative error %.3g above the bound %.3g" % (e_counts, tol.counts)
    assert hf.n_zero == ref.n_zero
    if ref.n_zero == c.n_forests:
        assert avg == -np.inf
    else:
        n_groups = (c.n_forests + 63) // 64
        assert abs(avg - ref.avg) <= (tol.lnp + (7 + n_groups) * U) * max(1.0, abs(float(ref.avg)))
    if c.oracle_ok:  # ... and the oracle, for gross errors, at the tolerances of test_forest_gpu.py
        oavg, ocounts_ln, opf = c.oracle_forests(logw).estimate(0.0)
        assert avg == pytest.approx(oavg, rel=1e-10)
        np.testing.assert_allclose(lnp, opf, rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(counts[1:], np.exp(ocounts_ln)[1:], rtol=1e-8, atol=1e-12)
    return counts


def _viterbi(c, hf, logw, kinds):
    best = hf.viterbi()
    ref_best, tol_v = fr.viterbi_ref(*c.arrays(), logw)
    assert tol_v < fr.CEILING
    e_v = dr.compare_lnp(best, ref_best)
    worst = 0.0
    first = 1 if c.case.with_ballast else 0
    for f in range(0, c.n_forests, c.case.every):
        d = hf.best_derivation(f)
        s = fr.score(*c.forest(f), d, logw)
        assert s is not None, "forest %d: %r is not a derivation of it" % (f, d)
        if np.isneginf(ref_best[f]):
            assert np.isneginf(s)
            continue
        e = float(abs(s - ref_best[f]) / max(1, abs(ref_best[f])))
        assert e <= tol_v, "forest %d: the returned derivation is %.3g below the best, bound %.3g" % (f, e, tol_v)
        worst = max(worst, e)
    print("f80 %-18s %-20s viterbi<%s> bound %.3g | observed value %.3g (%.4f of the bound), derivations %.3g (%.4f)" % (
        c.case.name, kinds, "true" if "gcol" in kinds.split("+")[0] else "false", tol_v, e_v, e_v / tol_v, worst, worst / tol_v))
    assert e_v <= tol_v, "Viterbi: error %.3g above the bound %.3g" % (e_v, tol_v)
    if logw is c.logw:
        for idx, want in c.expect.get("first_best", {}).items():  # bit-identical alternatives: the first (forest.hpp:547)
            assert hf.best_derivation(first + idx) == want
        if "deep" in c.expect:  # DEEP pending children on the walk's stack, whose LDS part holds 32
            assert len(hf.best_derivation(first + c.expect["deep"])) == 2 * fr.DEEP + 1


def _mstep(c, hf, old, counts):
    """the grid of the M-step's options from the counts the device holds (hf.counts(0.0) is an exact copy of them)"""
    out = np.ones(c.n_rules, bool)
    out[c.group_rule] = False
    worst = [0.0, 0.0]
    for prior_count in (0.0, 0.01):
        for add_k in (0.0, 0.5):
            for zz in (False, True):
                hf.set_weights(old)
                d = hf.maximize(prior_count=prior_count, add_k=add_k, zero_zerocounts=zz)
                got = hf.weights()
                new, delta, mt = fr.mstep_ref(counts, prior_count * float(c.n_forests), c.group_off, c.group_rule, add_k, zz, old)
                assert mt.lnw < fr.CEILING and mt.delta < fr.CEILING
                dead = np.isneginf(new)
                assert np.array_equal(np.isneginf(got), dead) and np.isfinite(got[~dead]).all()
                e_w = float(np.abs(got[~dead] - new[~dead]).max()) if (~dead).any() else 0.0
                e_d = float(abs(d - delta))
                assert e_w <= mt.lnw, "ln weight: error %.3g above the bound %.3g (%r)" % (e_w, mt.lnw, (prior_count, add_k, zz))
                assert e_d <= mt.delta, "max change: error %.3g above the bound %.3g (%r)" % (e_d, mt.delta, (prior_count, add_k, zz))
                assert np.array_equal(got[out].view(np.uint64), np.asarray(old)[out].view(np.uint64))
                worst = [max(worst[0], e_w / mt.lnw), max(worst[1], e_d / mt.delta)]
    print("f80 %-18s mstep %s | observed ln weight %.4f of the bound, max change %.4f" % (c.case.name, mt, worst[0], worst[1]))
    hf.set_weights(old)


@pytest.mark.parametrize("name,n_ballast", fr.PARAMS)
def test_forest_kernels_within_the_derived_tolerance_of_the_f80_run(name, n_ballast, hipopt, capfd):
    from carmel_amd.forests import HipForests
    case = fr.by_name(name)
    c = case.corpus(n_ballast)
    hipopt.set("timing", "1")
    capfd.readouterr()
    hf = HipForests(*c.arrays(), c.n_rules, c.logw, c.group_off, c.group_rule)
    layout = capfd.readouterr().err
    try:
        kinds = _classes(c, layout)
        counts = _estep(c, hf, c.logw, kinds, "first")
        _viterbi(c, hf, c.logw, kinds)
        _mstep(c, hf, c.logw, counts)
        if case.second:
            hf.estimate()
            hf.maximize(prior_count=0.01)
            logw = hf.weights()
            assert not np.array_equal(logw, c.logw)
            _estep(c, hf, logw, kinds, "second")
            _viterbi(c, hf, logw, kinds)
    finally:
        hf.close()
