"""CPU: the f80 restatement of forest-em's E-step, Viterbi and M-step (forest_ref.py) and its derived tolerances, on the
restatement alone.  On every case of test_forest_f80_gpu.py: the same walk in f64 stays within the tolerance of the f80 walk,
every bound comes out under 1e-10, the corpus has the size it is meant to have (the ballast's nodes, the groups, the slots of the
hot rules, the launch classes recomputed from the 2/3-and-256 rule), and the f64 walk is the oracle's estimate and maximize to
the 1e-8 of the older tests (the f80 run is a reference for precision, the oracle for structure).  On corpora small enough to
enumerate the f80 run equals the sums over the derivations.  And the tolerance sees a subtly wrong walk: each of four is beyond
the bound on some case."""
import numpy as np
import pytest

import dense_ref as dr
import forest_enum as fe
import forest_ref as fr

LD = np.longdouble
F80 = 1e-17  # two f80 evaluations of one quantity in different orders: a few dozen operations of 2^-64 each


def _check_expect(c):
    e, case = c.expect, c.case
    first = 1 if case.with_ballast else 0
    n_groups = (c.n_forests + 63) // 64
    assert not case.with_ballast or max([0] + [int(x) for x in c.nodes[1:]]) <= min(fr.BALLASTS), "an edge forest larger than the smallest ballast"
    if case.with_ballast:
        assert int(c.nodes[0]) == c.n_ballast and not (c.ref[:int(c.node_off[1])] >= 0).any()
        assert c.classes == [(0, n_groups, c.n_ballast, fr.estep_kind(c.n_ballast))]
        assert [fr.estep_kind(n) for n in fr.BALLASTS] == ["ext", "log", "log", "gcol"]
    if "n_forests" in e:
        assert c.n_forests == e["n_forests"]
    if "last_group" in e:
        assert (c.n_forests - 1) % 64 + 1 == e["last_group"]
    if "max_nodes" in e:
        assert int(c.nodes.max()) == e["max_nodes"]
    if "classes" in e:
        assert c.classes == e["classes"]
    ref = c.reference()
    for rule, k in e.get("slots", {}).items():
        assert int(ref.slots[rule]) == k
    if case.name == "hot":  # 64 is the last cold size, 65 the first hot one; 4096 one chunk, 4097 a chunk and a tail of one
        assert sorted(fr.HOT.values()) == [fr.COUNT_HOT, fr.COUNT_HOT + 1, fr.HOT_CHUNK, fr.HOT_CHUNK + 1]
    if case.name.startswith("two-class"):
        assert int(ref.slots[fr.E0]) > 4 * fr.HOT_CHUNK and int(ref.slots[fr.E0]) % fr.HOT_CHUNK  # five chunks, the last a tail
    if "min_zero" in e:
        assert ref.n_zero >= e["min_zero"] and ref.n_zero < c.n_forests
    for f, log10_p in e.get("roots", {}).items():
        assert abs(float(ref.lnp[first + f]) / np.log(10.0) - log10_p) < 5
    if "n_groups" in e:
        assert len(c.group_off) - 1 == e["n_groups"] > 4096 * 256
    if "deep" in e:
        lab, rf, nx = c.forest(first + e["deep"])
        assert len(lab) == 2 * fr.DEEP + 3 and fr.DEEP > 32


@pytest.mark.parametrize("name,n_ballast", fr.PARAMS)
def test_f64_walk_within_the_derived_tolerance_of_the_f80_walk(name, n_ballast):
    c = fr.by_name(name).corpus(n_ballast)
    _check_expect(c)
    ref = c.reference()
    tol = ref.tol
    best, tol_v = fr.viterbi_ref(*c.arrays(), c.logw)
    print("%s/%d: %s, Viterbi %.3g" % (name, n_ballast, tol, tol_v))
    assert tol.lnp < fr.CEILING and tol.counts < fr.CEILING and tol_v < fr.CEILING
    got = c.reference(dtype=np.float64)
    assert got.lnp.dtype == np.float64 and got.counts.dtype == np.float64 and ref.lnp.dtype == LD
    e_lnp, e_counts = dr.compare_lnp(got.lnp, ref.lnp, tol.lnp), dr.compare_counts(got.counts, ref.counts, tol.counts)
    assert got.n_zero == ref.n_zero
    assert abs(got.avg - ref.avg) <= tol.lnp * max(1.0, abs(float(ref.avg)))
    best64, _ = fr.viterbi_ref(*c.arrays(), c.logw, np.float64)
    e_v = dr.compare_lnp(best64, best, tol_v)
    print("    f64 walk: ln p %.3g (%.3f of the bound), counts %.3g (%.3f), Viterbi %.3g (%.3f)" % (
        e_lnp, e_lnp / tol.lnp, e_counts, e_counts / tol.counts, e_v, e_v / tol_v))
    # the M-step from the f64 counts, in f64 arithmetic of its own (numpy's), against the f80 one from the same counts
    prior = 0.01 * c.n_forests
    for add_k, zz in ((0.0, False), (0.5, True)):
        new, delta, mt = fr.mstep_ref(got.counts, prior, c.group_off, c.group_rule, add_k, zz, c.logw)
        assert mt.lnw < fr.CEILING and mt.delta < fr.CEILING
    if not c.oracle_ok:  # (norm groups built directly: the oracle's reader was not given them)
        return
    of = c.oracle_forests()
    oavg, ocounts_ln, opf = of.estimate(0.01)
    np.testing.assert_allclose(got.lnp, opf, rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose((got.counts + prior)[1:], np.exp(ocounts_ln)[1:], rtol=1e-8, atol=1e-12)
    assert float(got.avg) == pytest.approx(oavg, rel=1e-8)
    od = of.maximize()
    new, delta, _ = fr.mstep_ref(got.counts, prior, c.group_off, c.group_rule, 0.0, False, c.logw)
    ow = of.weights()
    fin = np.isfinite(ow)
    assert np.array_equal(fin, np.isfinite(new.astype(np.float64)))
    np.testing.assert_allclose(new.astype(np.float64)[fin], ow[fin], rtol=1e-8, atol=1e-12)
    assert float(delta) == pytest.approx(od, rel=1e-8, abs=1e-12)


def _toy(oracle, ftext, ntext, seed):
    of = oracle.OracleForests(ftext, ntext)
    lw = np.log(np.random.default_rng(seed).uniform(0.05, 1.0, of.n_rules))
    return of, lw


@pytest.mark.parametrize("which", ["toy", "toy2", "shared"])
def test_f80_run_is_the_sum_over_the_enumerated_derivations(oracle, which):
    """counts, ln p and the Viterbi value from forest_enum.derivations: every derivation's weight is the product of its rules'
    (a shared sub-forest expanded once per use), p their sum, a rule's count the weight of its uses over p"""
    if which == "shared":
        c = fr.by_name("shared").corpus(100)
        arrays, lw = c.arrays(), c.logw
    else:
        of, lw = _toy(oracle, *((fe.TOY_FORESTS, fe.TOY_NORM) if which == "toy" else (fe.TOY2_FORESTS, fe.TOY2_NORM)), seed=5)
        arrays = (of.node_off, of.label, of.ref, of.next)
    node_off, label, ref, nxt = arrays
    res = fr.reference(*arrays, lw)
    best, _ = fr.viterbi_ref(*arrays, lw)
    w = np.exp(np.asarray(lw, LD))
    counts = np.zeros(len(lw), LD)
    for f in range(len(node_off) - 1):
        b, e = int(node_off[f]), int(node_off[f + 1])
        ds = fe.derivations(label[b:e], ref[b:e], nxt[b:e], 0)
        assert len(ds) > 1 or which == "shared"
        dw = [np.prod(w[list(d)]) for d in ds]
        p = sum(dw, LD(0))
        assert abs(res.lnp[f] - np.log(p)) <= F80 * max(1, abs(np.log(p)))
        assert abs(best[f] - np.log(max(dw))) <= F80 * max(1, abs(np.log(max(dw))))
        for d, x in zip(ds, dw):
            for r in d:
                counts[r] += x / p
    assert ((counts == 0) == (res.counts == 0)).all()
    nz = counts > 0
    assert (np.abs(res.counts[nz] - counts[nz]) <= F80 * counts[nz]).all()
    if which == "shared":  # a sub-forest used twice in one derivation: the rule's count is twice its posterior
        c = fr.by_name("shared").corpus(100)
        first = int(c.node_off[1])
        post = res.post[1]  # (#1(OR a b) #1) under one AND: forest 1, nodes 2 and 3 are the OR's leaves
        lab = c.label[first:int(c.node_off[2])]
        assert lab[2] == fr.E0 + 1 and abs(post[2] + post[3] - 2) <= F80 * 2


def test_score_parses_a_derivation_against_its_forest(oracle):
    of, lw = _toy(oracle, fe.TOY2_FORESTS, fe.TOY2_NORM, seed=6)
    b, e = int(of.node_off[0]), int(of.node_off[1])  # (OR (1 (OR 4 5 6 7 8)) (2 #1(OR 4 5) #1))
    f = (of.label[b:e], of.ref[b:e], of.next[b:e])
    lw = np.asarray(lw, LD)
    assert fr.score(*f, [(1, 1), (6, 0)], lw) == lw[1] + lw[6]
    assert fr.score(*f, [(2, 2), (4, 0), (5, 0)], lw) == lw[2] + lw[4] + lw[5]
    assert fr.score(*f, [(2, 2), (4, 0)], lw) is None          # one child short
    assert fr.score(*f, [(2, 1), (4, 0), (5, 0)], lw) is None  # a wrong arity
    assert fr.score(*f, [(1, 1), (4, 0), (5, 0)], lw) is None  # not a derivation
    assert fr.score(*f, [(2, 2), (4, 0), (6, 0)], lw) is None
    b, e = int(of.node_off[1]), int(of.node_off[2])  # (OR (3 1 2 4 5 6 7 8 1 2) (3 4))
    f = (of.label[b:e], of.ref[b:e], of.next[b:e])
    assert fr.score(*f, [(3, 1), (4, 0)], lw) == lw[3] + lw[4]


def test_mstep_ref_is_the_loop_over_the_groups():
    c = fr.by_name("mstep").corpus(100)
    counts = c.reference(dtype=np.float64).counts
    sizes = np.diff(c.group_off.astype(np.int64))
    assert {1, 2, 257} <= set(sizes.tolist())
    grouped = set(c.group_rule.tolist())
    used = set(np.nonzero(counts)[0].tolist())
    assert used - grouped and not used & set(fr.ZERO_GROUP + [fr.SINGLE, fr.NO_GROUP])
    for prior in (0.0, 0.01 * c.n_forests):
        for add_k in (0.0, 0.5):
            for zz in (False, True):
                new, delta, _ = fr.mstep_ref(counts, prior, c.group_off, c.group_rule, add_k, zz, c.logw)
                want, d = np.asarray(c.logw, LD).copy(), LD(0)
                with np.errstate(divide="ignore"):
                    for g in range(len(sizes)):
                        rules = c.group_rule[int(c.group_off[g]):int(c.group_off[g + 1])]
                        s = LD(0)
                        for r in rules:
                            s += LD(counts[r]) + LD(prior)
                        for r in rules:
                            x = LD(counts[r]) + LD(prior)
                            v = x / (s + LD(add_k)) if s > 0 else (LD(0) if zz else 1 / LD(len(rules)))
                            d = max(d, abs(v - np.exp(LD(c.logw[r]))))
                            want[r] = np.log(v)
                assert np.array_equal(np.isneginf(want), np.isneginf(new))
                fin = ~np.isneginf(want)
                assert (np.abs(new[fin] - want[fin]) <= F80 * np.maximum(1, np.abs(want[fin]))).all()
                assert abs(delta - d) <= F80
                out = np.ones(c.n_rules, bool)
                out[c.group_rule] = False
                assert out.sum() >= 3 and (new[out] == np.asarray(c.logw, LD)[out]).all()
                if prior == 0.0:  # the all-zero groups: uniform or zero; with a prior they are live through it alone
                    assert np.isneginf(new[fr.SINGLE]) if zz else new[fr.SINGLE] == 0
                else:
                    assert abs(new[fr.ZERO_GROUP[0]] - np.log(LD(0.5) * prior / (prior + LD(add_k) / 2))) <= F80


def _beyond(c, got):
    """the walk `got` is outside the corpus's tolerance of its f80 run (or not even finite)"""
    ref = c.reference()
    try:
        dr.compare_lnp(got.lnp, ref.lnp, ref.tol.lnp)
        dr.compare_counts(got.counts, ref.counts, ref.tol.counts)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("variant,cases", [("shared_once", ["shared"]), ("skip_first_or", ["plain-63", "shared"]),
                                           ("no_guard", ["zero"]), ("weight", ["leaf-only", "plain-63", "range"])])
def test_the_tolerance_sees_a_subtly_wrong_walk(variant, cases):
    """the f64 walk with one thing wrong -- a twice-used shared sub-forest whose outside value is added once; the first child of
    every OR node skipped in the outside pass; the 0/0 guard removed (NaN, or a wrong count); one rule's weight moved by 1e-12
    relative -- is beyond the bound on at least one case, while the right f64 walk is inside it on every case (above)"""
    seen = []
    for name in cases:
        case = fr.by_name(name)
        c = case.corpus(case.ballasts[0])
        assert not _beyond(c, c.reference(dtype=np.float64))
        if variant == "weight":
            lw = c.logw.copy()
            r = int(np.argmax(c.reference().counts))
            lw[r] += np.log1p(1e-12)
            got = c.reference(logw=lw, dtype=np.float64)
        else:
            got = c.reference(dtype=np.float64, variant=variant)
        seen.append(_beyond(c, got))
    assert any(seen), seen
    if variant == "weight":
        assert all(seen[:2])  # (the deep case's bound, 1.5e-11 for ln p, is the one a change of 1e-12 can hide in)
