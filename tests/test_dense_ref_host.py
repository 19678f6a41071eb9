"""CPU: tests/dense_ref.py, the reference the dense cascade sweep is held against in tests/test_dense_gpu.py, is right --
against an enumeration of all paths, against the oracle's composition and forward-backward, against itself in f64 inside
the tolerance the GPU tests use, and against the one invariant of the counts."""
import numpy as np
import pytest

import dense_ref as dr


def reference(m, dtype=np.longdouble):
    return dr.dense_reference(m.A, m.B, m.start, m.fin, [e[:3] for e in m.eps], m.seqs, m.weights, dtype)


SMALL = [dict(n_plain=2, n_cipher=2), dict(n_plain=3, n_cipher=4, stop_states=2),
         dict(n_plain=3, n_cipher=2, eps_chain=True), dict(n_plain=2, n_cipher=3, eps_chain=2, stop_states=2),
         dict(n_plain=3, n_cipher=4, stop_states=3, eps_chain=True, a_density=0.5, b_density=0.5)]


@pytest.mark.parametrize("k", range(len(SMALL)))
def test_reference_equals_the_enumeration_of_all_paths(k):
    kw = dict(SMALL[k])
    lens = [1, 1, 2, 3, 4, 5, 5]
    m = dr.parse_cascade(*dr.make_cascade(kw.pop("n_plain"), kw.pop("n_cipher"), len(lens), lens, 10 + k, **kw))
    # two strings more that the sampler would not draw: one without a derivation where the model allows one
    V = m.V
    m.seqs += [np.array([V - 1] * 3), np.array([0, V - 1, 0, 0])]
    m.weights += [1.25, 0.75]
    lnp, cnt = reference(m)
    blnp, bcnt = dr.brute_force(m.A, m.B, m.start, m.fin, [e[:3] for e in m.eps], m.seqs, m.weights)
    assert np.isfinite(blnp[:len(lens)].astype(float)).all()
    dr.compare_lnp(lnp, blnp, 1e-15)
    dr.compare_counts(cnt, bcnt, 1e-15)


ORACLE_CASES = [dict(n_plain=5, n_cipher=8), dict(n_plain=11, n_cipher=14, stop_states=5),
                dict(n_plain=7, n_cipher=4, eps_chain=True), dict(n_plain=6, n_cipher=9, eps_chain=5, stop_states=6),
                dict(n_plain=11, n_cipher=14, a_density=0.3), dict(n_plain=9, n_cipher=12, b_density=0.4, stop_states=3),
                dict(n_plain=13, n_cipher=10, a_density=0.3, b_density=0.4, eps_chain=True)]


def channel_counts_of_composed(oracle, lm, ch, composed_counts):
    """composed-arc counts summed per channel arc of the file: every composed arc carries the chain of member arcs it was
    made of (chain_off / chain_param); which arc of the file a parameter is comes from composing the re-tagged texts"""
    oc = oracle.OracleCascade([lm, ch])
    tag = np.rint(np.exp(oracle.OracleCascade(list(dr.retag(lm, ch))).param_logw)).astype(np.int64) - 1
    grp = oc.composed().arrays()["group"]
    out = np.zeros(int(tag[oc.param_member == 1].max()) + 1, np.longdouble)
    for a, c in enumerate(composed_counts):
        for p in oc.chain_param[int(oc.chain_off[grp[a]]):int(oc.chain_off[grp[a] + 1])]:
            if oc.param_member[int(p)] == 1:
                out[tag[int(p)]] += c
    return out


@pytest.mark.parametrize("k", range(len(ORACLE_CASES)))
def test_reference_equals_the_oracle_on_the_composed_cascade(oracle, k):
    kw = dict(ORACLE_CASES[k])
    rng = np.random.default_rng(k)
    lens = [1] + [int(x) for x in rng.integers(1, 20, 24)]
    lm, ch, co = dr.make_cascade(kw.pop("n_plain"), kw.pop("n_cipher"), len(lens), lens, 20 + k, **kw)
    m = dr.parse_cascade(lm, ch, co)
    lnp, cnt = reference(m)
    oc = oracle.OracleCascade([lm, ch])
    r = oracle.estimate(oc.composed(), oc.corpus(co))
    assert r["has_deriv"].all()
    np.testing.assert_allclose(r["pair_logprob"], lnp.astype(float), rtol=1e-7, atol=1e-12)
    got = channel_counts_of_composed(oracle, lm, ch, np.exp(r["counts_ln"]))
    ref = np.zeros(m.n_ch_arcs, np.longdouble)
    np.add.at(ref, m.b_arc[m.b_arc >= 0], cnt[m.b_arc >= 0])
    assert ref.sum() > 0
    np.testing.assert_allclose(got.astype(float), ref.astype(float), rtol=1e-7, atol=1e-12)


@pytest.fixture(scope="module")
def longest():
    (lm, ch, co), L = dr.length_case(29)
    m = dr.parse_cascade(lm, ch, co)
    return m, L, reference(m)


def test_f64_restatement_stays_inside_the_tolerance_on_the_largest_gpu_case(longest):
    """S = 29 at the length ceiling of the unrolled layouts (T = 3689): the bound the GPU tests apply is attainable in f64"""
    m, L, (lnp, cnt) = longest
    assert m.S == 29 and L > 3000 and float(lnp.min()) < -5000
    lnp64, cnt64 = reference(m, np.float64)
    assert lnp64.dtype == np.float64 and cnt64.dtype == np.float64
    tol = dr.tol_rel(m.S, L, sum(len(s) for s in m.seqs))
    e1, e2 = dr.compare_lnp(lnp64, lnp, tol), dr.compare_counts(cnt64, cnt, tol)
    print("f64 against longdouble: ln p %.3g, counts %.3g, bound %.3g" % (e1, e2, tol))
    assert max(e1, e2) > 0  # (the two runs really differ in precision)


def test_counts_sum_to_the_weighted_number_of_positions(longest):
    m, _, (_, cnt) = longest
    cases = [(m, cnt)]
    for k in (1, 4, 6):
        kw = dict(ORACLE_CASES[k])
        lens = list(range(1, 30))
        mk = dr.parse_cascade(*dr.make_cascade(kw.pop("n_plain"), kw.pop("n_cipher"), len(lens), lens, 30 + k, **kw))
        cases.append((mk, reference(mk)[1]))
    for mk, c in cases:
        want = sum(np.longdouble(w) * len(s) for s, w in zip(mk.seqs, mk.weights))
        assert abs(c.sum() - want) <= 1e-14 * want
