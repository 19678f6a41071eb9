"""GPU: batch pair arc posteriors (carmel_hip_decode_pairs_posterior, Decoder.posterior_pairs, carmel -b --pair-lines=FILE
--pair-counts=FILE; csrc/decode_pairs_posterior.hip) -- random machines against the reference of decode_pairs_posterior_ref.py
(workload and reference: decode_pairs_posterior_cases.py, why the reference is right: test_decode_pairs_posterior_host.py),
exact small cases, lane striding, contended atomics, the memory tiers and chunking, the reductions to the one-sided posteriors,
the trainer's counts as an independent device route, pair weights, errors, handle state, and the front end on the epron-jpron
fixture.

Tolerance.  The device's counts against the f64 reference: |device - reference| <= TOL max(1, reference), TOL = 16 E floored at
1e-12.  E_REF below is a constant copied from profiles/measurement_log_decode_pairs_posterior.md: the largest discrepancy of the
f64 reference against the same reference in longdouble over the random workload (test_decode_pairs_posterior_host.py measures it
again and holds it to the logged figure) -- the reference's own error, never the device's.  The factor 16 is
test_decode_posterior_gpu.py's, for the same reasons: the device's exp and log differ from libm in the last ulps, and the atomics'
order over at most (pairs x cells) terms.  The sums are compared bit for bit with Decoder.sum_pairs everywhere."""
import os

import numpy as np
import pytest

from decode_pairs_cases import SEEDS, case, pairs_for, sides
from decode_pairs_posterior_cases import reference
from decode_pairs_posterior_ref import posterior
from decode_pairs_ref import Prepared
from decode_posterior_ref import net_flow
from test_decode_gpu import lines_for, random_machine, run
from test_decode_kbest_gpu import printed_ln
from test_decode_pairs_gpu import identity_machine
from test_decode_posterior_gpu import ARC

pytestmark = pytest.mark.gpu

E_REF = 7.11e-15  # copied from profiles/measurement_log_decode_pairs_posterior.md
TOL = max(16 * E_REF, 1e-12)
ERR_ARG, ERR_UNSUPPORTED = -1, -5


def close(got, want):
    """-> the largest |got - want| / max(1, want), asserted within TOL"""
    err = float((np.abs(got - want) / np.maximum(1.0, want)).max()) if len(want) else 0.0
    assert err <= TOL, (err, int((np.abs(got - want) / np.maximum(1.0, want)).argmax()))
    return err


def split(pairs):
    return [x for x, _ in pairs], [y for _, y in pairs]


def checked(w, pairs, side=0, weights=None, d=None):
    """the device's posterior of the pairs: sums bit-equal to Decoder.sum_pairs, counts within TOL of the reference;
    -> (sums, counts)"""
    from carmel_amd.decode import Decoder
    own = d is None
    d = d or Decoder(w, side=side)
    xs, ys = split(pairs)
    sums, counts = d.posterior_pairs(xs, ys, weights)
    assert sums.tobytes() == d.sum_pairs(xs, ys).tobytes()
    if own:
        d.close()
    msym, osym = sides(w, side)
    rs, rc = posterior(Prepared(w.n_states, w.final, w.src, w.dst, msym, osym, w.logw), pairs, weights)
    assert np.array_equal(sums > -np.inf, rs > -np.inf)
    np.testing.assert_allclose(sums[rs > -np.inf], rs[rs > -np.inf], rtol=0, atol=1e-9)
    close(counts, rc)
    return sums, counts


@pytest.mark.parametrize("seed", SEEDS)
def test_random_machines_against_the_reference(hipopt, seed):
    from carmel_amd._capi import CarmelHipError
    from carmel_amd.decode import Decoder
    c = case(seed)
    if c["lds_off"]:
        hipopt.set("decode_lds", "0")  # a small machine in the global tier
    xs, ys = split(c["pairs"])
    d = Decoder(c["w"], side=c["side"])
    if c["P"] is None:  # the 00 arcs have a cycle: refused, and the handle stays usable
        with pytest.raises(CarmelHipError, match="cycle") as e:
            d.posterior_pairs(xs, ys)
        assert e.value.code == ERR_UNSUPPORTED
        best, _ = d.decode(xs)
        assert best.shape == (len(xs),)
        d.close()
        return
    sums, counts = d.posterior_pairs(xs, ys)
    assert sums.tobytes() == d.sum_pairs(xs, ys).tobytes()
    d.close()
    _, rs, rc = reference(seed)
    assert np.array_equal(sums > -np.inf, rs > -np.inf)
    print("seed %d: worst |device - reference| / max(1, count): %.3g (TOL %.3g)" % (seed, close(counts, rc), TOL))


def test_exact_cases():
    from carmel_amd.model import Wfst
    h = np.log(0.5)
    # ([], []) with a single 00 derivation
    w = Wfst(2, 1, [0], [1], [0], [0], [h])
    sums, counts = checked(w, [([], [])])
    assert sums[0] == h and counts.tolist() == [1.0]
    # final = start with the empty pair: Z = 0 and all counts 0
    w0 = Wfst(2, 0, [0, 1], [1, 0], [1, 1], [2, 2], [h, h])
    sums, counts = checked(w0, [([], [])])
    assert sums[0] == 0.0 and not counts.any()
    sums, counts = checked(w0, [([1, 1], [2, 2]), ([], []), ([1], [2])])
    assert np.isneginf(sums[2]) and counts.tolist() == [1.0, 1.0]
    # MM against M0-then-0M for ([1], [2]), 0.25 against 0.5 x 0.125 (the one-sided exact case, rebuilt for pairs):
    # 0 -1:2-> 1, 0 -1:e-> 2, 2 -e:2-> 1, final 1
    w = Wfst(3, 1, [0, 0, 2], [1, 2, 1], [1, 1, 0], [2, 0, 2], np.log([0.25, 0.5, 0.125]))
    sums, counts = checked(w, [([1], [2])])
    np.testing.assert_allclose(counts, [0.8, 0.2, 0.2], rtol=0, atol=TOL)
    # an insertion loop used twice: 0 -1:2-> 1, 1 -e:3-> 1 on ([1], [2, 3, 3])
    w = Wfst(2, 1, [0, 1], [1, 1], [1, 0], [2, 3], np.log([0.3, 0.5]))
    sums, counts = checked(w, [([1], [2, 3, 3])])
    np.testing.assert_allclose(counts, [1.0, 2.0], rtol=0, atol=TOL)
    # n > m, n < m, x empty, y empty (the diagonal's index changes side): one state, a loop of each class but 00
    w = Wfst(1, 0, [0, 0, 0, 0], [0, 0, 0, 0], [1, 0, 1, 1], [0, 2, 2, 2], np.log([0.5, 0.3, 0.2, 1.0]) + [0, 0, 0, -np.inf])
    pairs = [([], []), ([1], []), ([], [2]), ([1], [2] * 5), ([1] * 5, [2]), ([1], [2]), ([1] * 3, [2] * 3), ([1] * 4, []), ([], [2] * 4)]
    for p in pairs:
        sums, counts = checked(w, [p])
        assert abs(counts[0] + counts[2] - len(p[0])) <= 1e-9 and abs(counts[1] + counts[2] - len(p[1])) <= 1e-9 and counts[3] == 0
    sums, counts = checked(w, pairs)
    assert np.isfinite(sums).all()
    # an unknown symbol on either side and pairs without a derivation add nothing to a batch
    w = Wfst(3, 2, [0, 0, 0, 1], [1, 2, 1, 2], [1, 1, 1, 2], [3, 4, 3, 5], np.log([0.5, 0.25, 0.125, 0.5]))
    sums, counts = checked(w, [([], []), ([2], [5]), ([9], [3]), ([1], [9]), ([1, 2], [3]), ([1], [3, 5])])
    assert np.isneginf(sums).all() and not counts.any()
    _, alone = checked(w, [([1, 2], [3, 5]), ([1], [4])])
    sums, mixed = checked(w, [([], []), ([1, 2], [3, 5]), ([2], [5]), ([9], [3]), ([1], [4]), ([1], [9])])
    assert np.isneginf(sums[[0, 2, 3, 5]]).all() and close(mixed, alone) <= TOL
    np.testing.assert_allclose(alone, [0.8, 1.0, 0.2, 1.0], rtol=0, atol=TOL)


def test_three_00_levels_and_all_kinds_of_arc():
    """00 levels 0 -> 1 -> 2 -> 3 (final), every state entered and left by arcs of all four kinds: a 00 arc out of the start in
    cell (0, 0), one into final in cell (n, m)"""
    from carmel_amd.model import Wfst
    src = [0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3]
    dst = [1, 2, 0, 3, 1, 2, 1, 3, 0, 3, 3, 0, 2, 3, 1, 2]
    isym = [0, 1, 1, 0, 0, 0, 1, 2, 0, 0, 1, 2, 0, 1, 2, 1]
    osym = [0, 1, 0, 0, 2, 0, 2, 0, 1, 0, 1, 2, 1, 0, 2, 2]
    rng = np.random.default_rng(3)
    w = Wfst(4, 3, src, dst, isym, osym, np.log(rng.uniform(0.1, 1.0, len(src))))
    assert Prepared(4, 3, w.src, w.dst, w.isym, w.osym, w.logw).n_levels == 3
    pairs = [([], []), ([1], []), ([], [2]), ([1, 1], [1]), ([1, 2, 1], [2, 1, 2, 1]), ([2, 2, 1, 1, 2], [1, 2]), ([1] * 9, [2] * 7),
             ([3], [1])]
    for side in (0, 1):
        ps = [(y, x) if side else (x, y) for x, y in pairs]
        sums, counts = checked(w, ps, side=side)
        k = int((sums > -np.inf).sum())
        assert k == 6 and np.isneginf(sums[[5, 7]]).all() and (counts > 0).all()
        net = net_flow(4, np.array(src), np.array(dst), counts)
        assert abs(net[3] - k) <= 1e-9 and abs(net[0] + k) <= 1e-9 and np.abs(net[1:3]).max() <= 1e-9


@pytest.mark.parametrize("other", ["same", "half", "none"])
def test_lane_striding_over_segments_and_entries(other):
    """more than 64 source segments of one symbol, with and without epsilon arcs out of them, and 70 entries in one 00 level"""
    from carmel_amd.model import Wfst
    n = 70
    s, r, u, t = range(1, n + 1), range(n + 1, 2 * n + 1), 2 * n + 1, 2 * n + 2
    src = [0] * n + [0] * n + list(s) + list(s) + list(r) + [u]
    dst = list(s) + list(r) + [t] * n + [u] * n + [t] * n + [t]
    sym = np.array([1] * (2 * n) + [2] * n + [0] * n + [2] * n + [2])
    osym = sym.copy()
    if other == "half":  # the arcs labelled 2 from the r states are M0: ([1, 2], [1]) runs through them alone
        osym[4 * n:5 * n] = 0
    if other == "none":
        osym[:] = 0
    o = np.argsort(src, kind="stable")
    rng = np.random.default_rng(4)
    w = Wfst(2 * n + 3, t, np.array(src)[o], np.array(dst)[o], sym[o], osym[o], np.log(rng.uniform(0.1, 1.0, len(src))))
    ys = {"same": [[1, 2], [1], [1, 2, 2]], "half": [[1, 2], [1], [1]], "none": [[], [], []]}[other]
    sums, counts = checked(w, list(zip([[1, 2], [1, 2], [1, 2, 2]], ys)))
    has = sums > -np.inf
    assert has.tolist() == [True, other != "same", False]
    assert (counts > 0).all() and abs(counts[w.isym != 0].sum() - 2.0 * has.sum()) <= 1e-9


def test_more_than_64_nodes_on_a_diagonal():
    rng = np.random.default_rng(77)
    w = random_machine(rng, 90, 3, 500, p_eps=0.3, cyclic=False)
    pairs = [p for p in pairs_for(rng, w, 0, 3, 12) if min(len(p[0]), len(p[1])) >= 1]
    sums, counts = checked(w, pairs)
    assert int((sums > -np.inf).sum()) >= 4


def test_contended_atomics_chunks_and_tiers(hipopt):
    """2 000 copies of one pair count 2 000 times one copy; zero pairs; every pair alone in its chunk, and the global tier: the
    same sums bit for bit, the counts within tolerance of the one-chunk LDS call"""
    from carmel_amd.decode import Decoder
    rng = np.random.default_rng(8)
    w = random_machine(rng, 30, 4, 150, p_eps=0.3, cyclic=False)
    pairs = pairs_for(rng, w, 0, 4, 60)
    xs, ys = split(pairs)
    d = Decoder(w)
    sums, counts = checked(w, pairs, d=d)
    assert int((sums > -np.inf).sum()) >= 20
    l = int(np.argmax([len(x) + len(y) if z > -np.inf else -1 for (x, y), z in zip(pairs, sums)]))  # the longest with a derivation
    _, one = d.posterior_pairs([xs[l]], [ys[l]])
    many_sums, many = d.posterior_pairs([xs[l]] * 2000, [ys[l]] * 2000)
    assert (many_sums == sums[l]).all() and one.sum() >= 1.0
    close(many, 2000 * one)
    zs, zc = d.posterior_pairs([], [])  # zero pairs: all counts 0
    assert len(zs) == 0 and len(zc) == w.n_arcs and not zc.any()
    hipopt.set("decode_chunk_bytes", "1")
    s1, c1 = d.posterior_pairs(xs, ys)
    hipopt.unset("decode_chunk_bytes")
    hipopt.set("decode_lds", "0")
    s2, c2 = d.posterior_pairs(xs, ys)
    d.close()
    assert s1.tobytes() == sums.tobytes() and s2.tobytes() == sums.tobytes()
    close(c1, counts)
    close(c2, counts)


@pytest.mark.parametrize("other_epsilon", [False, True])
@pytest.mark.parametrize("Q", [37, 4200])
def test_pairs_reduce_to_the_one_sided_posteriors(Q, other_epsilon):
    """osym = isym on pairs (x, x), or an other side of epsilons on pairs (x, []): carmel_hip_decode_sum's sums bit for bit,
    carmel_hip_decode_posterior's counts within TOL"""
    from carmel_amd.decode import Decoder
    rng = np.random.default_rng(31 + Q)
    w = identity_machine(rng, Q, 4, other_epsilon)
    n = 24 if Q < 4096 else 6
    lines = lines_for(rng, w, 0, 4, n // 2) + [x for x, _ in pairs_for(rng, w, 0, 4, n // 2 + 3)[3:]]
    d = Decoder(w)
    sums, counts = d.posterior(lines)
    other = [[] for _ in lines] if other_epsilon else lines
    psums, pcounts = d.posterior_pairs(lines, other)
    assert d.sum(lines).tobytes() == psums.tobytes() == sums.tobytes()
    d.close()
    assert np.isfinite(sums).sum() >= 3 and counts.sum() >= 3
    close(pcounts, counts)


@pytest.mark.parametrize("seed", [1, 2, 4])
def test_the_trainer_gives_the_same_counts(seed):
    """the same machine and pairs through carmel_hip_estimate (a derivation lattice per pair): a device route that shares no
    code with this one, held to the tolerance tests/test_gpu_parity.py holds the trainer's counts to"""
    from carmel_amd.decode import Decoder
    from carmel_amd.model import NORM_NONE, Corpus
    from carmel_amd.trainer import HipForwardBackward
    from test_gpu_parity import RTOL
    c = case(seed)
    assert c["P"] is not None
    pairs = c["pairs"]
    corpus = Corpus.from_lists([(y, x) if c["side"] else (x, y) for x, y in pairs])
    fb = HipForwardBackward(c["w"], corpus, norm_group=NORM_NONE, normalize_first=False)
    fb.estimate()
    want = fb.counts()
    fb.close()
    d = Decoder(c["w"], side=c["side"])
    sums, counts = d.posterior_pairs(*split(pairs))
    d.close()
    assert np.isfinite(sums).sum() >= 4 and want.sum() >= 4
    np.testing.assert_allclose(counts, want, rtol=RTOL, atol=1e-14)


@pytest.mark.parametrize("seed", [1, 5, 20])  # the LDS tier, decode_lds=0, beyond 4096 states
def test_pair_weights_against_the_reference(hipopt, seed):
    from carmel_amd.decode import Decoder
    c = case(seed)
    assert c["P"] is not None
    if c["lds_off"]:
        hipopt.set("decode_lds", "0")
    wt, rs, rc = reference(seed, weighted=True)
    assert (wt == 0).any() and (wt % 1 != 0).any()
    xs, ys = split(c["pairs"])
    d = Decoder(c["w"], side=c["side"])
    sums, counts = d.posterior_pairs(xs, ys, wt)
    assert sums.tobytes() == d.sum_pairs(xs, ys).tobytes()  # a weight of 0 is legal: the pair's sum is still reported
    d.close()
    close(counts, rc)


def test_errors_leave_the_outputs_alone():
    from carmel_amd._capi import CarmelHipError, f64, lib, ptr, u32, u64
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    F = lib.carmel_hip_decode_pairs_posterior
    # a 00 cycle 1 -> 2 -> 1
    w = Wfst(4, 3, [0, 1, 1, 2], [1, 3, 2, 1], [1, 2, 0, 0], [1, 2, 0, 0], np.log([1.0, 0.5, 0.5, 0.5]))
    d = Decoder(w)
    off, sym = u64([0, 2]), u32([1, 2])
    sums, counts = np.full(1, 7.5), np.full(4, 7.5)
    rc = F(d._h, 1, ptr(off), ptr(sym), ptr(off), ptr(sym), None, ptr(sums), ptr(counts))
    assert rc == ERR_UNSUPPORTED and (sums == 7.5).all() and (counts == 7.5).all()  # nothing written
    with pytest.raises(CarmelHipError, match="cycle") as e:
        d.posterior_pairs([[1, 2]], [[1, 2]])
    assert "1 -> 2 -> 1" in str(e.value) or "2 -> 1 -> 2" in str(e.value)
    best, _ = d.decode([[1, 2]])  # the handle stays usable
    assert best[0] == np.log(0.5)
    d.close()
    w = Wfst(2, 1, [0], [1], [1], [2], np.log([0.5]))
    d = Decoder(w)
    off2, x2, y2 = u64([0, 1, 2]), u32([1, 1]), u32([2, 2])
    for bad in (-1.0, np.nan, np.inf):
        sums, counts = np.full(2, 7.5), np.full(1, 7.5)
        rc = F(d._h, 2, ptr(off2), ptr(x2), ptr(off2), ptr(y2), ptr(f64([1.0, bad])), ptr(sums), ptr(counts))
        assert rc == ERR_ARG and (sums == 7.5).all() and (counts == 7.5).all(), bad
    off, x, y, rev = u64([0, 1]), u32([1]), u32([2]), u64([1, 0])
    sums, counts = np.full(1, 7.5), np.full(1, 7.5)
    for args in ((None, 1, ptr(off), ptr(x), ptr(off), ptr(y)), (d._h, 1, None, ptr(x), ptr(off), ptr(y)),
                 (d._h, 1, ptr(off), ptr(x), None, ptr(y)), (d._h, 1, ptr(off), None, ptr(off), ptr(y)),
                 (d._h, 1, ptr(off), ptr(x), ptr(off), None), (d._h, 1, ptr(rev), ptr(x), ptr(off), ptr(y)),
                 (d._h, 1, ptr(off), ptr(x), ptr(rev), ptr(y)), (d._h, 1 << 32, ptr(off), ptr(x), ptr(off), ptr(y))):
        assert F(*args, None, ptr(sums), ptr(counts)) == ERR_ARG, args
        assert (sums == 7.5).all() and (counts == 7.5).all()
    assert F(d._h, 1, ptr(off), ptr(x), ptr(off), ptr(y), None, ptr(sums), None) == ERR_ARG and sums[0] == 7.5
    assert b"carmel_hip_decode_pairs_posterior" in lib.carmel_hip_last_error()
    counts = np.full(1, 7.5)
    assert F(d._h, 2, ptr(off2), ptr(x2), ptr(off2), ptr(y2), ptr(f64([0.0, 2.5])), None, ptr(counts)) == 0
    assert counts[0] == 2.5  # (a null sum_logw is legal)
    d.close()


def test_set_weights_and_the_other_entry_points_on_one_handle():
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    # 0 -1:2-> 0 twice (arcs 0, 1), 0 -2:e-> 1, final 1
    lw = np.log([0.5, 0.25, 0.125])
    w = Wfst(2, 1, [0, 0, 0], [0, 0, 1], [1, 1, 2], [2, 2, 0], lw)
    x, y = [1, 1, 1, 2], [2, 2, 2]
    d = Decoder(w)
    sums, counts = checked(w, [(x, y)], d=d)
    np.testing.assert_allclose(counts, [2.0, 1.0, 1.0], rtol=0, atol=TOL)
    assert d.last_ms() >= 0
    new = lw.copy()
    new[1] = -np.inf  # one loop left, a single derivation: the next call sees it
    d.set_weights(new)
    sums, counts = d.posterior_pairs([x], [y])
    assert sums[0] == d.sum_pairs([x], [y])[0] and close(counts, np.array([3.0, 0.0, 1.0])) <= TOL
    # the entries alternate on one handle, every result unchanged
    calls = {"decode": lambda: d.decode([x]), "posterior": lambda: d.posterior([x]), "sample": lambda: d.sample([x], 3, seed=1),
             "decode_pairs": lambda: d.decode_pairs([x], [y]), "sum_pairs": lambda: d.sum_pairs([x], [y])}
    flat = lambda r: [flat(a) for a in r] if isinstance(r, (tuple, list)) else np.asarray(r).tolist()
    first = {name: flat(call()) for name, call in calls.items()}
    for name, call in calls.items():
        again_sums, again = d.posterior_pairs([x], [y])
        assert again_sums.tobytes() == sums.tobytes() and close(again, counts) <= TOL, name
        assert flat(call()) == first[name], name
    again_sums, again = d.posterior_pairs([x], [y])
    assert again_sums.tobytes() == sums.tobytes() and close(again, counts) <= TOL
    d.close()


def test_front_end_pair_counts_on_the_epron_jpron_pairs(oracle, golden_dir, tmp_path):
    from carmel_amd.model import NORM_NONE, Corpus, Wfst
    from carmel_amd.trainer import HipForwardBackward
    fst, data = os.path.join(golden_dir, "epron-jpron.fst"), os.path.join(golden_dir, "epron-jpron.data")
    rows = open(data).read().split("\n")[:-1]
    ins, outs = rows[0::2], rows[1::2]
    E, J, A, K = tmp_path / "E", tmp_path / "J", tmp_path / "A", tmp_path / "K"
    E.write_text("".join(l + "\n" for l in ins))
    J.write_text("".join(l + "\n" for l in outs))
    form = ["-qbIEk", "1", "-HJ", "--sum-paths", "--pair-lines=%s" % J, "--pair-alignments=%s" % A]
    rc0, out0, err0 = run(form + [str(E), fst])
    aligned0 = A.read_text()
    rc, out, err = run(form + ["--pair-counts=%s" % K, str(E), fst], env={"CARMEL_TIMING": "1"})
    assert rc0 == 0 and rc == 0, err
    assert out == out0 and A.read_text() == aligned0 and "timing: pairs posterior " in err
    assert [l for l in err.split("\n") if not l.startswith("timing:")] == err0.split("\n")  # nothing else changes
    assert "Derivations found for all %d inputs." % len(ins) in err  # every pair has a derivation
    lines = K.read_text().split("\n")
    final, arcs = lines[0], [ARC.match(r) for r in lines[1:] if r]
    assert len(arcs) >= 10 and all(arcs), [r for r, m in zip(lines[1:], arcs) if not m][:3]  # FILE parses, an arc a line
    c = np.array([float(m.group(5)) for m in arcs])  # (a count of 0 is written as the weight 0)
    tol = 1e-9 * max(1.0, c.sum())  # (15 significant digits a count)
    n_in, n_out = sum(len(l.split()) for l in ins), sum(len(l.split()) for l in outs)
    assert (c >= 0).all()
    assert abs(c[[m.group(3) != "*e*" for m in arcs]].sum() - n_in) <= tol
    assert abs(c[[m.group(4) != "*e*" for m in arcs]].sum() - n_out) <= tol
    net = {}
    for m, k in zip(arcs, c):
        net[m.group(1)] = net.get(m.group(1), 0.0) - k
        net[m.group(2)] = net.get(m.group(2), 0.0) + k
    into_final, rest = net.pop(final), sorted(net.values())
    assert all(abs(v) <= tol for v in rest[1:]), rest[:3]  # flow is conserved at every state but final and one other: start
    assert abs(into_final + rest[0]) <= tol and (abs(into_final - len(ins)) <= tol or abs(into_final) <= tol)
    # the trainer's counts of the same machine and corpus, on the oracle's reading of the files; its arcs get their names from
    # the oracle's own print of the machine with arc k's weight replaced by k + 2
    ow = oracle.OracleWfst.parse(open(fst).read())
    w, cp = ow.arrays(), oracle.OracleCorpus.parse(ow, open(data).read()).arrays()
    line = lambda side, l: [int(s) for s in cp[side + "_sym"][int(cp[side + "_off"][l]):int(cp[side + "_off"][l + 1])]]
    corpus = Corpus.from_lists([(line("in", l), line("out", l)) for l in range(len(ins))])
    fb = HipForwardBackward(Wfst(w["n_states"], w["final"], w["src"], w["dst"], w["isym"], w["osym"], w["logw"]), corpus,
                            norm_group=NORM_NONE, normalize_first=False)
    fb.estimate()
    trained = fb.counts()
    fb.close()
    ow.set_logw(np.log(np.arange(len(trained)) + 2.0))
    named = [ARC.match(r) for r in ow.write(full=True, onearc=True).split("\n")[1:] if r]
    assert len(named) == len(trained) and all(named)
    want = {}
    for m in named:
        k = int(round(np.exp(printed_ln(m.group(5))))) - 2
        key = m.group(1, 2, 3, 4)
        want[key] = want.get(key, 0.0) + trained[k]
    got = {}
    for m, k in zip(arcs, c):
        got[m.group(1, 2, 3, 4)] = got.get(m.group(1, 2, 3, 4), 0.0) + k
    assert set(got) == set(want)
    assert max(abs(got[k] - want[k]) for k in got) <= tol, max(abs(got[k] - want[k]) for k in got)
