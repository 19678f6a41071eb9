"""GPU (-m gpu): the next E-step's weight pass enqueued by maximize behind its M-step kernel (option weights_ahead, engine.cpp
weights_ahead_enqueue) changes no bit of any result, is taken only when neither the weights nor the lattices were touched between
the two calls, and never where it does not belong (no mailbox, a cascade).  The kernel is the E-step's own; what could go wrong is
a stale or mislaid X, so the shapes need no more than several buckets and more than one layout: the toy corpora at 3000 pairs,
each as the library lays it out by itself and with the tiles' weights forced through X (tile_gather=0: small transducers' tiles
fetch their weights from the table, and then there is no weight pass to send ahead).

The loopback exchange plan of the issue's list is not here: an RCCL communicator wants a process of its own in this suite
(test_multirank_gpu.py), which does not fit a test of a few seconds; under a plan weights_ahead_enqueue returns at `t->xplan`."""
import functools
import math
import os

import numpy as np
import pytest

from carmel_amd import synth
from carmel_amd.model import NORM_CONDITIONAL, Corpus, Wfst

pytestmark = pytest.mark.gpu
ITERS = 3


def _fb(*a, **k):
    from carmel_amd.trainer import HipForwardBackward
    return HipForwardBackward(*a, **k)


@functools.lru_cache(maxsize=None)
def shape(name):
    return synth.make_config(name) if name == "toymix" else synth.make_config(name, n_pairs=3000)


def same_counts(x, y):
    """the repository's convention for counts (test_tile_sweep_is_the_three_kernels_it_replaces): the one atomic add per piece of
    a split hub arc aside"""
    return (x != y).sum() <= 16 and np.allclose(x, y, rtol=1e-13, atol=0)


def same_step(a, b, key=""):
    """one recorded E-step (+ M-step): ln p, ln p per pair, counts, and what the M-step made of them"""
    assert a["lp"] == b["lp"], key
    assert np.array_equal(a["pair"], b["pair"]), key
    assert same_counts(a["counts"], b["counts"]), key
    if "weights" in a:
        assert np.array_equal(a["weights"], b["weights"]), key
        assert a["change"] == b["change"], key


def estep(fb):
    lp, _ = fb.estimate(per_pair=True)
    return {"lp": lp, "pair": fb.pair_logprob.copy(), "counts": fb.counts().copy()}


def step(fb, rate=1.0):
    r = estep(fb)
    r["change"] = fb.maximize(rate)
    r["weights"] = fb.weights().copy()
    return r


def has_weight_pass(fb):
    """lane corpora under the transposition: the weights go through X unless the tile passes fetch them from the table"""
    return (fb.weight_source & 1) == 0


@pytest.mark.parametrize("through_x", [False, True])
@pytest.mark.parametrize("name", ["toy", "toya", "toymix"])
def test_same_bits_with_and_without(name, through_x, hipopt):
    """three EM iterations with the option unset and with "0": every ln p, ln p per pair, weight vector and largest change the
    same bits, the counts by the repository's convention; every early pass but the last taken where the layout has a weight
    pass, none enqueued where it has none or the option is off"""
    w, c = shape(name)
    if through_x:
        hipopt.set("tile_gather", "0")
    runs = {}
    for mode in ("on", "off"):
        hipopt.set("weights_ahead", None if mode == "on" else "0")
        fb = _fb(w, c)
        if through_x:
            assert has_weight_pass(fb)
        runs[mode] = [step(fb) for _ in range(ITERS)]
        enq, con = fb.weights_ahead_stats()
        print(name, through_x, mode, "weight pass" if has_weight_pass(fb) else "no weight pass", "tile sweep" if fb.tile_sweep_tiles else "",
              "fused lanes" if fb.fused_lane_tiles else "", "enqueued", enq, "consumed", con)
        if mode == "off":
            assert (enq, con) == (0, 0)
        elif has_weight_pass(fb):
            assert con == ITERS - 1 and enq == ITERS
        else:
            assert (enq, con) == (0, 0)
        fb.close()
    for k, (a, b) in enumerate(zip(runs["on"], runs["off"])):
        same_step(a, b, (name, k))


def _invalidation_run(w, c, record_stats):
    from carmel_amd._capi import check, lib
    fb = _fb(w, c)
    out, taken = [], []

    def est(expect_taken):
        before = fb.weights_ahead_stats()[1]
        out.append(estep(fb))
        taken.append((fb.weights_ahead_stats()[1] - before, expect_taken))

    est(0)
    fb.maximize(1.0)
    est(1)  # nothing in between: the early pass is the E-step's
    fb.maximize(1.0)
    w0 = fb.weights()
    fin = np.isfinite(w0)
    w0[fin] += 0.05 * np.cos(np.arange(len(w0)))[fin]
    fb.set_weights(w0)
    est(0)
    fb.maximize(1.0)
    check(lib.carmel_hip_normalize(fb.h), "carmel_hip_normalize")
    est(0)
    fb.maximize(1.0)
    check(lib.carmel_hip_random_restart(fb.h, 17, 1), "carmel_hip_random_restart")
    est(0)
    fb.save_best()
    fb.maximize(1.0)
    fb.load_best()  # back to the weights of the last E-step: what maximize sent ahead is not theirs
    est(0)
    fb.maximize(1.0)
    est(1)
    fb.maximize(1.5)  # the over-relaxed step sends nothing ahead
    est(0)
    fb.maximize(1.5)
    fb.keep_em_weights()
    est(0)
    out.append({"lp": 0.0, "pair": fb.weights().copy(), "counts": np.zeros(1)})
    fb.close()
    if record_stats:
        for k, (got, want) in enumerate(taken):
            assert got == want, (k, taken)
    else:
        assert all(got == 0 for got, _ in taken)
    return out


def test_every_invalidation(hipopt):
    """set_weights, normalize, random_restart, save_best / load_best, the over-relaxed maximize and keep_em_weights between a
    maximize and the next estimate: that estimate is the one of the same sequence with the option off, and took no early pass"""
    w, c = shape("toy")
    hipopt.set("tile_gather", "0")
    hipopt.unset("weights_ahead")
    on = _invalidation_run(w, c, True)
    hipopt.set("weights_ahead", "0")
    off = _invalidation_run(w, c, False)
    for k, (a, b) in enumerate(zip(on, off)):
        same_step(a, b, k)


def _layout_run(w, c, hipopt):
    fb = _fb(w, c)
    assert fb.tile_sweep_tiles > 0 and has_weight_pass(fb)
    out = [estep(fb)]
    fb.maximize(1.0)
    hipopt.set("tile_sweep_kernel", "0")  # the same layout, the three kernels: X is what they read too
    out.append(estep(fb))
    taken_same_layout = fb.weights_ahead_stats()[1]
    fb.maximize(1.0)
    hipopt.set("tile_sweep", "0")
    fb.rebuild_lattices()  # other tiles, another X
    assert fb.tile_sweep_tiles == 0
    out.append(estep(fb))
    taken_rebuilt = fb.weights_ahead_stats()[1] - taken_same_layout
    fb.close()
    hipopt.unset("tile_sweep_kernel")
    hipopt.unset("tile_sweep")
    return out, taken_same_layout, taken_rebuilt


def test_layout_switches_between_the_two_calls(hipopt):
    """tile_sweep_kernel=0 after maximize: the same X, the early pass is taken; lattices rebuilt with tile_sweep=0: it is
    dropped.  Results are the off-run's either way."""
    w, c = shape("toy")
    hipopt.set("tile_gather", "0")
    hipopt.unset("weights_ahead")
    on, same, rebuilt = _layout_run(w, c, hipopt)
    assert same == 1 and rebuilt == 0
    hipopt.set("weights_ahead", "0")
    off, same, rebuilt = _layout_run(w, c, hipopt)
    assert same == 0 and rebuilt == 0
    for k, (a, b) in enumerate(zip(on, off)):
        same_step(a, b, k)


def test_estep_time_with_an_early_pass(hipopt):
    """carmel_hip_last_sweep_ms after an E-step that took an early pass, read before and after the next maximize has enqueued
    the following one: finite and positive (no threshold: it is a time)"""
    w, c = shape("toy")
    hipopt.set("tile_gather", "0")
    hipopt.unset("weights_ahead")
    fb = _fb(w, c)
    fb.estimate()
    fb.maximize(1.0)
    for _ in range(2):
        fb.estimate_async()
        assert fb.weights_ahead_stats()[1] >= 1
        a = fb.last_kernel_ms()
        fb.maximize(1.0)
        b = fb.last_kernel_ms()
        for ms in (a, b):
            assert math.isfinite(ms) and ms > 0
    fb.estimate()
    assert math.isfinite(fb.last.kernel_ms) and fb.last.kernel_ms > 0
    fb.close()


def test_no_early_pass_without_the_mailbox(hipopt):
    """mailbox=0: the host gets the M-step's result by synchronising the stream, nothing is sent ahead; same results"""
    w, c = shape("toy")
    hipopt.set("tile_gather", "0")
    runs = {}
    for mode in ("nobox", "off"):
        hipopt.set("mailbox", "0" if mode == "nobox" else None)
        hipopt.set("weights_ahead", "0" if mode == "off" else None)
        fb = _fb(w, c)
        runs[mode] = [step(fb) for _ in range(2)]
        assert fb.weights_ahead_stats() == (0, 0)
        fb.close()
    for k, (a, b) in enumerate(zip(runs["nobox"], runs["off"])):
        same_step(a, b, k)


def test_no_early_pass_for_a_cascade(oracle, golden_dir, hipopt):
    """the tagging cascade (its M-step ends in chain_update, its maximize in a stream synchronisation): nothing sent ahead, same
    results.  A cascade's parameter counts are atomic adds in the order the hardware schedules them (chain_scatter_kernel), so
    two runs of the SAME library agree bit for bit up to the first M-step only.  Behind it: a parameter's count is a sum of at
    most n_arcs = 400 994 non-negative terms, in any order within (n - 1) * 2^-53 = 4.5e-11 of the exact sum relatively, its
    group's total (sums of at most 10 934 such) within another 1.3e-12; ln weight = ln count - ln total moves by at most
    2 * 4.6e-11 = 1e-10.  A derivation of a pair is at most L = |input| + |output| arcs, so every term of the second E-step's
    sums moves by at most L * 1e-10 in the log domain: ln p per pair within that absolutely, posteriors -- ratios of two such
    -- and the counts they add up to within 2 * L * 1e-10 relatively."""
    texts = [open(os.path.join(golden_dir, n)).read() for n in ("tagging.fsa", "tagging.fst")]
    oc = oracle.OracleCascade(texts)
    a = oc.composed().arrays()
    w = Wfst(a["n_states"], a["final"], a["src"], a["dst"], a["isym"], a["osym"], a["logw"], a["group"])
    ca = oc.corpus(open(os.path.join(golden_dir, "tagging.data")).read()).arrays()
    c = Corpus(ca["in_off"], ca["in_sym"], ca["out_off"], ca["out_sym"], ca["weight"])
    runs = {}
    for mode in ("on", "off"):
        hipopt.set("weights_ahead", None if mode == "on" else "0")
        fb = _fb(w, c, cascade=oc.as_dict([NORM_CONDITIONAL, NORM_CONDITIONAL]))
        runs[mode] = [step(fb) for _ in range(2)]
        assert fb.weights_ahead_stats() == (0, 0)
        fb.close()
    (x, x2), (y, y2) = runs["on"], runs["off"]
    same_step({k: v for k, v in x.items() if k in ("lp", "pair", "counts")}, {k: v for k, v in y.items() if k in ("lp", "pair", "counts")})
    assert x["change"] == y["change"] == 10.0  # (train.cc:922: a cascade's maximize reports no change)
    assert np.array_equal(np.isfinite(x["weights"]), np.isfinite(y["weights"]))
    fin = np.isfinite(x["weights"])
    assert np.array_equal(x["weights"][~fin], y["weights"][~fin])
    assert np.abs(x["weights"][fin] - y["weights"][fin]).max() <= 1e-10
    L = (np.diff(c.in_off.astype(np.int64)) + np.diff(c.out_off.astype(np.int64))).astype(np.float64)
    ok = np.isfinite(x2["pair"])
    assert np.array_equal(ok, np.isfinite(y2["pair"]))
    assert (np.abs(x2["pair"][ok] - y2["pair"][ok]) <= L[ok] * 1e-10).all()
    assert abs(x2["lp"] - y2["lp"]) <= L[ok].sum() * 1e-10
    np.testing.assert_allclose(x2["counts"], y2["counts"], rtol=2 * L.max() * 1e-10, atol=0)
