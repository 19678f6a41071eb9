"""CPU: batch pair arc posteriors (carmel_hip_decode_pairs_posterior) -- the reference of decode_pairs_posterior_ref.py proved
four ways (against exhaustive enumeration, against the CPU oracle's E-step, by its invariants on every pair, and in f64 against
longdouble), what the workload contains, the front end's --pair-counts switch where no device is needed, and the new kernels'
resources.  Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest

from decode_pairs_cases import SEEDS, case
from decode_pairs_posterior_cases import per_pair, per_pair_in, reference
from decode_pairs_ref import enumerate_paths
from decode_posterior_ref import net_flow
from test_decode_host import run, signed
from test_decode_pairs_host import small_seeds
from test_decode_pairs_posterior_gpu import E_REF
from test_kernel_resources import device_asm, kernels

G = lambda golden_dir, n: os.path.join(golden_dir, n)
MACHINES = ["cat.fsa.trained.noe", "spellout.fst.trained"]


def test_reference_counts_against_exhaustive_enumeration():
    """(a) every pair of the small seeds (|Q| < 40) is enumerable: counts[a] = the sum over the derivations d of w(d) uses_d(a) /
    the sum of w(d), the derivations' weights in longdouble.  Bound: both sides are f64 at the end; a derivation's
    p = exp(w - Z) comes from sums of at most ~60 logs of magnitude <= ~100, so its relative error is below 60 x 100 x 2^-53 ~
    7e-13, and a count adds such terms: 1e-10 of max(1, count) leaves two orders."""
    n_pairs, worst, most = 0, 0.0, 0
    for s in small_seeds():
        c = case(s)
        P = c["P"]
        sums, counts = per_pair(s)
        for l, (x, y) in enumerate(c["pairs"]):
            every = enumerate_paths(P, x, y, limit=5000)
            assert every is not None and len(every) == c["count"][l], (s, l)
            if not every:
                assert sums[l] == -np.inf and not counts[l].any()
                continue
            lw = np.array([P.logw[np.array(p, np.int64)].astype(np.longdouble).sum() for p in every], np.longdouble)
            post = np.exp(lw - np.logaddexp.reduce(lw))
            want = np.zeros(len(P.src), np.longdouble)
            for p, pr in zip(every, post):
                np.add.at(want, np.array(p, np.int64), pr)
            want = want.astype(np.float64)
            err = np.abs(counts[l] - want) / np.maximum(1.0, want)
            assert err.max() <= 1e-10, (s, l, int(err.argmax()), float(err.max()))
            worst, most, n_pairs = max(worst, float(err.max())), max(most, len(every)), n_pairs + 1
    print("pairs %d, at most %d derivations, worst |count - enumerated| / max(1, count): %.3g" % (n_pairs, most, worst))
    assert n_pairs >= 800


def test_reference_counts_against_the_oracle_e_step(oracle):
    """(b) the same pairs as a corpus through the CPU oracle's E-step (a derivation lattice per pair, built by composition): an
    independent route.  Tolerance: what tests/test_gpu_parity.py holds the trainer's counts to against this oracle."""
    from carmel_amd.model import Corpus
    worst, n = 0.0, 0
    for s in small_seeds():
        c = case(s)
        pairs = [(y, x) if c["side"] else (x, y) for x, y in c["pairs"]]  # the corpus is (input, output)
        r = oracle.estimate(oracle.OracleWfst.from_arrays(c["w"]), oracle.OracleCorpus.from_arrays(Corpus.from_lists(pairs)))
        _, sums, counts = reference(s)
        assert np.array_equal(sums > -np.inf, r["has_deriv"]), s
        want = np.exp(r["counts_ln"])
        np.testing.assert_allclose(counts, want, rtol=1e-7, atol=1e-14, err_msg=str(s))
        worst, n = max(worst, float((np.abs(counts - want) / np.maximum(1.0, want)).max())), n + int((sums > -np.inf).sum())
    print("reference against the oracle: %d pairs with a derivation, worst |difference| / max(1, count) %.3g" % (n, worst))
    assert n >= 800


def test_reference_invariants_of_every_pair():
    """(c) per pair with a derivation: the counts of the arcs with a matched symbol add up to len(x), of those with an other
    symbol to len(y); net flow is +1 at final, -1 at start (0 if they coincide), 0 elsewhere; a zero-weight arc has count 0.
    Every identity holds exactly for exact posteriors; the f64 ones carry a relative error of ~1e-12 each ((a)'s reasoning):
    1e-9 of the larger of 1 and the total that flows."""
    from decode_pairs_cases import sides
    n = 0
    for s in SEEDS:
        c = case(s)
        if c["P"] is None:
            continue
        w = c["w"]
        msym, osym = sides(w, c["side"])
        sums, counts = per_pair(s)
        assert sums.tolist() == c["sum"].tolist()  # the forward planes are decode_pairs_ref's: the sums bit for bit
        for l, (x, y) in enumerate(c["pairs"]):
            k = counts[l]
            if not sums[l] > -np.inf:
                assert not k.any()
                continue
            tol = 1e-9 * max(1.0, float(k.sum()))
            assert (k >= 0).all() and not k[~(w.logw > -np.inf)].any()
            assert abs(float(k[msym != 0].sum()) - len(x)) <= tol and abs(float(k[osym != 0].sum()) - len(y)) <= tol, (s, l)
            want = np.zeros(w.n_states)
            want[w.final] += 1.0
            want[0] -= 1.0
            assert np.abs(net_flow(w.n_states, w.src, w.dst, k) - want).max() <= tol, (s, l)
            n += 1
    print("pairs with a derivation %d" % n)
    assert n >= 900


def test_reference_f64_against_longdouble():
    """(d) E = the largest |f64 count - longdouble count| / max(1, count) over the whole workload, a batch's counts per seed: the
    reference's own error, from which the GPU test's tolerance is taken (test_decode_pairs_posterior_gpu.E_REF is the figure
    logged in profiles/measurement_log_decode_pairs_posterior.md).  numpy's exp and log1p differ between builds in the last ulp,
    so a rerun may land a little off the logged figure: within a factor of 4 of it, above or below."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    from decode_pairs_posterior_cases import summed
    E, E_pair = 0.0, 0.0
    for s in SEEDS:
        if per_pair(s) is None:
            continue
        s64, c64 = per_pair(s)
        s80, c80 = per_pair_in(s, np.longdouble)
        assert np.array_equal(s64 > -np.inf, s80 > -np.inf)
        E_pair = max(E_pair, float((np.abs(c64 - c80) / np.maximum(1.0, c80)).max()))
        t64, t80 = summed(s64, c64, None), summed(s80, c80, None)
        E = max(E, float((np.abs(t64 - t80) / np.maximum(1.0, t80)).max()))
    print("E = %.3g (logged: %.3g); over single pairs %.3g" % (E, E_REF, E_pair))
    assert E_REF / 4 <= E <= 4 * E_REF, (E, E_REF)


def test_the_workload_has_fractional_counts():
    """the shares test_decode_pairs_host.test_gpu_test_inputs_really_pair asserts hold unchanged (the workload is imported, not
    changed); on top of them: pairs with several derivations that disagree on an arc"""
    fractional = 0
    for s in SEEDS:
        if per_pair(s) is None:
            continue
        sums, counts = per_pair(s)
        frac = np.abs(counts - np.round(counts)) > 1e-6
        fractional += int((frac.any(axis=1) & (sums > -np.inf)).sum())
    print("pairs with a non-integer count: %d" % fractional)
    assert fractional >= 100


@pytest.mark.parametrize("args", [
    ["-qbsriWIEk", "1", "--pair-counts=x.out"],  # no --pair-lines
    ["-qbsriWIEk", "1", "--pair-counts=", "--pair-lines=x"],  # no file name
    ["-q", "-t", "--pair-counts=x.out", "--pair-lines=x"],  # training
    ["-q", "--train-cascade", "--pair-counts=x.out", "--pair-lines=x"],
    ["-q", "-S", "--pair-counts=x.out", "--pair-lines=x"],
])
def test_pair_counts_out_of_place_are_refused(golden_dir, args):
    rc, out, err = run(args + [G(golden_dir, m) for m in MACHINES], stdin="c1 c2\n")
    assert signed(rc) == -12, err
    assert "--pair-counts" in err and "HIP" not in err
    assert out == ""
    assert not os.path.exists("x.out")


@pytest.mark.parametrize("form", [["-qbsriWIEk", "1"], ["-qbsriWIEk", "1", "--sum-paths"], ["-qsriWIEk", "1"],
                                  ["-qbsrOEk", "1", "--pair-alignments=%s"]])
def test_pair_counts_get_past_the_switches(golden_dir, tmp_path, form):
    """--pair-counts with --pair-lines and -k 1 fails only where the device is needed (-11, "no HIP device"); with a GPU it succeeds"""
    from carmel_amd._capi import lib
    other, counts = tmp_path / "other", tmp_path / "counts.fst"
    other.write_text("c1\n")
    form = [f % (tmp_path / "align") if "%s" in f else f for f in form]
    rc, out, err = run(form + ["--pair-lines=%s" % other, "--pair-counts=%s" % counts] + [G(golden_dir, m) for m in MACHINES],
                       stdin="c1 c2\n")
    if lib.carmel_hip_device_count() > 0:
        assert rc == 0 and os.path.getsize(counts) > 0, err
        return
    assert signed(rc) == -11, err
    assert "not implemented" not in err and "no HIP device" in err and "carmel_hip_decoder_create" in err


def test_help_names_pair_counts():
    rc, out, err = run(["-h"])
    assert rc == 0 and "--pair-counts" in out


def test_pair_posterior_kernels_use_no_scratch_memory():
    ks = kernels(device_asm("decode_pairs_posterior.hip"))
    assert len(ks) == 4, list(ks)  # the shared pair trellis around KeepAcc and the backward kernel, in their two tiers
    assert sum("pair_trellis_kernel" in k and "KeepAcc" in k for k in ks) == 2
    assert sum("pair_posterior_kernel" in k for k in ks) == 2
    for name, (body, tail) in ks.items():
        m = re.search(r"; ScratchSize: (\d+)", tail)
        assert m and int(m.group(1)) == 0, (name, m and m.group(0))
        assert "scratch_" not in body, name
        assert "global_atomic_add_f64" in body or "pair_trellis_kernel" in name, name  # the hardware atomic, no CAS loop
        assert "cmpswap" not in body, name
