"""CPU: batch arc posteriors (carmel_hip_decode_posterior) -- the reference of decode_posterior_ref.py proved four ways (against
exact enumeration, as the gradient of the sums, by its invariants on the random workload, and in f64 against longdouble), the front
end's --posterior-counts switch where no device is needed, and the new kernels' resources.  Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest

from decode_posterior_cases import SEEDS, case, prepared, reference, reference_in
from decode_posterior_ref import net_flow, posterior, rows
from decode_sample_cases import FREQ_SEEDS, msym_of
from decode_sample_cases import posterior as enumerated
from test_decode_host import run, signed
from test_decode_posterior_gpu import E_REF
from test_kernel_resources import device_asm, kernels


def test_reference_counts_against_exact_enumeration():
    """(a) the expected uses of every arc over the enumerated derivations of the lines with 2 .. 64 of them.  Bound: both sides
    are f64; a derivation's p = exp(w - Z) comes from sums of at most ~50 logs of magnitude <= ~100, so its relative error is
    below 50 x 100 x 2^-53 ~ 6e-13, and a count adds such terms: 1e-10 of max(1, count) leaves two orders."""
    n_lines = 0
    worst = 0.0
    for seed in FREQ_SEEDS:
        w = case(seed)["w"]
        for side, lines, post in enumerated(seed):
            if not post:
                continue
            picked = sorted(post)
            want = np.zeros(w.n_arcs)
            for l in picked:
                for path, p in post[l].items():
                    np.add.at(want, np.array(path, np.int64), p)
            sums, got = posterior(w.n_states, w.final, w.src, w.dst, msym_of(w, side), w.logw, [lines[l] for l in picked],
                                  prepared=prepared(seed, side))
            assert np.isfinite(sums).all()
            err = np.abs(got - want) / np.maximum(1.0, want)
            worst = max(worst, float(err.max()))
            assert err.max() <= 1e-10, (seed, side, int(err.argmax()), float(err.max()))
            n_lines += len(picked)
    print("lines %d, worst |count - enumerated| / max(1, count): %.3g" % (n_lines, worst))
    assert n_lines >= 60, n_lines


@pytest.mark.parametrize("seed", [1, 2, 4])
def test_reference_counts_are_the_gradient_of_the_sums(seed):
    """(b) counts[a] = d (the sum over the lines of Z_l) / d logw[a], by a central difference of the numpy forward in longdouble
    with h = 1e-6: the truncation error is h^2 / 6 times a third cumulant of the arc's uses (a few thousand at most for an arc
    used at every position of a 24-symbol line) ~ 1e-9, the rounding 2^-63 |Z| / h ~ 1e-11 a line; bound 1e-7 of max(1, count)."""
    w = case(seed)["w"]
    h = np.longdouble(1e-6)
    checked = 0
    for side, lines, _, sums, counts in reference(seed):
        src, dst, logw, by_sym, by_level = prepared(seed, side)
        with_z = [l for l, z in zip(lines, sums) if z > -np.inf]
        msym = msym_of(w, side)
        arcs = [int(a) for a in np.argsort(-counts)[:4]]
        arcs += [int(a) for a in np.flatnonzero((msym == 0) & (counts > 0))[:2]]
        arcs += [int(a) for a in np.flatnonzero((counts == 0) & (w.logw > -np.inf))[:1]]
        for a in sorted(set(arcs)):
            total = []
            for sign in (1, -1):
                lw = logw.astype(np.longdouble)
                lw[a] += sign * h
                prep = (src, dst, lw, by_sym, by_level)
                total.append(sum(rows(w.n_states, w.final, prep, l, np.longdouble)[0][len(l), w.final] for l in with_z))
            grad = float((total[0] - total[1]) / (2 * h))
            assert abs(grad - counts[a]) <= 1e-7 * max(1.0, counts[a]), (seed, side, a, grad, counts[a])
            checked += 1
    assert checked >= 5


@pytest.mark.parametrize("weighted", [False, True])
def test_reference_invariants_on_the_random_workload(weighted):
    """(c) the counts of the matched arcs add up to the weighted length of the lines with a derivation; flow is conserved at
    every state but start and final, which differ by the lines' weight; a zero-weight arc has count 0.  Bound: every identity
    holds exactly for exact posteriors, the f64 ones carry a relative error of ~1e-12 each ((a)'s reasoning): 1e-9 of the larger
    of 1 and the total that flows."""
    n_sides = n_lines = 0
    for seed in SEEDS:
        w = case(seed)["w"]
        sum_of = {side: ref for side, _, ref, _, _ in case(seed)["sides"]}
        for side, lines, wt, sums, counts in reference(seed, weighted):
            msym = msym_of(w, side)
            c = np.ones(len(lines)) if wt is None else wt
            has = sums > -np.inf
            assert sums.tolist() == sum_of[side].tolist()  # the forward rows end in decode_sum_ref's sums, bit for bit
            mass = float(c[has].sum())
            length = float(sum(c[l] * len(lines[l]) for l in np.flatnonzero(has)))
            tol = 1e-9 * max(1.0, float(counts.sum()))
            assert (counts >= 0).all() and not counts[~(w.logw > -np.inf)].any()
            assert abs(float(counts[msym != 0].sum()) - length) <= tol, (seed, side)
            want = np.zeros(w.n_states)
            want[w.final] += mass
            want[0] -= mass
            assert np.abs(net_flow(w.n_states, w.src, w.dst, counts) - want).max() <= tol, (seed, side)
            n_sides += 1
            n_lines += int(has.sum())
    print("sides %d, lines with a derivation %d" % (n_sides, n_lines))
    assert n_sides >= 150 and n_lines >= 1000


def test_reference_f64_against_longdouble():
    """(d) E = the largest |f64 count - longdouble count| / max(1, count) over the random workload: the reference's own error, from
    which the GPU test's tolerance is taken (test_decode_posterior_gpu.E_REF is the figure logged in
    profiles/measurement_log_decode_posterior.md).  numpy's exp and log1p differ between builds in the last ulp, so a rerun may
    land a little off the logged figure: within a factor of 4 of it, above or below."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    E = 0.0
    for seed in SEEDS:
        for (side, _, _, s64, c64), (_, _, _, s80, c80) in zip(reference(seed), reference_in(seed, np.longdouble, False)):
            assert np.array_equal(s64 > -np.inf, s80 > -np.inf)
            E = max(E, float((np.abs(c64 - c80) / np.maximum(1.0, c80)).max()))
    print("E = %.3g (logged: %.3g)" % (E, E_REF))
    assert E_REF / 4 <= E <= 4 * E_REF, (E, E_REF)


@pytest.mark.parametrize("args", [
    ["-q", "--posterior-counts=x.out"],  # no -b / -i
    ["-qk", "1", "-WIE", "--posterior-counts=x.out"],
    ["-qbsriWIEk", "1", "--posterior-counts="],  # no file name
    ["-qtbsriWIEk", "1", "--posterior-counts=x.out"],  # pairs
    ["-qSbsriWIEk", "1", "--posterior-counts=x.out"],
])
def test_posterior_counts_usage_errors(golden_dir, tmp_path, args):
    g = lambda n: os.path.join(golden_dir, n)
    rc, out, err = run(args + [g("cat.fsa.trained.noe"), g("spellout.fst.trained")], stdin="c1 c2\n")
    assert signed(rc) == -12, err
    assert "HIP" not in err and out == ""
    assert "--posterior-counts" in err, err
    assert not os.path.exists("x.out")


@pytest.mark.parametrize("form", [["-qbsriWIEk", "1"], ["-qbsriWIE", "--kbest=3"], ["-qbsriWIE", "--sample-paths=3", "-R", "7"],
                                  ["-qbsriWIEk", "1", "--sum-paths"]])
def test_posterior_counts_gets_past_the_switches(golden_dir, tmp_path, form):
    """fails only where the device is needed (-11, "no HIP device"); with a GPU it succeeds"""
    from carmel_amd._capi import lib
    g = lambda n: os.path.join(golden_dir, n)
    counts = str(tmp_path / "counts.fst")
    rc, out, err = run(form + ["--posterior-counts=" + counts, g("cat.fsa.trained.noe"), g("spellout.fst.trained")], stdin="c1 c2\n")
    if lib.carmel_hip_device_count() > 0:
        assert rc == 0 and os.path.getsize(counts) > 0, err
        return
    assert signed(rc) == -11, err
    assert "not implemented" not in err and "no HIP device" in err and "carmel_hip_decoder_create" in err


def test_help_names_posterior_counts():
    rc, out, err = run(["-h"])
    assert rc == 0 and "--posterior-counts" in out


def test_posterior_kernels_use_no_scratch_memory():
    ks = kernels(device_asm("decode_posterior.hip"))
    assert len(ks) == 4, list(ks)  # the shared trellis kernel around the sampler's node and the backward kernel, in their two tiers
    assert sum("trellis_kernel" in k and "SampleNode" in k for k in ks) == 2
    assert sum("decode_posterior_kernel" in k for k in ks) == 2
    for name, (body, tail) in ks.items():
        m = re.search(r"; ScratchSize: (\d+)", tail)
        assert m and int(m.group(1)) == 0, (name, m and m.group(0))
        assert "scratch_" not in body, name
        assert "global_atomic_add_f64" in body or "trellis_kernel" in name, name  # the hardware atomic, no CAS loop
        assert "cmpswap" not in body, name
