"""CPU: batch posterior path sampling (carmel_hip_decode_sample) -- the reference of decode_sample_ref.py: its uniform against the
library's, its paths on the random workload (derivations all, few ambiguous draws), its frequencies against the exact posterior
by enumeration, the front end's --sample-paths switch where no device is needed, and the new kernels' resources.  Nothing here
needs a GPU."""
import os
import re

import numpy as np
import pytest

from decode_sample_cases import FREQ_SEEDS, N_FREQ, SEED_FREQ, SEEDS, check_frequencies, model, posterior, reference
from decode_sample_ref import frequencies, is_derivation, paths_of, sample_line, uniform, uniform_many
from test_decode_host import run, signed
from test_kernel_resources import device_asm, kernels


def test_restated_uniform_equals_the_library():
    from carmel_amd._capi import lib
    rng = np.random.default_rng(1)
    tuples = [(0, 0, 0, 0), (1, 0, 0, 0), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1), (12345, 7, 23, 0), (777, 3999, 5, 41)]
    tuples += [(int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(0, 2 ** 32)),
                int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))) for _ in range(300)]
    for seed, it, block, step in tuples:
        u = uniform(seed, it, block, step)
        assert 0.0 <= u < 1.0
        assert u == lib.carmel_hip_gibbs_uniform(seed, it, block, step), (seed, it, block, step)
    its = np.arange(500)
    many = uniform_many(777, its, 17, 3)  # the array form the reference draws with
    assert many.tolist() == [uniform(777, int(i), 17, 3) for i in its]


def test_reference_paths_are_derivations_and_few_draws_are_ambiguous():
    n_paths = n_amb = n_lines = n_without = 0
    for seed in SEEDS:
        for side, lines, m, samples in reference(seed):
            for line, got in zip(lines, samples):
                n_lines += 1
                if got is None:
                    n_without += 1
                    continue
                mat, amb = got
                assert mat.shape[0] == 8 and amb.shape == (8,)
                for p in paths_of(mat):
                    assert is_derivation(m, line, p), (seed, side, line, p)
                n_paths += 8
                n_amb += int(amb.sum())
    print("lines %d (%d without a derivation), reference paths %d, ambiguous %d" % (n_lines, n_without, n_paths, n_amb))
    assert n_paths >= 8000 and n_without >= 100
    assert n_amb <= 0.01 * n_paths, (n_amb, n_paths)


@pytest.mark.parametrize("seed", FREQ_SEEDS)
def test_reference_frequencies_against_the_exact_posterior(seed):
    worst = 0.0
    for side, lines, post in posterior(seed):
        m = model(seed, side)
        for l, exact in post.items():
            assert abs(sum(exact.values()) - 1.0) <= 1e-9
            mat, _ = sample_line(m, lines[l], l, N_FREQ, SEED_FREQ)
            worst = max(worst, check_frequencies(frequencies(mat), exact, N_FREQ, (seed, side, l)))
    print("seed %d: worst |f - p| in units of the bound's sigma: %.2f" % (seed, worst))


def test_frequency_test_has_lines():
    n = sum(len(post) for seed in FREQ_SEEDS for _, _, post in posterior(seed))
    assert n >= 60, n


@pytest.mark.parametrize("args", [
    ["-q", "--sample-paths=3"],  # no -b / -i
    ["-qbsriWIE", "--sample-paths=3", "--kbest=3"],
    ["-qbsriWIE", "--sample-paths=0"],
    ["-qbsriWIE", "--sample-paths=65537"],
    ["-qbsriWIEk", "2", "--sample-paths=3"],
    ["-qbsri", "--sample-paths=3"],  # the arc path form stays refused
    ["-qbsriWIE", "-G", "3"],  # carmel's generation is another thing and stays refused
    ["-qbsriWIE", "-g", "3"],
])
def test_sample_paths_usage_errors(golden_dir, args):
    g = lambda n: os.path.join(golden_dir, n)
    rc, out, err = run(args + [g("cat.fsa.trained.noe"), g("spellout.fst.trained")], stdin="c1 c2\n")
    assert signed(rc) == -12, err
    assert "HIP" not in err and out == ""
    assert ("--sample-paths" in err) or ("-G" in err) or ("-g" in err) or ("-k" in err), err


@pytest.mark.parametrize("form", [["-qbsriWIE", "--sample-paths=3"], ["-qbsriWIEk", "3", "--sample-paths=3"],
                                  ["-qbsriWIEk", "1", "--sample-paths=3", "--sum-paths", "-R", "7"]])
def test_sample_paths_gets_past_the_switches(golden_dir, form):
    """fails only where the device is needed (-11, "no HIP device"); with a GPU it succeeds"""
    from carmel_amd._capi import lib
    g = lambda n: os.path.join(golden_dir, n)
    rc, out, err = run(form + [g("cat.fsa.trained.noe"), g("spellout.fst.trained")], stdin="c1 c2\n")
    if lib.carmel_hip_device_count() > 0:
        assert rc == 0 and len(out.split("\n")) == 4, err
        return
    assert signed(rc) == -11, err
    assert "not implemented" not in err and "no HIP device" in err and "carmel_hip_decoder_create" in err


def test_help_names_sample_paths():
    rc, out, err = run(["-h"])
    assert rc == 0 and "--sample-paths" in out


def test_sample_kernels_use_no_scratch_memory():
    ks = kernels(device_asm("decode_sample.hip"))
    assert len(ks) == 4, list(ks)  # the shared trellis kernel around the sampler's node in its two tiers, the walk's two passes
    assert sum("trellis_kernel" in k and "SampleNode" in k for k in ks) == 2
    assert sum("decode_sample_walk_kernel" in k for k in ks) == 2
    for name, (body, tail) in ks.items():
        m = re.search(r"; ScratchSize: (\d+)", tail)
        assert m and int(m.group(1)) == 0, (name, m and m.group(0))
        assert "scratch_" not in body, name
