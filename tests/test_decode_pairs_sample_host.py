"""CPU: what the GPU tests of batch pair alignment sampling rest on (tests/test_decode_pairs_sample_gpu.py) -- the reference of
decode_pairs_sample_ref.py against brute force (its frequencies over the pairs with 2 .. 64 derivations against exp(w - Z) over
every enumerated derivation), every path it samples a derivation of its pair, the front end's refusals around --pair-samples, the
help text, and the new file's kernels: four, without scratch memory."""
import os
import re

import numpy as np
import pytest

from decode_pairs_ref import rescore
from decode_pairs_sample_cases import (FREQ_SEEDS, N_FREQ, N_RANDOM, SEED_FREQ, SEEDS, case, check_frequencies, posterior,
                                       reference)
from decode_pairs_sample_ref import sample
from decode_sample_ref import frequencies, paths_of
from test_decode_host import run, signed
from test_kernel_resources import device_asm, kernels

G = lambda golden_dir, n: os.path.join(golden_dir, n)
MACHINES = ["cat.fsa.trained.noe", "spellout.fst.trained"]


def test_reference_frequencies_against_brute_force():
    """N = 4000 samples of every pair with 2 .. 64 derivations of the seeds s % 5 == 1, within 5 sigma of the exact posterior
    over decode_pairs_ref.enumerate_paths"""
    n_pairs, worst = 0, 0.0
    for seed in FREQ_SEEDS:
        post = posterior(seed)
        if not post:
            continue
        c = case(seed)
        got = sample(c["P"], c["pairs"], N_FREQ, SEED_FREQ, only=set(post))
        for l, exact in post.items():
            mat, _ = got[l]
            assert len(mat) == N_FREQ
            worst = max(worst, check_frequencies(frequencies(mat), exact, N_FREQ, (seed, l)))
            n_pairs += 1
    print("%d pairs, worst |f - p| in units of the bound's sigma: %.2f" % (n_pairs, worst))
    assert n_pairs >= 20, n_pairs


def test_every_sample_of_the_reference_is_a_derivation():
    n_paths = n_cycles = 0
    for seed in SEEDS:
        c, ref = case(seed), reference(seed)
        if ref is None:
            n_cycles += 1
            continue
        for l, (x, y) in enumerate(c["pairs"]):
            if ref[l] is None:
                assert c["count"][l] == 0, (seed, l)
                continue
            assert c["count"][l] > 0, (seed, l)
            mat, amb = ref[l]
            assert len(mat) == N_RANDOM and len(amb) == N_RANDOM
            for path in paths_of(mat):
                rescore(c["P"], x, y, path)  # (asserts: start to final, spells x and y, no arc of weight zero)
                n_paths += 1
    print("%d sampled paths, %d seeds with a 00 cycle" % (n_paths, n_cycles))
    assert n_paths >= 4000 and n_cycles >= 1


@pytest.mark.parametrize("args", [
    ["-qbsriWIEk", "1", "--pair-samples=3"],  # no --pair-lines
    ["-qsrWIE", "--pair-samples=3", "--pair-lines=x"],  # neither -b nor -i
    ["-qbsriWIE", "--pair-samples=0", "--pair-lines=x"],
    ["-qbsriWIE", "--pair-samples=65537", "--pair-lines=x"],
    ["-qbsriWIEk", "2", "--pair-samples=3", "--pair-lines=x"],  # -k neither 1 nor N
    ["-qbsriWIE", "--pair-samples=3", "--kbest=3", "--pair-lines=x"],
    ["-qbsriWIE", "--pair-samples=3", "--sample-paths=3", "--pair-lines=x"],
    ["-q", "-t", "--pair-samples=3", "--pair-lines=x"],
    ["-q", "--train-cascade", "--pair-samples=3", "--pair-lines=x"],
    ["-q", "-S", "--pair-samples=3", "--pair-lines=x"],
])
def test_pair_samples_out_of_place_are_refused(golden_dir, args):
    rc, out, err = run(args + [G(golden_dir, m) for m in MACHINES], stdin="c1 c2\n")
    assert signed(rc) == -12, err
    assert "--pair-samples" in err and "HIP" not in err
    assert out == ""


@pytest.mark.parametrize("form", [["-qbsriWIEk", "1"], ["-qbsriWIE"], ["-qbsriWIEk", "3"], ["-qbsriWIEk", "1", "--sum-paths"],
                                  ["-qsriWIEk", "1"], ["-qbsrOEk", "1", "--pair-alignments=%s"]])
def test_pair_samples_get_past_the_switches(golden_dir, tmp_path, form):
    """--pair-samples=3 with --pair-lines fails only where the device is needed (-11, "no HIP device"); with a GPU it succeeds"""
    from carmel_amd._capi import lib
    other = tmp_path / "other"
    other.write_text("c1\n")
    form = [f % (tmp_path / "align") if "%s" in f else f for f in form]
    rc, out, err = run(form + ["--pair-samples=3", "--pair-lines=%s" % other] + [G(golden_dir, m) for m in MACHINES], stdin="c1 c2\n")
    if lib.carmel_hip_device_count() > 0:
        assert rc == 0, err
        assert len(out.split("\n")) == 4 and "Viterbi" not in err
        return
    assert signed(rc) == -11, err
    assert "not implemented" not in err and "no HIP device" in err and "carmel_hip_decoder_create" in err


def test_help_names_pair_samples():
    rc, out, err = run(["-h"])
    assert rc == 0 and "--pair-samples" in out


def test_pair_sample_kernels_use_no_scratch_memory():
    ks = kernels(device_asm("decode_pairs_sample.hip"))
    assert len(ks) == 4, list(ks)  # the shared pair trellis around KeepAcc in its two tiers, the walk's two passes
    assert sum("pair_trellis_kernel" in k and "KeepAcc" in k for k in ks) == 2
    assert sum("pair_sample_walk_kernel" in k for k in ks) == 2
    for name, (body, tail) in ks.items():
        m = re.search(r"; ScratchSize: (\d+)", tail)
        assert m and int(m.group(1)) == 0, (name, m and m.group(0))
        assert "scratch_" not in body, name
