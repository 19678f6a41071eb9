"""CPU: k-best decoding -- the Python reference (decode_kbest_ref.py) against exhaustive enumeration, the inputs of the GPU test
against the tie cap, the front end's --kbest=N switches, and the k-best kernels' resources.  Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest

from decode_kbest_ref import CycleError, enumerate_all, kbest
from test_decode_host import run, signed
from test_kernel_resources import device_asm, kernels


def tiny_machine(rng, quantised):
    """|Q| <= 6, <= 14 arcs, epsilon arcs (matched side) only forward in state order; `quantised` weights tie often"""
    Q = int(rng.integers(2, 7))
    n = int(rng.integers(Q, 15))
    src = rng.integers(0, Q, n)
    dst = rng.integers(0, Q, n)
    msym = rng.integers(0, 3, n)  # 0 = epsilon, symbols 1 and 2
    msym[(msym == 0) & (dst <= src)] = 1
    logw = np.log(rng.choice([0.5, 0.25], n)) if quantised else np.log(rng.uniform(0.01, 1.0, n))
    logw[rng.uniform(size=n) < 0.05] = -np.inf
    return Q, src, dst, msym, logw


@pytest.mark.parametrize("seed", range(30))
def test_reference_equals_exhaustive_enumeration(seed):
    rng = np.random.default_rng(seed)
    Q, src, dst, msym, logw = tiny_machine(rng, quantised=seed % 3 == 0)
    for line in [[]] + [[int(x) for x in rng.integers(1, 3, rng.integers(1, 5))] for _ in range(8)]:
        every = enumerate_all(Q, Q - 1, src, dst, msym, logw, line)
        assert len(set(p for _, p in every)) == len(every)
        every.sort(key=lambda e: -e[0])
        for K in (1, 2, 3, 5):
            vals, paths, tied = kbest(Q, Q - 1, src, dst, msym, logw, line, K)
            assert vals == [v for v, _ in every[:K]], (line, K)
            assert len(set(paths)) == len(paths) == len(vals)
            top = [v for v, _ in every[:K + 1]]
            assert tied == (len(set(top)) < len(top)), (line, K)
            value_of = dict((p, v) for v, p in every)
            assert [value_of[p] for p in paths] == vals, (line, K)
            if not tied:
                assert paths == [p for _, p in every[:K]], (line, K)


def test_reference_refuses_an_epsilon_cycle():
    # 0 -a-> 1, 1 -eps-> 2, 2 -eps-> 1, 1 -b-> 3
    with pytest.raises(CycleError):
        kbest(4, 3, [0, 1, 1, 2], [1, 3, 2, 1], [1, 2, 0, 0], np.log([1.0, 0.5, 0.5, 1.0]), [1, 2], 2)


def test_gpu_test_inputs_exercise_the_lists():
    """of the lines of the GPU test that have a derivation, at least half have two or more and at most 10 % are tied (a tied
    line's paths are not compared with the reference's)"""
    from decode_kbest_cases import all_cases, case
    n_with = n_several = n_tied = 0
    for name in all_cases():
        c = case(name)
        w = c["w"]
        for side, lines, msym, ref in c["sides"]:
            for line, (vals, paths, tied) in zip(lines, ref):
                if not vals:
                    continue
                n_with += 1
                n_tied += tied
                n_several += len(vals) > 1 or len(kbest(w.n_states, w.final, w.src, w.dst, msym, w.logw, line, 2)[0]) > 1
    print("lines with a derivation %d, with several %d, tied %d" % (n_with, n_several, n_tied))
    assert n_with >= 200
    assert 2 * n_several >= n_with
    assert 10 * n_tied <= n_with


def test_kbest_gets_past_the_switches(golden_dir):
    """--kbest=3 on the tutorial machines fails only where the device is needed (-11, "no HIP device"); with a GPU it succeeds"""
    from carmel_amd._capi import lib
    g = lambda n: os.path.join(golden_dir, n)
    rc, out, err = run(["-qbsriWIE", "--kbest=3", g("cat.fsa.trained.noe"), g("spellout.fst.trained")], stdin="c1 c2\n")
    if lib.carmel_hip_device_count() > 0:
        assert rc == 0, err
        return
    assert signed(rc) == -11, err
    assert "not implemented" not in err and "no HIP device" in err and "carmel_hip_decoder_create" in err


@pytest.mark.parametrize("args", [
    ["-qbsriWIE", "--kbest=0"],
    ["-qbsriWIE", "--kbest=2000"],
    ["-qbsriWIE", "--kbest=3", "-k", "2"],
    ["-qsrWIE", "--kbest=3"],
    ["-qbsr", "--kbest=3"],
])
def test_bad_kbest_forms_are_refused(golden_dir, args):
    g = lambda n: os.path.join(golden_dir, n)
    rc, out, err = run(args + [g("cat.fsa.trained.noe"), g("spellout.fst.trained")], stdin="c1 c2\n")
    assert signed(rc) == -12, err
    assert out == "" and "HIP" not in err


def test_help_names_kbest():
    rc, out, err = run(["-h"])
    assert rc == 0 and "--kbest" in out


def test_kbest_kernels_use_no_scratch_memory():
    everything = kernels(device_asm("decode_kbest.hip"))
    ks = {k: v for k, v in everything.items() if "trellis_kernel" in k and "KbNode" in k}
    # the shared trellis kernel around the k-best node in its two tiers, and nothing else: the walk kernel is decode_paths.hip's,
    # in its two passes, and test_decode_host.py holds it to the same
    assert len(ks) == 2 and len(everything) == 2, list(everything)
    for name, (body, tail) in ks.items():
        m = re.search(r"; ScratchSize: (\d+)", tail)
        assert m and int(m.group(1)) == 0, (name, m and m.group(0))
        assert "scratch_" not in body, name
