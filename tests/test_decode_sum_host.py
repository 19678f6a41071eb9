"""CPU: the all-paths sum of a line (carmel -b --sum) -- the numpy reference (decode_sum_ref.py) against exhaustive enumeration,
what the GPU test's random workload contains, the front end's --sum-paths switch where no device is needed, and the sum kernel's
resources.  Nothing here needs a GPU."""
import math
import os
import re

import numpy as np
import pytest

from decode_sum_cases import SEEDS, case, cross_checked
from decode_sum_ref import CycleError, count, forward
from test_decode_host import run, signed
from test_kernel_resources import device_asm, kernels


def tiny_machine(rng):
    """2 .. 6 states, <= 14 arcs, symbols 1 and 2, epsilon arcs only forward in state order, some arcs of weight zero"""
    Q = int(rng.integers(2, 7))
    n = int(rng.integers(Q, 15))
    src = rng.integers(0, Q, n)
    dst = rng.integers(0, Q, n)
    msym = rng.integers(0, 3, n)
    msym[(msym == 0) & (dst <= src)] = 1
    logw = np.log(rng.uniform(0.01, 1.0, n))
    logw[rng.uniform(size=n) < 0.05] = -np.inf
    return Q, src, dst, msym, logw


def derivations(Q, final, src, dst, msym, logw, line):
    """every derivation's weight (a product of probabilities), depth first over (position, state)"""
    out = []

    def go(i, q, p):
        if i == len(line) and q == final:
            out.append(p)
        for k in range(len(src)):
            if src[k] != q or logw[k] == -np.inf:
                continue
            if msym[k] == 0:
                go(i, dst[k], p * math.exp(logw[k]))
            elif i < len(line) and msym[k] == line[i]:
                go(i + 1, dst[k], p * math.exp(logw[k]))

    go(0, 0, 1.0)
    return out


@pytest.mark.parametrize("seed", range(40))
def test_reference_equals_exhaustive_enumeration(seed):
    rng = np.random.default_rng(900 + seed)
    Q, src, dst, msym, logw = tiny_machine(rng)
    for line in [[]] + [[int(x) for x in rng.integers(1, 3, rng.integers(1, 5))] for _ in range(8)]:
        every = derivations(Q, Q - 1, src, dst, msym, logw, line)
        assert count(Q, Q - 1, src, dst, msym, logw, line) == len(every), line
        got = forward(Q, Q - 1, src, dst, msym, logw, line)
        if not every:
            assert got == -np.inf, line
            continue
        want = math.log(math.fsum(every))
        # every path's product is rounded <= 5 times, fsum is exact, the forward pass rounds a few times per node of <= 5 x 6
        assert abs(got - want) <= 1e-13 * max(1.0, abs(want)), (line, got, want)


def test_reference_refuses_an_epsilon_cycle():
    # 0 -a-> 1, 1 -eps-> 2, 2 -eps-> 1, 1 -b-> 3
    args = (4, 3, [0, 1, 1, 2], [1, 3, 2, 1], [1, 2, 0, 0])
    with pytest.raises(CycleError):
        forward(*args, np.log([1.0, 0.5, 0.5, 1.0]), [1, 2])
    with pytest.raises(CycleError):
        count(*args, np.log([1.0, 0.5, 0.5, 1.0]), [1, 2])
    # an arc of weight zero is no arc: no cycle
    assert forward(*args, [0.0, np.log(0.5), -np.inf, 0.0], [1, 2]) == np.log(0.5)


def test_gpu_test_inputs_really_sum():
    """the random workload of test_decode_sum_gpu.py: enough lines have several derivations (so a Viterbi value would fail), enough
    of them few enough for the k-best cross-check, and the epsilon closure is more than one level deep"""
    n_lines = n_cyclic = n_with = n_several = n_mid = n_cross = levels = 0
    for seed in SEEDS:
        c = case(seed)
        for side, lines, ref, counts, n_levels in c["sides"]:
            if ref is None:
                n_cyclic += 1
                continue
            n_lines += len(lines)
            levels = max(levels, n_levels)
            assert [n > 0 for n in counts] == [r > -np.inf for r in ref]
            n_with += sum(n > 0 for n in counts)
            n_several += sum(n > 1 for n in counts)
            n_mid += sum(2 <= n <= 1024 for n in counts)
        n_cross += sum(counts[l] >= 2 for _, _, _, counts, take in cross_checked(c) for l in take)
    print("lines %d, cyclic (machine, side) pairs %d, with a derivation %d, with several %d, with 2 .. 1024 %d, epsilon levels %d"
          % (n_lines, n_cyclic, n_with, n_several, n_mid, levels))
    assert n_cyclic >= 1 and any(case(s)["w"].n_states > 4096 for s in SEEDS) and any(case(s)["lds_off"] for s in SEEDS)
    assert n_with >= 1000
    assert n_several >= 750
    assert n_mid >= 550 and n_cross == n_mid
    assert levels >= 3


@pytest.mark.parametrize("args", [
    ["-q", "--sum-paths"],
    ["-qWIE", "--sum-paths"],
    ["-q", "-t", "--sum-paths"],
    ["-qbsriWIEk", "1", "--sum"],  # carmel's own spelling stays refused (test_decode_host.py pins it): --sum-paths is the switch
    ["-qbsriWIE", "--kbest=3", "--sum"],
])
def test_sum_without_batch_decoding_is_refused(golden_dir, args):
    g = lambda n: os.path.join(golden_dir, n)
    rc, out, err = run(args + [g("cat.fsa.trained.noe"), g("spellout.fst.trained")], stdin="c1 c2\n")
    assert signed(rc) == -12, err
    assert "--sum" in err and "HIP" not in err
    assert out == ""


def test_post_b_is_still_refused(golden_dir):
    g = lambda n: os.path.join(golden_dir, n)
    rc, out, err = run(["-qbsriWIEk", "1", "--sum-paths", "--post-b=x", g("cat.fsa.trained.noe"), g("spellout.fst.trained")],
                       stdin="c1 c2\n")
    assert signed(rc) == -12, err
    assert "--post-b" in err and "not implemented" in err and "HIP" not in err
    assert out == ""


@pytest.mark.parametrize("form", [["-qbsriWIEk", "1"], ["-qbsriWIE", "--kbest=3"], ["-qsriWIEk", "1"]])
def test_sum_gets_past_the_switches(golden_dir, form):
    """--sum-paths with batch decoding fails only where the device is needed (-11, "no HIP device"); with a GPU it succeeds"""
    from carmel_amd._capi import lib
    g = lambda n: os.path.join(golden_dir, n)
    rc, out, err = run(form + ["--sum-paths", g("cat.fsa.trained.noe"), g("spellout.fst.trained")], stdin="c1 c2\n")
    if lib.carmel_hip_device_count() > 0:
        assert rc == 0, err
        assert "Sum (all paths) product of probs=" in err
        return
    assert signed(rc) == -11, err
    assert "not implemented" not in err and "no HIP device" in err and "carmel_hip_decoder_create" in err


def test_help_names_sum():
    rc, out, err = run(["-h"])
    assert rc == 0 and "--sum-paths" in out


def test_sum_kernel_uses_no_scratch_memory():
    everything = kernels(device_asm("decode_sum.hip"))
    ks = {k: v for k, v in everything.items() if "trellis_kernel" in k and "SumNode" in k}
    assert len(ks) == 2 and len(everything) == 2, list(everything)  # the shared trellis kernel around the sum's node, in its two tiers
    for name, (body, tail) in ks.items():
        m = re.search(r"; ScratchSize: (\d+)", tail)
        assert m and int(m.group(1)) == 0, (name, m and m.group(0))
        assert "scratch_" not in body, name
