"""Consolidating duplicate arcs (carmel -C, carmel_hip_consolidate), what can be proved without a device: the Python reference of
the rule (consolidate_ref.py) against exact rational sums, its idempotence, the properties the case machines of
consolidate_cases.py are named for, the kernels' resources, and the front end's usage errors.  Transducer::consolidate is tested
through the front end on a device (test_consolidate_cli_gpu.py)."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from consolidate_cases import (ARC_COUNTS, DECODER_SEEDS, DEFAULT_WAVE_MEMBERS, GRID, HAND, RANDOM_SEEDS, SEGMENT_SIZES, decoder_case,
                               epsilon_acyclic_side, machine, names, reference)
from consolidate_ref import LD, NONE, Consolidated
from test_decode_host import run, signed

NEG_INF = -np.inf


def dyadic_machine(seed):
    """weights k / 2^j, k <= 15, j <= 6; a few states, symbols 0-2, half of the arcs copies of an earlier arc"""
    rng = np.random.default_rng(5000 + seed)
    n = int(rng.integers(1, 60))
    arcs, fracs = [], []
    for _ in range(n):
        f = Fraction(int(rng.integers(1, 16)), 2 ** int(rng.integers(0, 7)))
        if arcs and rng.random() < 0.5:
            key = arcs[int(rng.integers(0, len(arcs)))][:4]
        else:
            key = (int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, 3)))
        arcs.append(key + (f,))
    arcs.sort(key=lambda a: a[0])
    return arcs


@pytest.mark.parametrize("seed", range(20))
def test_reference_sums_equal_exact_fractions_on_dyadic_weights(seed):
    """every weight and so every sum is a multiple of 1/64: the unclamped sum of a segment, taken out of the log domain and rounded
    to that grid, IS the rational sum.  In the log domain the two agree as far as the inputs allow: a member's log is a double,
    within 2^-53 |ln w| of the exact logarithm, which moves the sum's log by at most the largest of those; the longdouble
    arithmetic adds 2^-60 (1 + |value|)"""
    arcs = dyadic_machine(seed)
    cols = list(zip(*arcs))
    logw = np.log(np.array([float(f) for f in cols[4]]))
    ref = Consolidated(cols[0], cols[1], cols[2], cols[3], logw, "sum", False)
    sums, first = {}, {}
    for a, arc in enumerate(arcs):
        sums[arc[:4]] = sums.get(arc[:4], 0) + arc[4]
        first.setdefault(arc[:4], a)
    assert ref.n_kept == len(sums) and ref.kept_id.tolist() == sorted(first.values())
    for j, a in enumerate(ref.kept_id):
        exact = sums[arcs[a][:4]]
        assert Fraction(int(np.rint(np.exp(LD(ref.value[j])) * 64)), 64) == exact, (seed, j)
        want = np.log(LD(exact.numerator)) - np.log(LD(exact.denominator))
        slack = LD(2.0) ** -53 * max(abs(float(x)) for x, arc in zip(logw, arcs) if arc[:4] == arcs[a][:4])
        assert abs(LD(ref.value[j]) - want) <= slack + LD(2.0) ** -60 * (1 + abs(want)), (seed, j)
        assert ref.arc_map[a] == j and ref.size[j] == sum(1 for x in arcs if x[:4] == arcs[a][:4])


@pytest.mark.parametrize("name", names())
def test_consolidating_twice_equals_consolidating_once(name):
    w = machine(name)
    for mode, clamp in GRID:
        once = reference(name, mode, clamp)
        k = once.kept_id
        weights = once.rounded()
        twice = Consolidated(w.src[k], w.dst[k], w.isym[k], w.osym[k], weights, mode, clamp)
        assert twice.n_kept == once.n_kept and twice.kept_id.tolist() == list(range(once.n_kept))
        assert (twice.size == 1).all() and twice.arc_map.tolist() == list(range(once.n_kept))
        assert np.array(twice.value, np.float64).tobytes() == weights.tobytes()
        # what the reference returns hangs together
        live = w.logw > NEG_INF
        assert (once.arc_map[~live] == NONE).all() and (once.arc_map[live] < once.n_kept).all()
        assert once.size.sum() == live.sum() and (np.diff(k.astype(np.int64)) > 0).all()
        assert (once.arc_map[k] == np.arange(once.n_kept)).all()
        assert (np.diff(w.src[k].astype(np.int64)) >= 0).all()  # still state-major


def keys(w):
    return list(zip(w.src.tolist(), w.dst.tolist(), w.isym.tolist(), w.osym.tolist()))


def test_the_case_machines_have_the_properties_they_are_named_for():
    assert machine("no_arcs").n_arcs == 0 and machine("one_arc").n_arcs == 1
    assert (machine("all_neg_inf").logw == NEG_INF).all() and reference("all_neg_inf", "sum", True).n_kept == 0
    w = machine("three_self_loops")
    assert w.n_states == 1 and len(set(keys(w))) == 1 and w.n_arcs == 3 and (w.src == w.dst).all()
    w = machine("dead_first_member")
    r = reference("dead_first_member", "sum", True)
    assert w.logw[0] == NEG_INF and keys(w)[0] == keys(w)[1] == keys(w)[3] and r.kept_id.tolist() == [1, 2] and r.size.tolist() == [2, 1]
    w = machine("interleaved")
    k = keys(w)
    assert k[0] == k[2] == k[4] != k[1] == k[3] and reference("interleaved", "sum", True).arc_map.tolist() == [0, 1, 0, 1, 0]
    w = machine("one_field_apart")
    k = keys(w)
    for pair, field in enumerate(range(4)):  # pair p differs in field p alone
        a, b = k[2 * pair], k[2 * pair + 1]
        assert [x != y for x, y in zip(a, b)] == [f == field for f in range(4)], (pair, a, b)
    assert reference("one_field_apart", "sum", True).n_kept == 8
    w = machine("wide_symbols")
    r = reference("wide_symbols", "sum", True)
    assert r.n_kept == 7 and (r.size == 2).all() and {0xFFFFFFFE, 0x80000005, 5} <= set(w.isym.tolist()) & set(w.osym.tolist())
    assert len({(i & 0x7FFFFFFF, o & 0x7FFFFFFF) for i, o in zip(w.isym.tolist(), w.osym.tolist())}) < 7  # 31 bits a field would merge some
    w = machine("far_state")
    r = reference("far_state", "sum", True)
    assert w.n_states == 70001 and w.n_arcs == 12 and 70000 in w.dst and (70000 & 0xFFFF) in w.dst and r.n_kept == 7
    assert len({(s & 0xFFFF, d & 0xFFFF) for s, d in zip(w.src.tolist(), w.dst.tolist())}) < 7  # 16 bits a state would merge some
    r = reference("sizes", "sum", False)
    assert set(SEGMENT_SIZES) <= set(r.size.tolist())
    assert any(s <= DEFAULT_WAVE_MEMBERS for s in SEGMENT_SIZES) and any(s > 64 * DEFAULT_WAVE_MEMBERS for s in SEGMENT_SIZES)  # lane form, wavefront form, several trips a lane
    assert all(float(v) < 0.0 for v in r.value)  # no clamp hides a sum
    for n in ARC_COUNTS:
        w = machine("count%d" % n)
        assert w.n_arcs == n
        r = reference("count%d" % n, "sum", True)
        assert n == 1 or r.n_kept < n
    assert 3000 <= reference("count10000", "sum", True).size.max() <= 3100
    removed, dead = 0, 0
    for seed in RANDOM_SEEDS:
        w = machine("random%d" % seed)
        assert 1 <= w.n_states <= 12 and w.n_arcs <= 200 and (w.n_arcs == 0 or max(w.isym.max(), w.osym.max()) <= 3)
        removed += w.n_arcs - reference("random%d" % seed, "sum", True).n_kept
        dead += int((w.logw == NEG_INF).sum())
    assert removed > 300 and dead > 100
    for seed in DECODER_SEEDS:  # the machines a Decoder is built on: input epsilons acyclic, lines with derivations, duplicates left
        w, lines = decoder_case(seed)
        r = Consolidated(w.src, w.dst, w.isym, w.osym, w.logw, "sum", False)
        assert epsilon_acyclic_side(w) == 0 and len(lines) >= 12 and r.n_kept < (w.logw > NEG_INF).sum() - 5, (seed, len(lines), r.n_kept)
    w = machine("clamp")
    free = reference("clamp", "sum", False)
    held = reference("clamp", "sum", True)
    assert [float(np.exp(LD(v))) for v in free.value] == pytest.approx([0.5, 1.0, 1.5, 2.0, 3.5], abs=1e-15)
    assert held.rounded().tolist()[2:] == [0.0, float(np.log(2.0)), 0.0] and held.rounded()[0] < 0.0 and abs(held.rounded()[1]) < 1e-15
    assert reference("clamp", "max", True).rounded().tolist() == [float(np.log(x)) for x in (0.25, 0.5, 0.75, 2.0, 3.0)]
    assert len(set(keys(machine("parallel_paths")))) == 3 and "parallel_paths" in HAND


def test_the_reference_refuses_what_the_rule_refuses():
    for bad in ([0.0, np.nan], [np.inf, 0.0]):
        with pytest.raises(ValueError):
            Consolidated([0, 0], [1, 1], [1, 1], [1, 1], bad)
    with pytest.raises(ValueError):
        Consolidated([1, 0], [1, 1], [1, 1], [1, 1], [0.0, 0.0])


def test_consolidate_kernels_use_no_scratch_memory():
    from test_kernel_resources import device_asm, kernels
    ks = {k: v for k, v in kernels(device_asm("consolidate.hip")).items() if "consolidate_" in k and "hipcub" not in k and "rocprim" not in k}
    assert len(ks) == 9, list(ks)
    for name, (body, tail) in ks.items():
        m = re.search(r"; ScratchSize: (\d+)", tail)
        assert m and int(m.group(1)) == 0, (name, m and m.group(0))


def G(golden_dir, name):
    return os.path.join(golden_dir, name)


@pytest.mark.parametrize("args,needle", [
    (["--consolidate-max"], "--consolidate-max applies to -C"), (["--consolidate-unclamped"], "--consolidate-unclamped applies to -C"),
    (["--consolidate-max", "--prune-paths=2"], "--consolidate-max applies to -C"),
    (["-C", "-t"], "-C with -t is"), (["-C", "-S"], "-C with -S is"), (["-C", "-b"], "-C with -b is"), (["-C", "-i"], "-C with -i is"),
    (["-C", "--train-cascade"], "-C with --train-cascade is"), (["-C", "--crp"], "-C with --crp is"),
    (["-C", "--generate-paths=2", "-I"], "-C with --generate-paths=N is"), (["-C", "--generate-pairs=2"], "-C with --generate-pairs=N is"),
    (["-C", "--consolidate-max", "-b"], "-C with -b is"),
])
def test_consolidate_usage_errors(golden_dir, args, needle):
    """each exits -12 naming the option (and what it does not go with), before any device call"""
    rc, out, err = run(args + [G(golden_dir, "train.a.w")])
    assert signed(rc) == -12, err
    assert "HIP" not in err and out == ""
    assert needle in err, err


def test_a_valid_command_reaches_the_device(golden_dir):
    from carmel_amd._capi import lib
    for args in (["-C"], ["-C", "--consolidate-max", "-c"], ["-C", "--consolidate-unclamped", "-HJ"], ["-C", "--prune-paths=2"],
                 ["-C", "--best-paths=2"]):
        rc, out, err = run(["-q"] + args + [G(golden_dir, "train.a.w")])
        if lib.carmel_hip_device_count() > 0:
            assert rc == 0 and out, err
        else:
            assert signed(rc) == -11 and "no HIP device" in err and "not implemented" not in err, err
    rc, out, err = run(["-h"])
    assert rc == 0 and all(x in out + err for x in ("-C consolidates", "--consolidate-max", "--consolidate-unclamped"))


def test_the_abi_without_a_device_fails_with_the_hip_error():
    """no CPU fallback: CARMEL_HIP_ERR_HIP and untouched buffers (with a device the same call succeeds)"""
    import ctypes as C
    from carmel_amd._capi import lib, ptr
    one, w = np.ones(2, np.uint32), np.zeros(2)
    arc_map, kept_id, kept_logw, n = np.full(2, 7, np.uint32), np.full(2, 7, np.uint32), np.full(2, 7.0), C.c_uint64(7)
    rc = lib.carmel_hip_consolidate(0, 2, ptr(one), ptr(one), ptr(one), ptr(one), ptr(w), 0, 1, ptr(arc_map), ptr(kept_id), ptr(kept_logw),
                                    C.byref(n), None)
    if lib.carmel_hip_device_count() > 0:
        assert rc == 0 and n.value == 1 and arc_map.tolist() == [0, 0] and kept_id[0] == 0
        return
    assert rc == -2 and n.value == 7 and (arc_map == 7).all() and (kept_id == 7).all() and (kept_logw == 7.0).all()
