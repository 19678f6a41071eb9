"""CPU: what the GPU tests of batch pair k-best alignments rest on (tests/test_decode_pairs_kbest_gpu.py) -- the reference of
decode_pairs_kbest_ref.py against brute force (the K greatest path-order values over every enumerated derivation, bit for bit),
what the workload of decode_pairs_kbest_cases.py contains, the front end's refusals around --pair-kbest, the help text, and the
new file's kernels: four, without scratch memory, with decode_kbest.hip's two unchanged in number."""
import os
import re

import pytest

from decode_pairs_kbest_cases import CASES, LDS_DOUBLES, SEEDS, V, case, reference
from decode_pairs_ref import enumerate_paths, rescore
from test_decode_host import run, signed
from test_kernel_resources import device_asm, kernels

G = lambda golden_dir, n: os.path.join(golden_dir, n)
MACHINES = ["cat.fsa.trained.noe", "spellout.fst.trained"]
BRUTE_LIMIT = 20000


def test_reference_against_brute_force():
    """every pair with <= 20 000 derivations: the reference's values are the K greatest path-order values over all derivations,
    bit for bit and in order; its paths are derivations with those values; where the best K + 1 are untied, they are THE paths"""
    n_pairs = n_exact = n_skipped = 0
    for seed, tie in CASES:
        c, ref = case(seed, tie), reference(seed, tie)
        K, P = c["K"], c["P"]
        for l, (x, y) in enumerate(c["pairs"]):
            vals, paths, tied = ref[l]
            if c["count"][l] > BRUTE_LIMIT:
                n_skipped += 1
                continue
            every = enumerate_paths(P, x, y, limit=BRUTE_LIMIT)
            assert len(every) == c["count"][l], (seed, tie, l)
            scored = []
            for p in every:
                v = 0.0
                for a in p:
                    v = v + P.logw[a]
                scored.append((float(v), tuple(p)))
            scored.sort(key=lambda t: -t[0])
            assert vals == [v for v, _ in scored[:K]], (seed, tie, l)
            assert len(paths) == len(vals) == min(K, len(every)) and len(set(paths)) == len(paths), (seed, tie, l)
            for v, p in zip(vals, paths):
                fwd, _ = rescore(P, x, y, list(p))
                assert fwd == v, (seed, tie, l, p)
            top = [v for v, _ in scored[:K + 1]]
            assert tied == (len(set(top)) < len(top)), (seed, tie, l)
            if not tied:
                assert paths == [p for _, p in scored[:K]], (seed, tie, l)
                n_exact += 1
            n_pairs += 1
    print("%d pairs against brute force, %d of them path for path, %d beyond %d derivations" % (n_pairs, n_exact, n_skipped, BRUTE_LIMIT))
    assert n_pairs >= 600 and n_exact >= 400


def test_what_the_workload_contains():
    plain = [case(s) for s in SEEDS]
    counts = [(c, n) for c in plain for n in c["count"]]
    n = len(counts)
    assert n == 12 * len(SEEDS)
    assert sum(k >= 2 for _, k in counts) >= 0.30 * n
    assert sum(k >= 5 for _, k in counts) >= 0.10 * n
    assert sum(c["K"] > 1 and k > c["K"] for c, k in counts) >= 40
    assert sum(2 <= k < c["K"] for c, k in counts) >= 40
    assert sum(c["loop"] and k >= 2 for c, k in counts) >= 30
    assert sum(c["diag"] > LDS_DOUBLES for c in plain) >= 3  # seeds whose largest pair is beyond the LDS tier by size
    n_tied = n_untied = 0
    for seed, tie in CASES:
        c, ref = case(seed, tie), reference(seed, tie)
        for k, (_, _, tied) in zip(c["count"], ref):
            if k >= 2:
                n_tied += tied
                n_untied += not tied
    print("%d tied and %d untied pairs with several derivations" % (n_tied, n_untied))
    assert n_tied >= 20 and n_untied >= 150
    for seed, tie in CASES:
        pairs = case(seed, tie)["pairs"]
        assert pairs[0] == ([], []) and pairs[1][0] == [V + 7] and pairs[2][1] == [V + 7], (seed, tie)
        assert len(pairs) == 12 and case(seed, tie)["count"][1:3] == [0, 0], (seed, tie)


@pytest.mark.parametrize("args", [
    ["-qbsriWIEk", "1", "--pair-kbest=3"],  # no --pair-lines
    ["-qsrWIE", "--pair-kbest=3", "--pair-lines=x"],  # neither -b nor -i
    ["-qbsriWIE", "--pair-kbest=0", "--pair-lines=x"],
    ["-qbsriWIE", "--pair-kbest=1025", "--pair-lines=x"],
    ["-qbsriWIEk", "2", "--pair-kbest=3", "--pair-lines=x"],  # -k neither 1 nor N
    ["-qbsriWIE", "--pair-kbest=3", "--kbest=3", "--pair-lines=x"],
    ["-qbsriWIE", "--pair-kbest=3", "--sample-paths=3", "--pair-lines=x"],
    ["-qbsriWIE", "--pair-kbest=3", "--pair-samples=3", "--pair-lines=x"],
    ["-q", "-t", "--pair-kbest=3", "--pair-lines=x"],
    ["-q", "--train-cascade", "--pair-kbest=3", "--pair-lines=x"],
    ["-q", "-S", "--pair-kbest=3", "--pair-lines=x"],
])
def test_pair_kbest_out_of_place_is_refused(golden_dir, args):
    rc, out, err = run(args + [G(golden_dir, m) for m in MACHINES], stdin="c1 c2\n")
    assert signed(rc) == -12, err
    assert "--pair-kbest" in err and "HIP" not in err
    assert out == ""


@pytest.mark.parametrize("form", [["-qbsriWIEk", "1"], ["-qbsriWIE"], ["-qbsriWIEk", "3"], ["-qbsriWIEk", "1", "--sum-paths"],
                                  ["-qsriWIEk", "1"], ["-qbsrOEk", "1", "--pair-alignments=%s"]])
def test_pair_kbest_gets_past_the_switches(golden_dir, tmp_path, form):
    """--pair-kbest=3 with --pair-lines fails only where the device is needed (-11, "no HIP device"); with a GPU it succeeds"""
    from carmel_amd._capi import lib
    other = tmp_path / "other"
    other.write_text("c1\n")
    form = [f % (tmp_path / "align") if "%s" in f else f for f in form]
    rc, out, err = run(form + ["--pair-kbest=3", "--pair-lines=%s" % other] + [G(golden_dir, m) for m in MACHINES], stdin="c1 c2\n")
    if lib.carmel_hip_device_count() > 0:
        assert rc == 0, err
        assert len(out.split("\n")) == 4  # three lines for the one pair
        return
    assert signed(rc) == -11, err
    assert "not implemented" not in err and "no HIP device" in err and "carmel_hip_decoder_create" in err


def test_kbest_with_pair_lines_points_to_pair_kbest(golden_dir):
    """--kbest=N with --pair-lines stays refused before any device call; its message names both switches"""
    rc, out, err = run(["-qbsriWIE", "--kbest=3", "--pair-lines=x"] + [G(golden_dir, m) for m in MACHINES], stdin="c1 c2\n")
    assert signed(rc) == -12 and "--pair-lines" in err and "--pair-kbest" in err and "HIP" not in err and out == ""


def test_help_names_pair_kbest():
    rc, out, err = run(["-h"])
    assert rc == 0 and "--pair-kbest" in out


def test_pair_kbest_kernels_use_no_scratch_memory():
    ks = kernels(device_asm("decode_pairs_kbest.hip"))
    assert len(ks) == 4, list(ks)  # the k-list pair trellis in its two tiers, the walk's two passes
    assert sum("pair_kbest_trellis_kernel" in k for k in ks) == 2
    assert sum("pair_kbest_walk_kernel" in k for k in ks) == 2
    for name, (body, tail) in ks.items():
        m = re.search(r"; ScratchSize: (\d+)", tail)
        assert m and int(m.group(1)) == 0, (name, m and m.group(0))
        assert "scratch_" not in body, name


def test_the_one_sided_kbest_object_keeps_its_kernels():
    ks = kernels(device_asm("decode_kbest.hip"))
    assert len(ks) == 2 and all("trellis_kernel" in k and "KbNode" in k for k in ks), list(ks)
    for name, (body, tail) in ks.items():
        m = re.search(r"; ScratchSize: (\d+)", tail)
        assert m and int(m.group(1)) == 0 and "scratch_" not in body, name
