"""The K best paths of the whole machine (carmel --best-paths=N, carmel_hip_decoder_best_paths), what can be proved without a
device: the Python reference of the rule (best_paths_ref.py) against an exhaustive enumerator where every sum is exact, its
read-out, the host-only table builder and cycle search (csrc/decode_best_paths_tables.cpp) in a stand-alone program under
ASan/UBSan, and the front end's usage errors."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from best_paths_cases import HAND, KS, RANDOM_SEEDS, REFUSED, machine, names, random_case, reference
from best_paths_ref import NONE, Machine, enumerate_walks, merge, positive_cycle_arc, read_out, rounds, sorted_walks
from test_decode_host import run, signed

CSRC = os.path.join(ROOT, "carmel_amd", "csrc")
K_ENUM = 4


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_reference_equals_the_enumerator_on_dyadic_machines(seed):
    """log weights -m / 8, m in 4 .. 12: every sum is exact, so the rule's lists are the walks sorted by (value desc, length asc,
    last arc asc, then the prefix in the same order).  L is at least the longest path returned and large enough that the K-th
    value is strictly better than any walk of L + 1 arcs (or more: every weight is negative) can be."""
    w = random_case(seed, dyadic=True)
    m = Machine(w)
    got = read_out(m, rounds(m, K_ENUM)[0])
    assert got, "the spine makes the final state reachable"
    w_max = max(x for x in m.logw if x > -np.inf)
    assert w_max < 0.0
    L = max(len(p) for _, _, p in got)
    if len(got) == K_ENUM:
        while (L + 1) * w_max >= got[-1][0]:
            L += 1
        assert got[-1][0] > (L + 1) * w_max
    else:  # fewer than K paths exist: the machine's walks to the final state are finitely many, none longer than |Q| - 1 arcs ...
        L = max(L, m.n_states) + 2  # ... so a cycle-free bound and two more arcs show that nothing longer turns up
    walks = enumerate_walks(m, L)
    assert len(walks) < 3000000
    want = sorted_walks(m, walks, K_ENUM)
    assert [tuple(p) for _, _, p in got] == list(want), (seed, L)
    if len(got) < K_ENUM:
        assert len(walks) == len(got)


@pytest.mark.parametrize("name", [n for n in names() if n not in ("medium", "hub", "chain")])
def test_worklist_equals_the_literal_rounds(name):
    """a state none of whose sources' lists changed keeps its list: the worklist gives the lists of recomputing every state"""
    m = Machine(machine(name))
    for K in (1, 5):
        assert rounds(m, K, worklist=True)[0] == rounds(m, K, worklist=False)[0]


@pytest.mark.parametrize("name", names())
def test_read_out_terminates_with_decreasing_lengths(name):
    """read_out asserts that every step back shortens the length by one and ends at the empty path of state 0"""
    for K in KS:
        paths = reference(name, K)
        m = Machine(machine(name))
        assert len(paths) <= K
        for value, _, arcs in paths:
            q = 0
            for a in arcs:
                assert m.src[a] == q and m.logw[a] > -np.inf
                q = m.dst[a]
            assert q == m.final
        assert len({tuple(p) for _, _, p in paths}) == len(paths)
        vals = [v for v, _, _ in paths]
        assert vals == sorted(vals, reverse=True)


def test_self_loop_trap():
    """the zero-weight self-loop has a lower arc id than the arc entering its state; ordered by (value, arc id) alone, rank 0 of
    state 1 would be (loop, rank 0) -- itself.  With the length key rank r takes the loop r times."""
    m = Machine(HAND["self_loop_trap"])
    lists = rounds(m, 5)[0]
    assert [e[1:] for e in lists[1]] == [(2, 3, 0), (3, 1, 0), (4, 1, 1), (5, 1, 2), (6, 1, 3)]
    assert [p for _, _, p in read_out(m, lists)] == [[0, 3] + [1] * r + [2] for r in range(5)]


def test_hand_made_edges():
    assert [p for _, _, p in reference("start_is_final", 5)] == [[], [0], [0, 0], [2], [1, 3]]
    assert reference("unreachable", 5) == []
    assert len(reference("dag3", 16)) == 3
    assert [p for _, _, p in reference("zero_cycle", 5)] == [[0] + [1, 0] * r for r in range(5)]
    assert [p for _, _, p in reference("parallel", 16)] == [[a, b] for b in (3, 4) for a in (0, 1, 2)]
    assert reference("positive_off_cycle", 2)[0][0] > 0.0
    assert len(reference("hub", 16)) == 16 and len(reference("chain", 16)) == 1
    assert merge(Machine(HAND["dag3"]), 0, [[(0.0, 0, NONE, 0)], [], [], []], 4) == [(0.0, 0, NONE, 0)]
    for name in names():
        assert positive_cycle_arc(machine(name)) is None, name
    for name, (w, arc) in REFUSED.items():
        assert positive_cycle_arc(w) == arc, name


DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "decode_best_paths_tables.hpp"
using namespace carmel_hip;

template <class T>
static void put(const char* name, const std::vector<T>& v) {
  std::printf("%s", name);
  for (T x : v) std::printf(" %lu", (unsigned long)x);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc > 1) {  // a cycle of n states with one arc of weight above 1: a recursive search would be n frames deep
    const unsigned n = (unsigned)std::atol(argv[1]);
    std::vector<uint32_t> src(n), dst(n);
    std::vector<double> logw(n, -0.5);
    for (unsigned k = 0; k < n; ++k) {
      src[k] = k;
      dst[k] = (k + 1) % n;
    }
    logw[n - 2] = 0.25;
    std::printf("%ld\n", (long)positive_cycle_arc(build_best_paths_tables(n, src, dst, logw), src, dst, logw));
    logw[n - 1] = -1.0 / 0.0;  // the cycle is cut: the chain is legal
    std::printf("%ld\n", (long)positive_cycle_arc(build_best_paths_tables(n, src, dst, logw), src, dst, logw));
    return 0;
  }
  unsigned Q, n;
  while (std::scanf("%u %u", &Q, &n) == 2) {
    std::vector<uint32_t> src(n), dst(n);
    std::vector<double> logw(n);
    for (unsigned k = 0; k < n; ++k) {
      char w[64];
      if (std::scanf("%u %u %63s", &src[k], &dst[k], w) != 3 || src[k] >= Q || dst[k] >= Q) return 2;
      logw[k] = std::strtod(w, nullptr);
    }
    const BestPathsTablesHost H = build_best_paths_tables(Q, src, dst, logw);
    put("in_off", H.in_off);
    put("in_src", H.in_src);
    put("in_id", H.in_id);
    put("out_off", H.out_off);
    put("out_dst", H.out_dst);
    std::printf("in_w");
    for (double x : H.in_w) std::printf(" %a", x);
    std::printf("\ncycle %ld\n==\n", (long)positive_cycle_arc(H, src, dst, logw));
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("best_paths_tables")
    src, exe = str(tmp / "driver.cpp"), str(tmp / "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", CSRC,
                        src, os.path.join(CSRC, "decode_best_paths_tables.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if r.returncode != 0:
        pytest.fail(r.stderr[-2000:])
    return exe


def test_table_builder_and_cycle_search(driver):
    """the host-only builder, stand-alone under ASan/UBSan: the arcs by destination and by source in arc-id order, only arcs that
    exist, and the arc on a cycle with a weight above 1 that the reference's closure names"""
    cases = [machine(n) for n in names()] + [w for w, _ in REFUSED.values()]
    text = ""
    for w in cases:
        text += "%d %d\n" % (w.n_states, w.n_arcs)
        text += "".join("%d %d %s\n" % (s, t, "-inf" if x == -np.inf else float(x).hex()) for s, t, x in zip(w.src, w.dst, w.logw))
    r = subprocess.run([driver], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = r.stdout.split("==\n")[:-1]
    assert len(blocks) == len(cases)
    for w, block in zip(cases, blocks):
        got = dict(line.split(" ", 1) if " " in line else (line, "") for line in block.split("\n")[:-1])
        m = Machine(w)
        ints = lambda key: [int(x) for x in got[key].split()]
        assert ints("in_off") == list(np.concatenate([[0], np.cumsum([len(x) for x in m.ins])]))
        assert ints("out_off") == list(np.concatenate([[0], np.cumsum([len(x) for x in m.outs])]))
        assert ints("in_src") == [s for q in m.ins for s, _, _ in q]
        assert ints("in_id") == [a for q in m.ins for _, _, a in q]
        assert [float.fromhex(x) for x in got["in_w"].split()] == [x for q in m.ins for _, x, _ in q]
        assert ints("out_dst") == [t for q in m.outs for t, _, _ in q]
        want = positive_cycle_arc(w)
        assert ints("cycle") == [-1 if want is None else want]


def test_cycle_search_is_not_recursive(driver):
    """a cycle of 10^6 states: the arc above 1 is found; with the cycle cut the chain is legal"""
    r = subprocess.run([driver, "1000000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["999998", "-1"]


def test_best_paths_kernels_use_no_scratch_memory():
    """the wave form keeps a lane's best head in registers and the head counters in global memory: nothing is indexed per lane"""
    import re
    from test_kernel_resources import device_asm, kernels
    ks = kernels(device_asm("decode_best_paths.hip"))
    assert len(ks) == 6 and all("best_paths_" in k for k in ks), list(ks)
    for name, (body, tail) in ks.items():
        m = re.search(r"; ScratchSize: (\d+)", tail)
        assert m and int(m.group(1)) == 0, (name, m and m.group(0))
        assert "scratch_" not in body, name


def G(golden_dir, name):
    return os.path.join(golden_dir, name)


@pytest.mark.parametrize("args,needle", [
    (["--best-paths=0"], "--best-paths=N needs 1 <= N <= 1024"), (["--best-paths=1025"], "--best-paths=N needs 1 <= N <= 1024"),
    (["--best-paths=3", "-b"], "with -b is"), (["--best-paths=3", "-i"], "with -i is"), (["--best-paths=3", "-s"], "with -s is"),
    (["--best-paths=3", "-r"], "with -r is"), (["--best-paths=3", "-t"], "with -t is"),
    (["--best-paths=3", "--train-cascade"], "with --train-cascade is"), (["--best-paths=3", "--crp"], "with --crp is"),
    (["--best-paths=3", "-S"], "with -S is"), (["--best-paths=3", "-F", "out"], "with -F is"),
    (["--best-paths=3", "--pair-lines=x"], "with --pair-lines=FILE is"), (["--best-paths=3", "--kbest=3"], "with --kbest=N is"),
    (["--best-paths=3", "--sample-paths=3"], "with --sample-paths=N is"),
    (["--best-paths=3", "--generate-paths=3"], "with --generate-paths=N is"),
    (["--best-paths=3", "--generate-pairs=3"], "with --generate-pairs=N is"),
    (["--best-paths=3", "-k", "2"], "--best-paths=N with -k m: m must be 1 or N"),
])
def test_best_paths_usage_errors(golden_dir, args, needle):
    """each exits -12 naming --best-paths and the option it does not go with (the whole phrase: "-b" alone is part of
    "--best-paths"), before any device call"""
    rc, out, err = run(args + [G(golden_dir, "train.a.w")])
    assert signed(rc) == -12, err
    assert "HIP" not in err and out == ""
    assert needle in err and "--best-paths=N" in err, err


def test_k_without_b_is_still_refused_and_names_best_paths(golden_dir):
    rc, out, err = run(["-k", "3", G(golden_dir, "train.a.w")])
    assert signed(rc) == -12 and out == ""
    assert "not implemented" in err and "--best-paths" in err, err
    rc, out, err = run(["-h"])
    assert rc == 0 and "--best-paths=N" in out + err
