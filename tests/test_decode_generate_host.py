"""CPU: batch generation (carmel_hip_decoder_generate; carmel -G / -g) -- the reference of decode_generate_ref.py against its
exact enumerator (frequencies, mean attempts), its paths on the committed workload of decode_generate_cases.py (valid walks, no
ambiguous draw, pinned counts), the host-only table builder under AddressSanitizer and UBSan against the reference's lists, the
front end's switches where no device is needed, and the new kernels' resources.  Nothing here needs a GPU."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from decode_generate_cases import (HAND, MODES, N_FREQ, N_PATHS, SEED_FREQ, TRIES, UNREACHABLE, check_frequencies, exact,
                                   frequency_cases, machine, model, names, reference, workload)
from decode_generate_ref import (CONDITIONAL, JOINT, Machine, choose, frequencies, generate, is_walk, path_order_weight,
                                 reported_weight)
from test_decode_host import run, signed
from test_kernel_resources import device_asm, kernels

CSRC = os.path.join(ROOT, "carmel_amd", "csrc")


@pytest.mark.parametrize("name,mode", frequency_cases())
def test_reference_frequencies_and_attempts_against_the_enumerator(name, mode):
    """N = 4000 paths: every accepted path's share against its exact probability within 5 (sqrt(p (1 - p) / n) + 1 / n), and the
    mean number of attempts against 1 / P(accept) within 5 standard errors of a geometric variable's mean (plus 1e-9 for the
    enumerator's own rounding of P(accept)).  Only cases with P(accept) >= 0.3: 64 attempts then fail with probability < 1e-9."""
    L, dist, accept = exact(name, mode)
    assert abs(sum(dist.values()) - 1.0) <= 1e-9 and accept >= 0.3
    m = model(name)
    paths, tries, _, _ = generate(m, mode, N_FREQ, SEED_FREQ, L, TRIES)
    assert all(p is not None and is_walk(m, p, L) for p in paths)
    worst = check_frequencies(frequencies(paths), dist, N_FREQ, (name, mode))
    mean, se = sum(tries) / float(N_FREQ), math.sqrt((1.0 - accept) / accept ** 2 / N_FREQ)
    print("%s %s: %d accepted paths, worst |f - p| %.2f of the bound's unit; mean attempts %.4f, 1 / P(accept) %.4f, s.e. %.4f"
          % (name, mode, len(dist), worst, mean, 1.0 / accept, se))
    assert abs(mean - 1.0 / accept) <= 5.0 * se + 1e-9, (name, mode, mean, 1.0 / accept, se)


def test_frequency_test_has_machines():
    cases = frequency_cases()
    assert len({n for n, _ in cases}) >= 20 and {m for _, m in cases} == set(MODES), cases
    assert all(2 <= len(exact(n, m)[1]) <= 64 for n, m in cases)


def test_workload_paths_are_walks_and_no_draw_is_ambiguous():
    """the committed workload: pinned counts, every reference path a valid walk within its machine's L, 0 ambiguous draws"""
    wl = workload()
    n_paths = n_draws = n_amb = n_retried = n_empty = 0
    for name, mode in wl:
        m, L = model(name), machine(name)[1]
        paths, tries, draws, amb = reference(name, mode)
        assert len(paths) == len(tries) == N_PATHS
        for p, t in zip(paths, tries):
            assert is_walk(m, p, L), (name, mode, p)
            assert 1 <= t <= TRIES
            assert abs(reported_weight(m, p) - path_order_weight(m, p)) <= 1e-12 * max(1.0, abs(path_order_weight(m, p)))
            n_retried += t > 1
            n_empty += not p
        n_paths += len(paths)
        n_draws += draws
        n_amb += amb
    left_out = [(n, mode) for n in names() for mode in MODES if reference(n, mode) is None]
    print("workload: %d (machine, mode) of %d machines, %d paths (%d retried, %d empty), %d draws, %d ambiguous; left out %s"
          % (len(wl), len({n for n, _ in wl}), n_paths, n_retried, n_empty, n_draws, n_amb, left_out))
    assert set(HAND) <= {n for n, _ in wl}
    assert (len(wl), len({n for n, _ in wl}), n_paths, n_draws, n_retried) == (96, 49, 19200, 138304, 4163)
    assert n_amb == 0


def test_edges_of_the_rule():
    # t == S: the first k with cum_k == S, not a later arc whose p_k vanished beside it.  (The clause completes the rule; the
    # 53-bit uniform never gets there: u <= 1 - 2^-53, and S 2^-53 is at least half an ulp of S, a whole one below a power of two)
    assert choose([1.0, 3.0, 3.0], 1.0)[0] == 1 and choose([1.0, 3.0, 3.0], 1.0 - 2.0 ** -53)[0] == 1
    assert all(s * (1.0 - 2.0 ** -53) < s for s in (1.0, 1.0 + 2.0 ** -52, 3.0, 2.0 - 2.0 ** -52, 1e300, 5e-324 * 2 ** 60))
    assert choose([0.0, 1.0], 0.0)[0] == 1  # an arc whose p_k underflowed is never chosen, first in its list either
    m = model("underflow")
    assert all(0 not in p for mode in MODES for p in reference("underflow", mode)[0])
    assert m.groups[JOINT][0][0][1] == [0.0, math.exp(-1.0), math.exp(-1.0) + 1.0]
    # a zero-weight arc is in no list
    z = model("zero_first_and_last")
    assert z.groups[JOINT][0][0][0] == [1, 2, 3] and [g[0] for g in z.groups[CONDITIONAL][0]] == [[1, 2], [3]]
    # groups in ascending symbol id, epsilon first
    g = model("groups")
    assert [[g.msym[k] for k in arcs] for arcs, _ in g.groups[CONDITIONAL][0]] == [[0], [1, 1, 1], [2]]
    # the start state is final: the empty path, one attempt, weight 0.0
    paths, tries, draws, _ = reference("start_is_final", JOINT)
    assert paths == [[]] * N_PATHS and tries == [1] * N_PATHS and draws == 0 and reported_weight(model("start_is_final"), []) == 0.0
    # exactly L arcs is accepted, L + 1 never; one arc fewer and the longer road is all there is: every path fails
    for mode in MODES:
        assert {tuple(p) for p in reference("exactly_L", mode)[0]} == {(0, 1, 2, 3)}
        assert any(t > 1 for t in reference("exactly_L", mode)[1])
        assert generate(model("exactly_L"), mode, 20, 1, 3, 8)[0] == [None] * 20
    # an unreachable final state: every path fails
    u = Machine(UNREACHABLE.n_states, UNREACHABLE.final, UNREACHABLE.src, UNREACHABLE.dst, UNREACHABLE.isym, UNREACHABLE.logw)
    assert generate(u, JOINT, 5, 0, 12, 16) == ([None] * 5, [16] * 5, 5 * 16 * 12, 0)


DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "decode_generate_tables.hpp"
using namespace carmel_hip;

template <class T>
static void put(const char* name, const std::vector<T>& v) {
  std::printf("%s", name);
  for (T x : v) std::printf(" %lu", (unsigned long)x);
  std::printf("\n");
}
static void put(const char* name, const std::vector<double>& v) {
  std::printf("%s", name);
  for (double x : v) std::printf(" %a", x);
  std::printf("\n");
}

int main() {
  unsigned Q, n;
  while (std::scanf("%u %u", &Q, &n) == 2) {
    std::vector<uint32_t> src(n), dst(n), msym(n);
    std::vector<double> logw(n);
    for (unsigned k = 0; k < n; ++k) {
      char w[64];
      if (std::scanf("%u %u %u %63s", &src[k], &dst[k], &msym[k], w) != 4 || src[k] >= Q || dst[k] >= Q) return 2;
      logw[k] = std::strtod(w, nullptr);
    }
    const GenerateTablesHost H = build_generate_tables(Q, src, dst, msym, logw);
    put("j.list_arc", H.joint.list_arc);
    put("j.id", H.joint.id);
    put("j.dst", H.joint.dst);
    put("j.cum", H.joint.cum);
    put("c.st_grp", H.st_grp);
    put("c.grp_sym", H.grp_sym);
    put("c.list_arc", H.cond.list_arc);
    put("c.id", H.cond.id);
    put("c.dst", H.cond.dst);
    put("c.cum", H.cond.cum);
    std::printf("==\n");
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("decode_generate_tables")
    src, exe = str(tmp / "driver.cpp"), str(tmp / "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", CSRC,
                        src, os.path.join(CSRC, "decode_generate_tables.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if r.returncode != 0:
        pytest.fail(r.stderr[-2000:])
    return exe


def expected_tables(w, msym):
    """the builder's tables as the reference's lists give them"""
    m = Machine(w.n_states, w.final, w.src, w.dst, msym, w.logw)
    hexes = lambda xs: [float(x).hex() for x in xs]
    out = {}
    list_arc, ids, cum = [0], [], []
    for s in range(m.Q):
        for arcs, c in m.groups[JOINT][s]:
            ids += arcs
            cum += c
        list_arc.append(len(ids))
    out["j.list_arc"], out["j.id"], out["j.dst"], out["j.cum"] = list_arc, ids, [m.dst[k] for k in ids], hexes(cum)
    st_grp, grp_sym, list_arc, ids, cum = [0], [], [0], [], []
    for s in range(m.Q):
        for arcs, c in m.groups[CONDITIONAL][s]:
            grp_sym.append(m.msym[arcs[0]])
            ids += arcs
            cum += c
            list_arc.append(len(ids))
        st_grp.append(len(grp_sym))
    out["c.st_grp"], out["c.grp_sym"], out["c.list_arc"] = st_grp, grp_sym, list_arc
    out["c.id"], out["c.dst"], out["c.cum"] = ids, [m.dst[k] for k in ids], hexes(cum)
    return out


def test_table_builder_under_the_sanitizers_gives_the_reference_lists(driver):
    """every machine of the cases from both sides, the machine without arcs and one whose only arc has weight zero, through a
    stand-alone program built with -fsanitize=address,undefined: the tables are the reference's lists, the sums bit for bit"""
    from carmel_amd.model import Wfst
    machines = [(machine(n)[0], side) for n in names() for side in (0, 1)]
    machines += [(UNREACHABLE, 0), (Wfst(2, 1, [], [], [], [], []), 0), (Wfst(2, 1, [0], [1], [1], [1], [-np.inf]), 0)]
    text = ""
    for w, side in machines:
        msym = w.osym if side else w.isym
        text += "%d %d\n" % (w.n_states, w.n_arcs)
        text += "".join("%d %d %d %s\n" % (w.src[k], w.dst[k], msym[k], "-inf" if np.isneginf(w.logw[k]) else float(w.logw[k]).hex())
                        for k in range(w.n_arcs))
    r = subprocess.run([driver], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = r.stdout.split("==\n")[:-1]
    assert len(blocks) == len(machines)
    for (w, side), block in zip(machines, blocks):
        want = expected_tables(w, w.osym if side else w.isym)
        got = {}
        for line in block.split("\n")[:-1]:
            f = line.split(" ")
            got[f[0]] = [float.fromhex(x).hex() for x in f[1:]] if f[0].endswith("cum") else [int(x) for x in f[1:]]
        assert got == want, (w.n_states, w.n_arcs, side, [k for k in want if got.get(k) != want[k]])


G = lambda golden_dir, n: os.path.join(golden_dir, n)


@pytest.mark.parametrize("args,needle", [
    (["-q", "--generate-paths=3", "-IWE", "--generate-pairs=3"], "--generate-pairs"),  # both at once
    (["-q", "--generate-paths=0", "-IWE"], "--generate-paths"),
    (["-q", "--generate-pairs=0"], "--generate-pairs"),
    (["-q", "--generate-pairs=4294967297"], "--generate-pairs"),
    (["-q", "--generate-pairs=3", "--generate-max-arcs=0"], "--generate-max-arcs"),
    (["-q", "--generate-pairs=3", "--generate-max-arcs=1048577"], "--generate-max-arcs"),
    (["-q", "--generate-pairs=3", "--generate-tries=0"], "--generate-tries"),
    (["-q", "--generate-pairs=3", "--generate-tries=65537"], "--generate-tries"),
    (["-q", "--generate-pairs=3", "--generate-max-arcs=1000", "--generate-tries=65536"], "--generate-max-arcs"),  # the product
    (["-q", "--generate-max-arcs=10"], "--generate-max-arcs"),  # nothing to generate
    (["-q", "--generate-tries=10"], "--generate-tries"),
    (["-q", "--generate-paths=3"], "--generate-paths"),  # the arc path form stays refused
    (["-qb", "--generate-pairs=3"], "-b"),
    (["-qi", "--generate-pairs=3"], "-i"),
    (["-qs", "--generate-pairs=3"], "-s"),
    (["-qk", "1", "--generate-pairs=3"], "-k"),
    (["-q", "--generate-pairs=3", "--kbest=2"], "--kbest"),
    (["-q", "--generate-pairs=3", "--sample-paths=2"], "--sample-paths"),
    (["-q", "--generate-pairs=3", "--pair-lines=x"], "--pair-lines"),
    (["-qt", "--generate-pairs=3"], "-t"),
    (["-q", "--train-cascade", "--generate-pairs=3"], "--train-cascade"),
    (["-qS", "--generate-paths=3", "-IWE"], "-S"),
    (["-q", "--crp", "--generate-pairs=3"], "--crp"),
])
def test_generate_usage_errors(golden_dir, args, needle):
    """each exits -12 naming the switch, before any device call"""
    rc, out, err = run(args + [G(golden_dir, "cat.fsa.trained.noe"), G(golden_dir, "spellout.fst.trained")])
    assert signed(rc) == -12, err
    assert "HIP" not in err and out == ""
    assert needle in err and "--generate-" in err, err


@pytest.mark.parametrize("args,long_option", [(["-g", "5"], "--generate-pairs"), (["-G", "3"], "--generate-paths"),
                                              (["-L", "20"], "--generate-max-arcs")])
def test_carmels_own_switches_stay_refused_and_name_the_long_option(golden_dir, args, long_option):
    rc, out, err = run(args + [G(golden_dir, "train.a.w")])
    assert signed(rc) == -12 and out == "", err
    assert "not implemented" in err and args[0] in err and long_option in err, err


@pytest.mark.parametrize("form", [["-q", "--generate-pairs=5"], ["-q", "--generate-pairs=5", "-R", "7", "--generate-max-arcs=20",
                                                                 "--generate-tries=8"],
                                  ["-qIWE", "--generate-paths=5"], ["-qOWEQ", "--generate-paths=5"], ["-q@", "--generate-paths=5"]])
def test_generate_gets_past_the_switches(golden_dir, form):
    """fails only where the device is needed (-11, "no HIP device"); with a GPU it succeeds"""
    from carmel_amd._capi import lib
    rc, out, err = run(form + [G(golden_dir, "cat.fsa.trained.noe"), G(golden_dir, "spellout.fst.trained")])
    if lib.carmel_hip_device_count() > 0:
        assert rc == 0 and len(out.split("\n")) - 1 in (5, 10), err
        return
    assert signed(rc) == -11, err
    assert "not implemented" not in err and "no HIP device" in err and "carmel_hip_decoder_create" in err


def test_help_names_the_generate_options():
    rc, out, err = run(["-h"])
    assert rc == 0
    for option in ("--generate-paths", "--generate-pairs", "--generate-max-arcs", "--generate-tries"):
        assert option in out


def test_the_library_exports_the_entry_point():
    from carmel_amd._capi import SYMBOLS, lib
    assert "carmel_hip_decoder_generate" in SYMBOLS and lib.carmel_hip_decoder_generate.argtypes is not None
    assert lib.carmel_hip_decoder_generate(None, 0, 1, 0, 0, 10, 10, None) == -1  # CARMEL_HIP_ERR_ARG: a null handle


def test_generate_kernels_use_no_scratch_memory():
    ks = kernels(device_asm("decode_generate.hip"))
    assert len(ks) == 4 and all("decode_generate_walk_kernel" in k for k in ks), list(ks)  # two modes, two passes
    for name, (body, tail) in ks.items():
        m = re.search(r"; ScratchSize: (\d+)", tail)
        assert m and int(m.group(1)) == 0, (name, m and m.group(0))
        assert "scratch_" not in body, name


@pytest.mark.parametrize("src,names_of", [("decode.hip", ["decode_trellis_kernelILb0E", "decode_trellis_kernelILb1E"]),
                                          ("decode_paths.hip", ["decode_walk_kernelILb0E", "decode_walk_kernelILb1E"])])
def test_the_objects_the_handle_lives_in_keep_their_kernels(src, names_of):
    """generation adds a member to the handle and a line to carmel_hip_decoder_set_weights (decode.hip) and uses the chunk
    bracket of decode_paths.hip: neither object gains a kernel"""
    ks = kernels(device_asm(src))
    assert len(ks) == len(names_of) and all(any(n in k for k in ks) for n in names_of), list(ks)
