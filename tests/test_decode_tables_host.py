"""CPU: the decoders' host tables (carmel_amd/csrc/decode_tables.cpp), through a small compiled driver.

Every file of tests/golden/decode_tables is a machine ("n_states n_arcs", then "src dst msym osym logw" per arc), a line "--"
and every table as the builder that preceded decode_tables.cpp made it, when the four views were four copies of the same steps
in carmel_hip_decoder::upload_tables: one machine per place where those copies differed (no arcs, one state, a cyclic epsilon
subgraph, a 0M self-loop, a 00 cycle, a cycle that only an arc of weight zero breaks, symbol ids with gaps, duplicate arcs, no
epsilon arcs, deep levels) and ten random ones.  The driver prints the tables under the names of the device structs of
decode.hpp (o. DecodeOutTables, p. DecodePairTables, po. DecodePairOutTables); weights are hexadecimal floats: the comparison
is bit for bit."""
import glob
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "carmel_amd", "csrc")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "decode_tables", "*.txt")))

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "decode_tables.hpp"
using namespace carmel_hip;

template <class T>
static void put(const char* name, const std::vector<T>& v) {
  std::printf("%s %zu:", name, v.size());
  for (T x : v) std::printf(" %lu", (unsigned long)x);
  std::printf("\n");
}
static void put(const char* name, const std::vector<double>& v) {
  std::printf("%s %zu:", name, v.size());
  for (double x : v) std::printf(" %a", x);
  std::printf("\n");
}
static void put(const char* name, unsigned long x) { std::printf("%s = %lu\n", name, x); }

static void put(const std::string& pre, const char* state, const char* other, const FiledBySymbol& f) {
  put((pre + "sym_seg").c_str(), f.sym_seg);
  put((pre + "seg_" + state).c_str(), f.seg_state);
  put((pre + "seg_arc").c_str(), f.seg_arc);
  put((pre + "m_" + other).c_str(), f.other);
  put((pre + "m_w").c_str(), f.w);
  put((pre + "m_id").c_str(), f.id);
}
static void put(const std::string& pre, const char* state, const char* other, const FiledByState& f) {
  put((pre + "lvl_ent").c_str(), f.lvl_ent);
  put((pre + "ent_" + state).c_str(), f.ent_state);
  put((pre + "ent_arc").c_str(), f.ent_arc);
  put((pre + "e_" + other).c_str(), f.other);
  put((pre + "e_w").c_str(), f.w);
  put((pre + "e_id").c_str(), f.id);
}

int main() {
  unsigned Q, n;
  while (std::scanf("%u %u", &Q, &n) == 2) {
    std::vector<uint32_t> src(n), dst(n), msym(n), osym(n);
    std::vector<double> logw(n);
    for (unsigned k = 0; k < n; ++k) {
      char w[64];
      if (std::scanf("%u %u %u %u %63s", &src[k], &dst[k], &msym[k], &osym[k], w) != 5 || src[k] >= Q || dst[k] >= Q) return 2;
      logw[k] = std::strtod(w, nullptr);
    }
    const DecodeTablesHost H = build_decode_tables(Q, src, dst, msym, osym, logw);
    put("n_syms", H.n_syms);
    put("n_levels", H.e.n_levels);
    put("eps_cyclic", H.eps_cyclic);
    put("n_eps", H.n_eps);
    put("", "dst", "src", H.m);
    put("", "dst", "src", H.e);
    put("e_dst", H.e_dst);
    put("st_ent", H.e.st_ent);
    put("eps_in", H.e.has);
    put("a_eps", H.a_eps);
    put("a_flags", H.a_flags);
    put("o.", "src", "dst", H.om);
    put("o.", "src", "dst", H.oe);
    put("o.eps_out", H.oe.has);
    put("pair_levels", H.pair_levels);
    std::printf("pair_cycle = %s\n", H.pair_cycle.c_str());
    put("p.m_osym", H.m.osym);
    put("p.n_levels", H.pe.n_levels);
    put("p.max_seg", H.m.max_seg);
    put("p.", "dst", "src", H.pe);
    put("p.e_osym", H.pe.osym);
    put("p.st_ent", H.pe.st_ent);
    put("po.m_osym", H.om.osym);
    put("po.n_levels", H.poe.n_levels);
    put("po.max_seg", H.om.max_seg);
    put("po.", "src", "dst", H.poe);
    put("po.e_osym", H.poe.osym);
    put("po.eps_out", H.poe.has);
    std::printf("==\n");
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("decode_tables")
    src, exe = str(tmp / "driver.cpp"), str(tmp / "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    # (the sanitizers' runtimes linked in: the driver then runs whatever else the environment loads before it)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", CSRC,
                        src, os.path.join(CSRC, "decode_tables.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if r.returncode != 0:
        pytest.fail(r.stderr[-2000:])
    return exe


def test_there_is_a_fixture_for_every_case():
    names = {os.path.basename(f)[:-4] for f in FIXTURES}
    assert {"empty_machine", "one_state", "cyclic_epsilon", "self_loop_0m", "cycle_00", "cycle_broken_by_inf", "symbol_gaps",
            "duplicate_arcs", "no_epsilon_arcs", "deep_levels"} <= names
    assert len([n for n in names if n.startswith("random_")]) == 10


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_tables_are_those_recorded(driver, path):
    with open(path) as f:
        machine, want = f.read().split("--\n", 1)
    # (memory errors and undefined behaviour end the driver; the leak check at exit needs ptrace, which not every sandbox grants)
    r = subprocess.run([driver], input=machine, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.split("\n")
    for g, w in zip(got, want.split("\n")):  # (name the first table that differs)
        assert g == w
    assert r.stdout == want
