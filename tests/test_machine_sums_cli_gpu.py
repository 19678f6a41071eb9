"""GPU: the front end's --machine-sums and --machine-counts=FILE on two small cascades written here (the tutorial machines under
tests/golden/ all have a cycle among their useful states: one of them is the refused case).  A cascade is composed and listed once
(-HJZ: an arc a line, weights as e^x with 15 significant digits, which the front end and Python read back to the same doubles); the
listing is the machine both sides then work on: the front end prints its two lines for it, machine_sums_ref.py computes N, Z and
ln gamma from the same text.  With -C and with --prune-paths=W the front end's own listing of the consolidated or pruned machine is
the reference's input, so the check is that the sums are taken after those stages, of that machine.

Tolerances.  The printed sum is Z, or e^Z, to 15 significant digits: 5e-15 (1 + |Z|), beside the bound E(final) of machine_sums_ref.py.  Where
the reference reads a listing that the front end printed from weights it holds to more digits (the cascade's members, the
consolidated and the pruned machine), every arc's log weight is off by at most 5e-15 |w|, every path's by that times its arcs, and
so is the sum: (levels - 1) 5e-15 max |w| more."""
import math
import os
import re

import numpy as np
import pytest

from machine_sums_ref import LD, MachineSums
from test_decode_gpu import run
from test_decode_host import signed
from test_prune_cli_gpu import ARC_LINE

pytestmark = pytest.mark.gpu

PRINT = 5e-15  # 15 significant digits
# a lattice of three positions with parallel arcs, and a string; each goes through a one-state channel that ends on an epsilon arc
LATTICE = """3
(0 (1 a a 0.5) (1 b b 0.25) (1 a a 0.125))
(1 (2 a a 0.5) (2 b b 0.5) (3 b b 0.1))
(2 (3 a a 0.9) (3 b b 0.3) (3 a a 0.05))
(3)
"""
STRING = """4
(0 (1 a a))
(1 (2 b b 0.5))
(2 (3 a a))
(3 (4 b b))
(4)
"""
CHANNEL = """1
(0 (1 *e* *e* 0.7) (0 a c .6) (0 a d .4) (0 b d .2) (0 b e .8) (0 a c .1))
(1)
"""
CASCADES = {"lattice": LATTICE, "string": STRING}


def parse(text):
    """-> (Wfst, rows): an -HJZ listing, the states numbered as they appear (the start state has the first line)"""
    from carmel_amd.model import Wfst
    lines = text.split("\n")[1:-1]
    rows = [ARC_LINE.match(l).groups() for l in lines]
    ids = {}
    for r in rows:
        ids.setdefault(r[0], len(ids))
    for r in rows:
        ids.setdefault(r[1], len(ids))
    final = ids.setdefault(text.split("\n")[0], len(ids))
    src = [ids[r[0]] for r in rows]
    assert src == sorted(src) and src[0] == 0
    one = np.ones(len(rows), np.uint32)
    return Wfst(len(ids), final, src, [ids[r[1]] for r in rows], one, one, [float(r[4]) for r in rows]), rows


def members(tmp_path, case):
    a, b = str(tmp_path / (case + ".fsa")), str(tmp_path / "channel.fst")
    with open(a, "w") as f:
        f.write(CASCADES[case])
    with open(b, "w") as f:
        f.write(CHANNEL)
    return [a, b]


def listed(tmp_path, case, stage=()):
    """-> (file, Wfst, rows): the cascade composed (and put through `stage`), listed, and the listing in a file"""
    rc, text, err = run(["-q", "-HJZ"] + list(stage) + members(tmp_path, case))
    assert rc == 0, err
    name = str(tmp_path / ("%s%s.listing" % (case, "".join(stage))))
    for _ in range(4):  # the reader numbers the states as they appear, so a listing read back may come out in another order: once
        with open(name, "w") as f:
            f.write(text)
        rc, again, err = run(["-q", "-HJZ", name])
        assert rc == 0, err
        if again == text:
            break
        text = again
    assert again == text  # reading this listing back changes nothing: the file's order is the front end's arc-id order
    w, rows = parse(text)
    return name, w, rows


def sums(args):
    """-> (N, ln W) the front end prints"""
    rc, out, err = run(["-q"] + args)
    assert rc == 0, err
    m = re.fullmatch(r"Number of paths in result: (\d+)\nSum of all paths in result: (\S+)\n", out)
    assert m, out
    text = m.group(2)
    return int(m.group(1)), float(text[2:]) if text.startswith("e^") else (math.log(float(text)) if float(text) > 0 else -np.inf)


def rounding(w, ref):
    """what reading a listing of 15 digits moves the sum by"""
    return (ref.levels[0] - 1) * PRINT * float(np.abs(w.logw).max())


@pytest.mark.parametrize("case", list(CASCADES))
def test_front_end_prints_the_count_and_the_sum(tmp_path, case):
    file, w, rows = listed(tmp_path, case)
    ref = MachineSums(w)
    assert not ref.refused and ref.N > 1
    for style in (["-Z"], [], ["-D"]):
        n, lw = sums(style + ["--machine-sums", file])
        assert n == ref.N
        assert abs(LD(lw) - ref.Z) <= ref.E[w.final] + PRINT * (1 + abs(float(ref.Z))), (case, style, lw, float(ref.Z))
    n, lw = sums(["-Z", "--machine-sums"] + members(tmp_path, case))  # the cascade itself: its weights have more digits than the listing
    assert n == ref.N and abs(LD(lw) - ref.Z) <= ref.E[w.final] + PRINT * (1 + abs(float(ref.Z))) + rounding(w, ref)
    # -F names where the lines go; with -c they follow -c's own two lines
    target = str(tmp_path / "sums.txt")
    rc, plain, err = run(["-q", "-Z", "--machine-sums", file])
    rc2, out, err = run(["-q", "-Z", "--machine-sums", "-F", target, file])
    assert rc == 0 and rc2 == 0 and out == "" and open(target).read() == plain, err
    rc, report, err = run(["-q", "-c", file])
    rc2, out, err = run(["-q", "-Z", "-c", "--machine-sums", file])
    assert rc == 0 and rc2 == 0 and out == report + plain and report.count("\n") == 2, (out, err)
    rc, out, err = run(["-Z", "--machine-sums", file], env={"CARMEL_TIMING": "1"})
    assert rc == 0 and "timing: machine sums " in err and " forward levels, " in err and "%d useful states" % ref.n_useful in err, err


@pytest.mark.parametrize("case", list(CASCADES))
@pytest.mark.parametrize("stage", [("-C",), ("--prune-paths=2",), ("-C", "--prune-paths=1.5")])
def test_the_sums_are_taken_after_consolidation_and_pruning(tmp_path, case, stage):
    plain_file, plain_w, _ = listed(tmp_path, case)
    plain = MachineSums(plain_w)
    _, w, rows = listed(tmp_path, case, stage)  # the front end's own listing of the machine after the stage
    ref = MachineSums(w)
    assert not ref.refused and 0 < ref.N < plain.N, (case, stage, ref.N, plain.N)  # the stage took paths away
    n, lw = sums(["-Z"] + list(stage) + ["--machine-sums", plain_file])
    assert n == ref.N
    assert abs(LD(lw) - ref.Z) <= ref.E[w.final] + PRINT * (1 + abs(float(ref.Z))) + rounding(w, ref), (case, stage, lw, float(ref.Z))
    if stage == ("-C",):  # merging duplicate arcs adds their weights: the sum over all paths stays, to the listings' rounding
        assert abs(LD(lw) - plain.Z) <= 1e-12


@pytest.mark.parametrize("case", list(CASCADES))
def test_machine_counts_writes_every_arcs_expected_count(tmp_path, case):
    file, w, rows = listed(tmp_path, case)
    ref = MachineSums(w)
    target = str(tmp_path / "counts.fst")
    n, lw = sums(["-HJZ", "--machine-counts=" + target, file])
    assert n == ref.N and abs(LD(lw) - ref.Z) <= ref.E[w.final] + PRINT * (1 + abs(float(ref.Z)))
    text = open(target).read()
    counted, crows = parse(text)  # it parses as a transducer: the same machine, arc for arc
    assert [r[:4] for r in crows] == [r[:4] for r in rows] and text.split("\n")[0] == open(file).read().split("\n")[0]
    for k in range(w.n_arcs):
        assert ref.arc_useful[k]
        got, want = LD(counted.logw[k]), ref.ln_gamma[k]
        bound = ref.Eg[k] + PRINT * (1 + abs(float(want)))
        assert abs(got - want) <= bound, (case, k, float(got), float(want))
        assert abs(np.exp(got) - np.exp(want)) <= np.exp(want) * bound * (1 + bound) + LD(1e-300)  # exp(ln gamma), within the same bound
    first = sum(math.exp(counted.logw[k]) for k in range(w.n_arcs) if w.src[k] == 0)
    assert abs(first - 1.0) <= 1e-12  # a path leaves the start state once
    rc, again, err = run(["-q", "-HJZ", target])  # and the front end reads it back (it numbers the states as they appear)
    assert rc == 0 and sorted(again.split("\n")) == sorted(text.split("\n")), err


def test_a_cyclic_machine_is_refused_with_the_librarys_message(golden_dir, tmp_path):
    target = tmp_path / "counts.fst"
    for args in (["--machine-sums"], ["--machine-counts=%s" % target]):
        rc, out, err = run(["-q"] + args + [os.path.join(golden_dir, "train.a.w")])
        assert signed(rc) == -11 and out == "", (rc, out, err)
        assert "carmel_hip_decoder_machine_sums" in err and "state 0 lies on or behind a cycle" in err, err
        assert not target.exists()
