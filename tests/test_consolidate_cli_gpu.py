"""GPU: the front end's -C / --consolidate-max / --consolidate-unclamped on three machines written here in carmel's text format
and on one composition of two files under tests/golden/ (spellout.fst.trained with epron-jpron.fst: 370 arcs, 262 after -C).  The
machine is listed once (-HJZ: an arc a line, weights as e^x, which both sides read back exactly), and the front end's output on
that listing is compared with the text built here from consolidate()'s result on the same flattened machine -- and, for -C with
--prune-paths, from Decoder.prune's masks on the consolidated machine, reduced once more as the front end does.  This is also the
test of Transducer::consolidate: which arcs stay, in which order, with which weights shows in the -HJ, -J and -c forms.  On a
machine without duplicates -C prints the plain listing."""
import math
import os
import re

import numpy as np
import pytest

from consolidate_ref import Consolidated
from test_decode_gpu import run

pytestmark = pytest.mark.gpu

SYM = r'(\*e\*|"[^"]*"|\S+)'
ARC_LINE = re.compile(r"^\((\S+) \((\S+) %s %s e\^([^\s!)]+)(!\d*)?\)\)$" % (SYM, SYM))  # (!, !n: the arc's tie group)

# (the weights are short decimals: e^x is read back to the same double however often it is listed)
PARALLEL = """F
(S (A "a" "x" e^-0.5) (A "a" "x" e^-1.25) (A "b" "x" e^-0.75) (A "a" "x" e^-3))
(A (F "c" "y" e^-0.25) (F "c" "y" e^-2) (F "c" "y" e^-3) (A *e* "z" e^-1) (A *e* "z" e^-1.5))
"""
# sums above 1 (the clamp shows), interleaved duplicates, and a branch that only the ratio of --prune-paths=10 cuts
OVER_ONE = """END
(0 (1 "a" "a" e^-0.25) (2 "b" "b" e^-0.5) (1 "a" "a" e^-0.125) (2 "b" "b" e^-4) (1 "a" "a" e^-0.5) (3 "c" "c" e^-6))
(1 (END "d" *e* e^-0.0625) (END "d" *e* e^-0.0625))
(2 (END "d" *e* e^-1) (1 *e* "f" e^-2))
(3 (END "d" "d" e^-5) (END "d" "d" e^-5.5))
"""
PLAIN = """F
(S (A "a" "x" e^-0.5) (A "a" "y" e^-1.25) (B "a" "x" e^-0.75))
(A (F "c" "y" e^-0.25) (F "d" "y" e^-2))
(B (F "c" "y" e^-3))
"""
CASES = {"parallel": PARALLEL, "over_one": OVER_ONE, "plain": PLAIN, "spellout_epron": ["spellout.fst.trained", "epron-jpron.fst"]}
COMMANDS = [(["-C"], "HJ", ("sum", True), None), (["-C", "--consolidate-max"], "J", ("max", True), None),
            (["-C", "--consolidate-unclamped"], "c", ("sum", False), None), (["-C", "--prune-paths=10"], "HJ", ("sum", True), math.log(10.0))]
FLAGS = {"HJ": "-HJZ", "J": "-JZ", "c": "-c"}


class Listing(object):
    """the machine as the front end lists it and reads it back: the file, its lines in arc-id order, the Wfst of those lines"""

    def __init__(self, golden_dir, case, tmp_path):
        from carmel_amd.model import Wfst
        if isinstance(CASES[case], str):
            members = [str(tmp_path / "written.fst")]
            with open(members[0], "w") as f:
                f.write(CASES[case])
        else:
            members = [os.path.join(golden_dir, m) for m in CASES[case]]
        rc, text, err = run(["-q", "-HJZ"] + members)
        assert rc == 0, err
        self.file = str(tmp_path / "listed.fst")
        for _ in range(4):  # the reader numbers the states as they appear, so a listing read back may come out in another order: once
            with open(self.file, "w") as f:
                f.write(text)
            rc, again, err = run(["-q", "-HJZ", self.file])
            assert rc == 0, err
            if again == text:
                break
            text = again
        assert again == text  # reading this listing back changes nothing: the file's order is the front end's arc-id order
        self.plain = text
        self.lines = text.split("\n")[1:-1]
        self.final_name = text.split("\n")[0]
        rows = [ARC_LINE.match(l).groups() for l in self.lines]
        rc, grouped, err = run(["-q", "-JZ", self.file])  # a line per state, in the front end's state order
        assert rc == 0, err
        self.state_names = [re.match(r"^\(([^ )]+)", l).group(1) for l in grouped.split("\n")[1:-1]]
        ids = {n: i for i, n in enumerate(self.state_names)}
        assert len(ids) == len(self.state_names) and rows[0][0] == self.state_names[0]
        self.src = [ids[r[0]] for r in rows]
        self.dst = [ids[r[1]] for r in rows]
        assert self.src == sorted(self.src)  # the listing is in arc-id order: by source state
        syms = {}
        sym = lambda s: syms.setdefault(s, len(syms))
        self.w = Wfst(len(ids), ids[self.final_name], self.src, self.dst, [sym(r[2]) for r in rows], [sym(r[3]) for r in rows],
                      [float(r[4]) for r in rows])

    def line(self, k, logw):
        """line k of the listing with another weight, as the front end's -Z writes it (the arc's tie group stays)"""
        return self.lines[k][:self.lines[k].rindex(" e^")] + " e^%.15g%s))" % (logw, ARC_LINE.match(self.lines[k]).group(6) or "")

    def useful(self, arcs, src, dst):
        """-> (states, arcs) on a path from state 0 to the final state over these arcs (positions into src / dst)"""
        final = self.w.final

        def reach(start, a, b):
            seen, todo = {start}, [start]
            while todo:
                q = todo.pop()
                for k in arcs:
                    if a[k] == q and b[k] not in seen:
                        seen.add(b[k])
                        todo.append(b[k])
            return seen

        ok = reach(0, src, dst) & reach(final, dst, src)
        if 0 not in ok or final not in ok:
            return [], []
        return sorted(ok), [k for k in arcs if src[k] in ok and dst[k] in ok]

    def text(self, states, rows, form):
        """what the front end prints for these states and arcs; rows: (source state, line) in order; form "HJ", "J" or "c" """
        if form == "c":
            return "Number of states in result: %d\nNumber of arcs in result: %d\n" % (len(states), len(rows))
        if form == "HJ":
            return "".join(l + "\n" for l in [self.final_name] + [l for _, l in rows])
        out = [self.final_name]
        for q in states:
            name = self.state_names[q]
            out.append("(" + " ".join([name] + [l[len(name) + 2:-1] for s, l in rows if s == q]) + ")")
        return "".join(l + "\n" for l in out)


def removed_on_the_cpu(L, mode, clamp):
    w = L.w
    return w.n_arcs - Consolidated(w.src, w.dst, w.isym, w.osym, w.logw, mode, clamp).n_kept


@pytest.mark.parametrize("case", list(CASES))
def test_front_end_prints_the_consolidated_machine(golden_dir, tmp_path, case):
    from carmel_amd.decode import Decoder, consolidate
    L = Listing(golden_dir, case, tmp_path)
    Q, A = L.w.n_states, L.w.n_arcs
    removed = removed_on_the_cpu(L, "sum", True)  # (the reference, before any device call)
    assert (removed > 0) == (case != "plain"), (case, removed)
    for args, form, (mode, clamp), log_ratio in COMMANDS:
        c, arc_map, _ = consolidate(L.w, mode, clamp)
        assert c.n_arcs == A - removed
        kept = [int(np.flatnonzero(arc_map == j)[0]) for j in range(c.n_arcs)]  # the representatives' old ids, in the new order
        states, arcs = list(range(Q)), list(range(c.n_arcs))
        if log_ratio is not None:
            d = Decoder(c)
            state_keep, arc_keep = d.prune(log_ratio)
            d.close()
            arcs = [k for k in arcs if arc_keep[k] and state_keep[c.src[k]] and state_keep[c.dst[k]]]
            states, arcs = L.useful(arcs, c.src.tolist(), c.dst.tolist()) if state_keep[0] and state_keep[c.final] else ([], [])
        rows = [(int(c.src[k]), L.line(kept[k], c.logw[k]) if removed else L.lines[kept[k]]) for k in arcs]
        rc, out, err = run([FLAGS[form]] + args + [L.file], env={"CARMEL_TIMING": "1"})
        assert rc == 0, err
        assert out == L.text(states, rows, form), (case, args, form, err)
        assert "timing: consolidate " in err and " s (kernels " in err, err
        assert ("consolidate-> %d/%d" % (Q, c.n_arcs) in err) == (removed > 0), err
        if log_ratio is not None and case == "over_one":
            assert len(arcs) < c.n_arcs and "prune-> %d/%d" % (len(states), len(arcs)) in err, err  # the ratio cuts the far branch
    rc, quiet_out, err = run(["-q", FLAGS[form]] + args + [L.file])  # (the last command once more, quietly)
    assert rc == 0 and quiet_out == out and "consolidate->" not in err, err


def test_at_least_two_machines_lose_arcs_and_the_clamp_shows(golden_dir, tmp_path):
    """the condition of the cases, from the reference alone; and on `over_one` the three modes print three different machines"""
    from carmel_amd.decode import consolidate
    lost = {}
    for case in CASES:
        os.makedirs(str(tmp_path / case))
        L = Listing(golden_dir, case, tmp_path / case)
        lost[case] = removed_on_the_cpu(L, "sum", True)
        if case == "over_one":
            weights = {key: consolidate(L.w, *key)[0].logw.tolist() for key in (("sum", True), ("sum", False), ("max", True))}
            assert 0.0 in weights["sum", True] and max(weights["sum", False]) > 0.0
            assert len({tuple(v) for v in weights.values()}) == 3
    assert lost["plain"] == 0 and sum(1 for v in lost.values() if v > 0) >= 2, lost
    assert lost["spellout_epron"] == 370 - 262, lost


def test_a_machine_without_duplicates_gives_the_plain_output(golden_dir, tmp_path):
    L = Listing(golden_dir, "plain", tmp_path)
    for flags, extra in ((["-HJZ"], []), (["-JZ"], ["--consolidate-max"]), (["-c"], ["--consolidate-unclamped"]), (["-Z"], [])):
        rc, plain, err = run(["-q"] + flags + [L.file])
        assert rc == 0, err
        rc, out, err = run(["-q"] + flags + ["-C"] + extra + [L.file])
        assert rc == 0 and out == plain, (flags, extra, err)
    target = str(tmp_path / "out.fst")  # -F names the file the consolidated machine goes to
    rc, out, err = run(["-q", "-HJZ", "-C", "-F", target, L.file])
    assert rc == 0 and out == "" and open(target).read() == L.plain, err
