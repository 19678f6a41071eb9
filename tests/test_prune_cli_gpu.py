"""GPU: the front end's --prune-paths=W / --prune-states=N / --prune-arcs=W (carmel -w / -z / -p) on the tutorial machines under
tests/golden/: the composed machine is listed once (-HJZ: an arc a line, weights as e^x, which both sides read back exactly), and
the front end's output on that listing is compared with the text built here from Decoder.prune's masks on the same flattened
machine -- the states in the front end's order, the arcs in the listing's --, reduced once more as the front end does.  This is
also the test of Transducer::keep: its renumbering, its state names and its cleared machine show in the -J, -HJ and -c forms.
A ratio large enough to keep everything gives the plain listing byte for byte."""
import math
import os
import re

import numpy as np
import pytest

from test_decode_gpu import run

pytestmark = pytest.mark.gpu

SYM = r'(\*e\*|"[^"]*"|\S+)'
ARC_LINE = re.compile(r"^\((\S+) \((\S+) %s %s e\^(\S+?)\)\)$" % (SYM, SYM))
CASES = {"train.a.w": ["train.a.w"], "cat_spellout": ["cat.fsa.trained.noe", "spellout.fst.trained"], "epron_jpron": ["epron-jpron.fst"]}


class Listing(object):
    """the composed machine as the front end lists it and reads it back"""

    def __init__(self, golden_dir, case, tmp_path):
        from carmel_amd.model import Wfst
        members = [os.path.join(golden_dir, m) for m in CASES[case]]
        rc, text, err = run(["-q", "-HJZ"] + members)
        assert rc == 0, err
        self.file = str(tmp_path / "composed.fst")
        for _ in range(4):  # the reader numbers the states as they appear, so a listing read back may come out in another order: once
            with open(self.file, "w") as f:
                f.write(text)
            rc, again, err = run(["-q", "-HJZ", self.file])
            assert rc == 0, err
            if again == text:
                break
            text = again
        assert again == text  # reading this listing back changes nothing: the file's order is the front end's arc-id order
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
        one = np.ones(len(rows), np.uint32)
        self.w = Wfst(len(ids), ids[self.final_name], self.src, self.dst, one, one, [float(r[4]) for r in rows])

    def useful(self, state_keep, arc_keep):
        """-> (states, arcs) that stay after the masks and one more reduction: on a path from state 0 to the final state"""
        n, final = self.w.n_states, self.w.final
        arcs = [k for k in range(len(self.src)) if arc_keep[k] and state_keep[self.src[k]] and state_keep[self.dst[k]]]
        if not state_keep[0] or not state_keep[final]:
            return [], []

        def reach(start, a, b):
            seen, todo = {start}, [start]
            while todo:
                q = todo.pop()
                for k in arcs:
                    if a[k] == q and b[k] not in seen:
                        seen.add(b[k])
                        todo.append(b[k])
            return seen

        ok = reach(0, self.src, self.dst) & reach(final, self.dst, self.src)
        if 0 not in ok or final not in ok:
            return [], []
        return sorted(ok), [k for k in arcs if self.src[k] in ok and self.dst[k] in ok]

    def text(self, states, arcs, form):
        """what the front end prints for the machine of these states and arcs: form "HJ", "J" or "c" """
        if form == "c":
            return "Number of states in result: %d\nNumber of arcs in result: %d\n" % (len(states), len(arcs))
        if form == "HJ":
            return "".join(l + "\n" for l in [self.final_name] + [self.lines[k] for k in arcs])
        out = [self.final_name]
        for q in states:
            name = self.state_names[q]
            out.append("(" + " ".join([name] + [self.lines[k][len(name) + 2:-1] for k in arcs if self.src[k] == q]) + ")")
        return "".join(l + "\n" for l in out)


@pytest.mark.parametrize("case", list(CASES))
def test_front_end_prints_the_pruned_machine(golden_dir, tmp_path, case):
    from carmel_amd.decode import Decoder
    L = Listing(golden_dir, case, tmp_path)
    Q = L.w.n_states
    d = Decoder(L.w)
    seen = set()
    # (every point is one start of the front end, a third of a second: few points, each with another mix of options and form)
    for ratio, n_states, min_arc, form in [("1", None, None, "HJ"), ("2", None, None, "J"), ("10", max(2, Q - 1), None, "HJ"),
                                           ("1000", 2, None, "c"), ("0.5", None, "0.1", "HJ"), (None, max(2, Q // 2), "0.25", "J"),
                                           (None, 1, None, "J"), ("e^12", None, None, "J"), ("e^30", 3, None, "HJ")]:
        args, log_ratio, logw = [], np.inf, -np.inf
        if ratio is not None:
            args.append("--prune-paths=" + ratio)
            log_ratio = max(0.0, float(ratio[2:]) if ratio.startswith("e^") else math.log(float(ratio)))  # a ratio below 1 becomes 1
        if n_states is not None:
            args.append("--prune-states=%d" % n_states)
        if min_arc is not None:
            args.append("--prune-arcs=" + min_arc)
            logw = math.log(float(min_arc))
        state_keep, arc_keep = d.prune(log_ratio, n_states, logw)
        states, arcs = L.useful(state_keep, arc_keep)
        rc, out, err = run(["-" + {"HJ": "HJZ", "J": "JZ", "c": "c"}[form]] + args + [L.file], env={"CARMEL_TIMING": "1"})
        assert rc == 0, err
        assert out == L.text(states, arcs, form), (case, args, form, err)
        assert "timing: prune " in err and " F rounds, " in err and " R rounds)" in err, err
        changed = (len(states), len(arcs)) != (Q, len(L.lines))
        assert ("prune-> %d/%d" % (len(states), len(arcs)) in err) == changed, err
        seen.add((len(states), len(arcs)))
    rc, quiet_out, err = run(["-q", "-HJZ"] + args + [L.file])  # (the last point once more, quietly)
    assert rc == 0 and quiet_out == out and "prune->" not in err, err
    d.close()
    assert len(seen) >= 3, seen  # the points really prune to different machines
    assert (0, 0) in seen if Q > 1 and L.w.final != 0 else True  # --prune-states=1 loses an endpoint: the machine is cleared


@pytest.mark.parametrize("case", list(CASES))
def test_a_ratio_that_keeps_everything_gives_the_plain_output(golden_dir, tmp_path, case):
    members = [os.path.join(golden_dir, m) for m in CASES[case]]
    for flags, prune in (([], ["--prune-paths=1e300"]), (["-H"], ["--prune-states=1000000"]), (["-c"], ["--prune-arcs=0"]),
                         (["-J"], ["--prune-paths=1e300", "--prune-states=1000000", "--prune-arcs=0"])):
        rc, plain, err = run(["-q"] + flags + members)
        assert rc == 0, err
        rc, out, err = run(["-q"] + flags + prune + members)
        assert rc == 0 and out == plain, (case, flags, prune, err)
    # -F names the file the pruned machine goes to
    target = str(tmp_path / "out.fst")
    rc, plain, err = run(["-q", "-HJ"] + members)
    rc, out, err = run(["-q", "-HJ", "--prune-paths=1e300", "-F", target] + members)
    assert rc == 0 and out == "" and open(target).read() == plain, err
