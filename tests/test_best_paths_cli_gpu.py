"""GPU: the front end's --best-paths=N (carmel -k N without -b / -i) on tests/golden/train.a.w, on a two-machine cascade and on a
machine with fewer than N paths: the arc form and the -I, -OQWE and -@ forms against lines formatted here from Decoder.best_paths
on the same composed machine (the front end's own -HJ listing of it, read back by the oracle), fill lines included."""
import math
import os
import re

import numpy as np
import pytest

from test_decode_gpu import run
from test_decode_kbest_gpu import printed_ln

pytestmark = pytest.mark.gpu

SYM = r'(\*e\*|"[^"]*"|\S+)'
ARC_LINE = re.compile(r"^\((\S+) \((\S+) %s %s (\S+?)!?\)\)$" % (SYM, SYM))
ARC_FORM = re.compile(r"\((\S+) -> (\S+) %s : %s / (\S+)\)" % (SYM, SYM))
A_FST = 'F\n(S (A a x 0.5) (A b y 0.5))\n(A (A c z 0.25) (F d *e* 0.25) (F *e* w 0.5))\n'
B_FST = 'E\n(E (E x "p q" 0.5) (E y r 0.25) (E z *e* 0.5) (E w s 0.125) (E *e* t 0.125))\n'
C_FST = 'F\n(S (F a "x" 0.5) (F b y 0.25))\n'  # two paths: --best-paths=4 prints two fill lines


def same_weight(tok, ln):
    return abs(printed_ln(tok) - ln) <= 1e-4 * max(1.0, abs(ln))


def composed(oracle, members, tmp_path):
    """-> (the file of the composed machine, its Wfst, per arc (source name, destination name, input name, output name))"""
    from carmel_amd.model import Wfst
    rc, text, err = run(["-q", "-HJ"] + members)
    assert rc == 0, err
    path = tmp_path / "composed.fst"
    path.write_text(text)
    w = oracle.OracleWfst.parse(text).arrays()
    rows = [ARC_LINE.match(l).groups() for l in text.split("\n")[1:] if l.count("(") == 2]
    assert len(rows) == len(w["src"])
    # The oracle numbers the states its own way and keeps a state's arcs in the listing's order: state 0 is the listing's first
    # source, and the k-th arc of a named state is the k-th line of that name, which names the arc's destination.
    by_name = {}
    for r in rows:
        by_name.setdefault(r[0], []).append(r)
    by_id = {}
    for k in range(len(rows)):
        by_id.setdefault(int(w["src"][k]), []).append(k)
    state, isym, osym, names, todo = {0: rows[0][0]}, {}, {}, [None] * len(rows), [0]
    while todo:
        q = todo.pop()
        mine = by_name.get(state[q], [])
        assert len(mine) == len(by_id.get(q, []))
        for k, (s, t, i, o, x) in zip(by_id.get(q, []), mine):
            if int(w["dst"][k]) not in state:
                todo.append(int(w["dst"][k]))
            for table, key, name in ((state, w["dst"][k], t), (isym, w["isym"][k], i), (osym, w["osym"][k], o)):
                assert table.setdefault(int(key), name) == name
            assert same_weight(x, w["logw"][k])
            names[k] = (s, t, i, o)
    assert len(set(state.values())) == len(state) and None not in names  # (every state of the listing can be reached)
    return str(path), Wfst(w["n_states"], w["final"], w["src"], w["dst"], w["isym"], w["osym"], w["logw"]), names


def unquote(x):
    return x[1:-1] if len(x) >= 2 and x[0] == '"' and x[-1] == '"' else x


def check_forms(file, w, names, paths, n):
    """the four forms of --best-paths=n on `file` against `paths` (Decoder.best_paths) -> the -OQWE output"""
    fill = n - len(paths)
    value = lambda p: sum(float(w.logw[a]) for a in p)
    # the arc form: (src -> dst in : out / w) per arc, then the path's weight
    rc, out, err = run(["-q", "--best-paths=%d" % n, file], env={"CARMEL_TIMING": "1"})
    assert rc == 0 and "timing: best paths " in err and " rounds, " in err, err
    lines = out.split("\n")
    assert len(lines) == n + 1 and lines[-1] == "" and lines[len(paths):n] == ["0"] * fill, out
    for line, (_, p) in zip(lines, paths):
        arcs = ARC_FORM.findall(line)
        assert [a[:4] for a in arcs] == [names[k] for k in p], line
        assert all(same_weight(a[4], float(w.logw[k])) for a, k in zip(arcs, p)), line
        assert ARC_FORM.sub("", line).split() == [line.split(" ")[-1]] and same_weight(line.split(" ")[-1], value(p)), line
    # -I: the input symbols, epsilons kept, then the weight
    rc, out, err = run(["-qI", "--best-paths=%d" % n, file])
    assert rc == 0, err
    lines = out.split("\n")
    assert len(lines) == n + 1 and lines[len(paths):n] == ["0"] * fill, out
    for line, (_, p) in zip(lines, paths):
        toks = re.findall(SYM, line)
        assert toks[:-1] == [names[k][2] for k in p] and same_weight(toks[-1], value(p)), line
    # -OQWE: the output symbols without quotes and epsilons, no weight; empty fill lines
    rc, out_o, err = run(["-qOQWE", "--best-paths=%d" % n, file])
    assert rc == 0, err
    want = [" ".join(unquote(names[k][3]) for k in p if names[k][3] != "*e*") for _, p in paths] + [""] * fill
    assert out_o == "".join(l + "\n" for l in want), out_o
    # -@: the pair the path spells, two lines; one empty fill line each
    rc, out, err = run(["-q@", "--best-paths=%d" % n, file])
    assert rc == 0, err
    want = []
    for _, p in paths:
        want += [" ".join(names[k][2] for k in p if names[k][2] != "*e*"), " ".join(names[k][3] for k in p if names[k][3] != "*e*")]
    assert out == "".join(l + "\n" for l in want + [""] * fill), out
    return out_o


@pytest.mark.parametrize("case", ["train.a.w", "cascade", "two_paths"])
def test_front_end_lists_the_best_paths(oracle, golden_dir, tmp_path, case):
    from carmel_amd.decode import Decoder
    if case == "train.a.w":
        members = [os.path.join(golden_dir, "train.a.w")]
    else:
        texts = {"cascade": [A_FST, B_FST], "two_paths": [C_FST]}[case]
        members = []
        for i, t in enumerate(texts):
            (tmp_path / ("m%d.fst" % i)).write_text(t)
            members.append(str(tmp_path / ("m%d.fst" % i)))
    file, w, names = composed(oracle, members, tmp_path)
    d = Decoder(w)
    paths = d.best_paths(4)
    d.close()
    assert len(paths) == (2 if case == "two_paths" else 4)
    out_o = check_forms(file, w, names, paths, 4)
    # the cascade itself (composed by the front end, also on the device) lists what its listing lists: the weights are dyadic
    for extra in ([], ["--gpu-compose"]):
        rc, out, err = run(["-qOQWE", "--best-paths=4"] + extra + members)
        assert rc == 0 and out == out_o, (err, out, out_o)
    # --best-paths=1 names the first line's string; -k 1 and -k N are accepted beside it
    rc, out1, err = run(["-qOQWE", "--best-paths=1", "-k", "1"] + members)
    assert rc == 0 and out1 == out_o.split("\n")[0] + "\n", (err, out1)
    rc, out4, err = run(["-qOQWE", "--best-paths=4", "-k", "4"] + members)
    assert rc == 0 and out4 == out_o, err
