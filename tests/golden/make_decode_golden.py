#!/usr/bin/env python3
"""Regenerates the batch-decoding fixtures of tests/golden/ from the reference tree (run in the build container only; the
reference does not exist on the GPU box).  Like make_golden.py it copies DATA only: the tutorial's decoding inputs and the
three `carmel -qbsriWIEk 1` runs recorded in carmel/carmel-tutorial/commands.trace (their path lines and the two summary lines),
parsed into decode_expected.json.gz.  No reference source code is copied.

tagging.data.noe and cipher.data.noe are not copied: they are `awk 'NF>0'` of the committed tagging.data / cipher.data (the
tests derive them).  cipher.fst.trained is committed by make_golden.py; tagging.fst.trained is not usable (the tutorial's copy
is the later --crp run's output), so the tagging decode is checked through this project's own EM run."""
import gzip, json, os, shutil, sys

REF = "/root/reference/carmel"
HERE = os.path.dirname(os.path.abspath(__file__))
TUT = os.path.join(REF, "carmel-tutorial")

FIXTURES = ["cat.fsa.trained.noe", "spellout.fst.trained"]
# the larger files are committed gzip-compressed (<name>.gz; tests/decode_ref.py golden_text / golden_file read them back)
GZ_FIXTURES = ["cluster.data.noe", "cipher.wfsa.noe", "tagging.fsa.trained.noe"]
# (name, command line of carmel-tutorial/commands, data file, first and last path line of the trace, 1-based)
RUNS = [
    ("cluster", "cat cluster.data.noe | carmel -qbsriWIEk 1 cat.fsa.trained.noe spellout.fst.trained", "cluster.data.noe",
     4744, 5864),
    ("tagging", "cat tagging.data.noe | carmel -qbsriWIEk 1 tagging.fsa.trained.noe tagging.fst.trained", "tagging.data.noe",
     5896, 6900),
    ("cipher", "cat cipher.data.noe | carmel -qbsriWIEk 1 cipher.wfsa.noe cipher.fst.trained", "cipher.data.noe", 6958, 6967),
]


def main():
    if not os.path.isdir(TUT):
        sys.exit("reference tree not found: %s" % TUT)
    for f in FIXTURES:
        shutil.copyfile(os.path.join(TUT, f), os.path.join(HERE, f))
    for f in GZ_FIXTURES:
        write_gz(os.path.join(HERE, f + ".gz"), open(os.path.join(TUT, f), "rb").read())
    trace = open(os.path.join(TUT, "commands.trace")).read().split("\n")
    out = {}
    for name, cmd, data, a, b in RUNS:
        paths = trace[a - 1:b]
        derivs, viterbi = trace[b], trace[b + 1]
        assert derivs.startswith("Derivations found for all ") and viterbi.startswith("Viterbi (best path) "), (name, derivs)
        n_lines = sum(1 for ln in open(os.path.join(TUT, data)))
        assert n_lines == len(paths), (name, n_lines, len(paths))
        out[name] = {"command": cmd, "data": data, "trace_lines": [a, b + 2], "paths": paths, "derivations": derivs,
                     "viterbi": viterbi}
    write_gz(os.path.join(HERE, "decode_expected.json.gz"), (json.dumps(out, indent=1) + "\n").encode())


def write_gz(path, data):
    with open(path, "wb") as f:  # (no name or time in the header: the same bytes on every run)
        with gzip.GzipFile(fileobj=f, mode="wb", compresslevel=9, mtime=0, filename="") as g:
            g.write(data)


if __name__ == "__main__":
    main()
