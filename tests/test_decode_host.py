"""CPU: batch 1-best decoding's front-end switches (carmel -qbsriWIEk 1), the decoding fixtures, and the decode kernel's
resources.  Nothing here needs a GPU."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from decode_ref import decode_expected, golden_text
from test_kernel_resources import device_asm, kernels

CLI = os.path.join(ROOT, "carmel_amd", "bin", "carmel")


def run(args, stdin=""):
    p = subprocess.run([CLI] + list(args), input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    return p.returncode, p.stdout, p.stderr


def signed(rc):
    return rc - 256 if rc > 127 else rc


def test_tutorial_decode_is_no_longer_refused(golden_dir):
    """the tutorial's decode command gets past the switches: on a machine without a GPU it fails where the device is needed
    (-11, "no HIP device"), not with -12 for an unimplemented switch"""
    from carmel_amd._capi import lib
    g = lambda n: os.path.join(golden_dir, n)
    rc, out, err = run(["-qbsriWIEk", "1", g("cat.fsa.trained.noe"), g("spellout.fst.trained")], stdin="c1 c2\n")
    if lib.carmel_hip_device_count() > 0:
        assert rc == 0, err
        return
    assert signed(rc) == -11, err
    assert "not implemented" not in err and "no HIP device" in err and "carmel_hip_decoder_create" in err


@pytest.mark.parametrize("args,needle", [
    (["-qbsriWIEk", "2"], "-k n with n > 1"),
    (["-qbsrk", "1"], "arc path form"),
    (["-qsrWIEk", "1"], "-k without -b or -i"),
    (["-qbsriWIEk", "1", "-P"], "switch -P"),
    (["-qbsriWIEk", "1", "--sum"], "--sum"),
    (["-qbsriWIEk", "1", "--post-b"], "--post-b"),
    (["-qbsriWIE"], "without -k 1"),
])
def test_unimplemented_decoding_forms_are_refused(golden_dir, args, needle):
    g = lambda n: os.path.join(golden_dir, n)
    rc, out, err = run(args + [g("cat.fsa.trained.noe"), g("spellout.fst.trained")], stdin="c1 c2\n")
    assert signed(rc) == -12, err
    assert needle in err and "HIP" not in err
    assert out == ""


def test_help_lists_the_decoding_switches():
    rc, out, err = run(["-h"])
    assert rc == 0 and "-b -i -s -r -k 1" in out


def noe(golden_dir, name):
    """tagging.data.noe / cipher.data.noe are `awk 'NF>0'` of the committed corpora"""
    if name in ("tagging.data.noe", "cipher.data.noe"):
        return [l for l in open(os.path.join(golden_dir, name[:-4])).read().split("\n") if l.split()]
    return golden_text(golden_dir, name).split("\n")[:-1]


def test_decode_fixtures(golden_dir):
    gold = decode_expected(golden_dir)
    assert {k: len(v["paths"]) for k, v in gold.items()} == {"cluster": 1121, "tagging": 1005, "cipher": 10}
    for name, v in gold.items():
        lines = noe(golden_dir, v["data"])
        assert len(lines) == len(v["paths"])
        n_sym = sum(len(l.split()) for l in lines)
        assert v["derivations"] == "Derivations found for all %d inputs." % len(lines)
        m = re.match(r"Viterbi \(best path\) product of probs=e\^(\S+), probability=2\^(\S+) "
                     r"per-input-symbol-perplexity\(N=(\d+)\)=2\^(\S+) per-line-perplexity\(N=(\d+)\)=2\^(\S+)$", v["viterbi"])
        assert m, v["viterbi"]
        ln_p = float(m.group(1))
        assert int(m.group(3)) == n_sym and int(m.group(5)) == len(lines)
        assert float(m.group(2)) == float("%.6g" % (ln_p / 0.6931471805599453))
        assert float(m.group(4)) == float("%.6g" % (-ln_p / n_sym / 0.6931471805599453))


def test_decode_kernels_use_no_scratch_memory():
    """the 1-best trellis kernel in its two tiers (decode.hip), and the walk kernel that it shares with the k-best decoder in its
    two passes (decode_paths.hip)"""
    ks = kernels(device_asm("decode.hip"))
    assert len(ks) == 2 and all("decode_trellis_kernel" in k for k in ks), list(ks)
    walks = kernels(device_asm("decode_paths.hip"))
    assert len(walks) == 2 and all("decode_walk_kernel" in k for k in walks), list(walks)
    ks.update(walks)
    assert len(ks) == 4, list(ks)
    for name, (body, tail) in ks.items():
        m = re.search(r"; ScratchSize: (\d+)", tail)
        assert m and int(m.group(1)) == 0, (name, m and m.group(0))
        assert "scratch_" not in body, name
