"""The count pass's bucket kernel as a walk (kernels.hip: trans_c_bucket_kernel<.., WALK>, option trans_bucket_walk: a grid of at
most a workgroup per CU, each workgroup taking the buckets of its XCD's eighth a grid apart, the next bucket's descriptor
requested while this one is worked on) against one workgroup per bucket (trans_bucket_walk = "0"): the same trainer inputs
through both, estimate(per_pair=True), maximize(1.0), estimate() again, and what comes out compared bit for bit -- the two ln p
scalars, ln p per pair, every count.  The one allowance is the project's standing one for the atomic add per piece of a split
hub arc (at most 16 counts, to 1e-13 relative); where the layout has no split arc there is none.  (The weight pass's bucket
kernel asks for its runs with its first batch of loads in either form; it does not walk -- profiles/
measurement_log_bucket_walk.md -- and is covered here by the same comparisons.)

A small workgroup cap is what makes a small corpus walk many buckets: trans_bucket_walk = "8" gives every workgroup an eighth of
them.

The last test needs no GPU: it compiles kernels.hip for gfx950 with the Makefile's flags and checks that no instantiation of the
two bucket kernels uses scratch memory and that each leaves room for one 1024-thread workgroup per CU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import host_lattices

from carmel_amd import synth
from carmel_amd.model import NORM_CONDITIONAL

TRANS_SPLIT, TRANS_SINGLE = 1, 2
RTOL = 1e-7  # against the oracle (test_gpu_parity.py)


def _fb(*a, **k):
    from carmel_amd.trainer import HipForwardBackward
    return HipForwardBackward(*a, **k)


def run(w, c):
    fb = _fb(w, c)
    lp, _ = fb.estimate(per_pair=True)
    out = [lp, fb.pair_logprob.copy(), fb.counts().copy()]
    fb.maximize(1.0)
    lp2, _ = fb.estimate()
    out += [lp2, fb.counts().copy()]
    fb.close()
    return out


_parent = {}


def parent(hipopt, key, w, c, **opts):
    """one workgroup per bucket: computed once per (corpus, options), shared, left unchanged"""
    k = (key,) + tuple(sorted(opts.items()))
    if k not in _parent:
        hipopt.set("trans_bucket_walk", "0")
        _parent[k] = run(w, c)
        for x in _parent[k]:
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return _parent[k]


def layout_flags(w, c):
    tr = host_lattices(w, c)["transpose"]
    return tr["buckets"]["flags"], len(tr["split_arcs"])


def same(a, b, n_split, what, hub=False):
    assert a[0] == b[0], what
    assert np.array_equal(a[1], b[1]), what
    first_equal = np.array_equal(a[2], b[2])
    rounds = ((a[2], b[2]),) if hub and not first_equal else ((a[2], b[2]), (a[4], b[4]))
    for x, y in rounds:
        if n_split == 0:
            assert np.array_equal(x, y), (what, int((x != y).sum()))
        else:  # (the one atomic add per piece of a split hub arc aside)
            assert (x != y).sum() <= 16 and np.allclose(x, y, rtol=1e-13, atol=0), (what, int((x != y).sum()))
    if not hub or first_equal:
        assert a[3] == b[3], what
    else:
        # hub machines (test_hub_arcs): four or six arcs, one of them in pieces whose sums meet in atomic adds in whatever
        # order they arrive.  When that count came out in other last bits than the parent's (the allowance above), the M-step
        # normalises other numbers and NOTHING the second estimate computes can be expected bit for bit: measured with one
        # workgroup per bucket against ITSELF, seed 1, 1 run of 8 had the count differ and with it the second ln p
        # (-4724.678350009059 against -4724.67835000906) and one of the four second counts.  Then: counts to 1e-13 relative
        # are weights to 2e-13, ln w to 2e-13 absolute, ln p of a pair of at most 60 arcs to 1.2e-11 absolute against
        # |ln p| >= 20 ln 2 = 13.9, below 1e-12 relative, and so their sum; a posterior is exp of a difference of such sums
        # (2.4e-11 relative), a count a sum of posteriors.
        assert abs(a[3] - b[3]) <= 1e-12 * abs(b[3]), (what, a[3], b[3])
        np.testing.assert_allclose(a[4], b[4], rtol=1e-10, atol=0, err_msg=str(what))
    assert not np.any(np.isnan(a[2])) and not np.any(np.isnan(a[4])), what


_c4 = {}


def c4_small():
    if not _c4:
        w, c = synth.make_config("c4", n_pairs=120000)
        _c4["wc"] = (w, c)
        _c4["split"] = layout_flags(w, c)[1]
    return _c4["wc"] + (_c4["split"],)


@pytest.mark.gpu
@pytest.mark.parametrize("walk", [None, "1000", "8", "24"])
def test_small_c4_walks_its_buckets(hipopt, walk):
    """bench.py's c4 shape at 120 000 pairs, about 165 buckets.  Unset: fewer buckets than the device has CUs, the launch helper
    keeps one workgroup per bucket; "1000": the walking kernel at one bucket per workgroup (the request ahead has no
    successor); "8": every workgroup walks an eighth of the buckets; "24": uneven shares, some workgroups a bucket short"""
    w, c, n_split = c4_small()
    old = parent(hipopt, "c4", w, c)
    if walk is None:
        hipopt.unset("trans_bucket_walk")
    else:
        hipopt.set("trans_bucket_walk", walk)
    same(run(w, c), old, n_split, walk)


@pytest.mark.gpu
@pytest.mark.parametrize("runs", ["0", "1"])
@pytest.mark.parametrize("scatter", ["0", "1", "2", "3"])
def test_the_other_instantiations_walk_too(hipopt, runs, scatter):
    """per-item and run-length indices, gathering and scattering first passes: every form of the two kernels, eight workgroups"""
    w, c, n_split = c4_small()
    hipopt.set("trans_runs", runs)
    hipopt.set("trans_scatter", scatter)
    old = parent(hipopt, "c4", w, c, runs=runs, scatter=scatter)
    hipopt.set("trans_bucket_walk", "8")
    same(run(w, c), old, n_split, (runs, scatter))


@pytest.mark.gpu
@pytest.mark.parametrize("walk", [None, "8"])
def test_one_bucket(hipopt, walk):
    """a single bucket: seven of the eight workgroups have nothing and leave before any barrier"""
    w, c = synth.make_config("toy")
    flags, n_split = layout_flags(w, c)
    assert len(flags) == 1 and n_split == 0
    old = parent(hipopt, "toy", w, c)
    if walk is None:
        hipopt.unset("trans_bucket_walk")
    else:
        hipopt.set("trans_bucket_walk", walk)
    same(run(w, c), old, 0, walk)


def hub_corpus(seed, n_pairs=None):
    """the shapes of test_estep_random_shapes seeds 0 and 1 (test_gpu_parity.py): hub arcs with more items than a bucket holds"""
    rng = np.random.default_rng(100 + seed)
    if seed == 0:
        kw = dict(n_states=2, deg=2, n_sym=2, p_eps=0.0, n_pairs=1500, lo=40, hi=60)
    else:
        kw = dict(n_states=3, deg=2, n_sym=2, p_eps=0.0, n_pairs=int(rng.integers(900, 1500)), lo=20, hi=40)
    if n_pairs:
        kw["n_pairs"] = n_pairs
    w = synth.random_wfst(kw["n_states"], kw["deg"], n_sym=kw["n_sym"], p_eps=kw["p_eps"], seed=200 + seed)
    c = synth.random_walk_corpus(w, kw["n_pairs"], min_arcs=kw["lo"], max_arcs=kw["hi"], seed=200 + seed, out_degree=kw["deg"])
    c.weight[:] = rng.uniform(0.25, 2.0, c.n_pairs)
    return w, c


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n_pairs", [(0, None), (1, None), (0, 6000), (1, 6000)])
def test_hub_arcs(oracle, hipopt, seed, n_pairs):
    """buckets that are one arc (TRANS_SINGLE) or a piece of one (TRANS_SPLIT) among a workgroup's buckets: the branch with a
    barrier of its own that used to end the kernel.  The 6000-pair corpora are the same machines with four times the items,
    so that at eight workgroups every one of them walks several such buckets in a row; those of the parity test's own size
    are compared with the oracle as that test does.  The second estimate is compared bit for bit whenever the first one's
    counts are bit for bit the parent's; where the split arc's atomic adds came in another order it stands on other
    weights (see same())."""
    w, c = hub_corpus(seed, n_pairs)
    flags, n_split = layout_flags(w, c)
    assert np.any(flags & TRANS_SINGLE) and np.any(flags & TRANS_SPLIT) and n_split > 0
    if n_pairs:
        assert len(flags) >= 24  # three buckets a workgroup at least
    old = parent(hipopt, ("hub", seed, n_pairs), w, c)
    hipopt.set("trans_bucket_walk", "8")
    new = run(w, c)
    same(new, old, n_split, (seed, n_pairs), hub=True)
    if not n_pairs:
        ow, oc = oracle.OracleWfst.from_arrays(w), oracle.OracleCorpus.from_arrays(c)
        ow.normalize(NORM_CONDITIONAL, 0.0)
        r = oracle.estimate(ow, oc)
        ok = r["has_deriv"]
        np.testing.assert_allclose(new[1][ok], r["pair_logprob"][ok], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(new[2], np.exp(r["counts_ln"]), rtol=RTOL, atol=1e-13)


# ---------------- no GPU: what the compiler made of the two kernels ----------------
def makefile_flags():
    txt = open(os.path.join(ROOT, "carmel_amd", "csrc", "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*=\s*(.*)$" % name, txt, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    rule = re.search(r"^kernels\.o:.*\n\t(.*)$", txt, flags=re.M).group(1)
    flags = []
    for name in ("CXXFLAGS", "HIPFLAGS"):
        if "$(%s)" % name in rule:
            flags += var(name)
    assert "--offload-arch=gfx950" in flags
    return flags


def test_the_bucket_kernels_use_no_scratch_and_fit_a_workgroup_per_cu():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "carmel_amd", "csrc", "kernels.hip")
    r = subprocess.run([hipcc] + makefile_flags() + ["--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    found = 0
    for m in re.finditer(r"^(_Z\w*trans_[wc]_bucket_kernel\w*):.*?\n\ts_endpgm(.*?)(?=^_Z\w+:|\Z)", r.stdout, flags=re.S | re.M):
        name, tail = m.group(1), m.group(2)
        scratch, occ = re.search(r"; ScratchSize: (\d+)", tail), re.search(r"; Occupancy: (\d+)", tail)
        assert scratch and occ, name
        assert int(scratch.group(1)) == 0, (name, scratch.group(0))
        assert int(occ.group(1)) >= 4, (name, occ.group(0))  # waves per SIMD: 4 = one 1024-thread workgroup resident
        found += 1
    assert found == 15, found  # three index forms each: the weight pass at full and half size, the count pass and its walk too
