"""The batched one-pass window M-step (mstep_wide.hip: mstep_wide_kernel, ONE launch that also delivers the step's largest
change) against the two launches it replaces (mstep_window_kernel + mstep_max_final_kernel, option mstep_wide = "0"): the
same inputs through both, and everything that comes out compared bit for bit -- the weights after the initial normalisation,
after estimate + maximize, the returned largest change, and the same again for a second iteration (which stands on the
slots and ticket counters that the first one's last workgroup put back to zero).

The last test needs no GPU: it compiles the file for gfx950 with the Makefile's flags and checks that no instantiation of the
kernel uses scratch memory and that each keeps at least four workgroups per CU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import hip_env

from carmel_amd import synth
from carmel_amd.model import NORM_CONDITIONAL, NORM_JOINT, NORM_NONE, Corpus, Wfst

OLD = {"CARMEL_HIP_MSTEP_WIDE": "0"}


def _fb(*a, **k):
    from carmel_amd.trainer import HipForwardBackward
    return HipForwardBackward(*a, **k)


def locked(w, every=7, value=0.05):
    """lock every 7th arc: locked arcs keep their weight and reserve mass (fst.cc:196-230)"""
    grp, logw = w.group.copy(), w.logw.copy()
    grp[::every] = 0
    logw[::every] = np.log(value)
    return Wfst(w.n_states, w.final, w.src, w.dst, w.isym, w.osym, logw, grp)


def sized_model(n_arcs, deg, seed):
    """a model with exactly n_arcs parameters: states of `deg` arcs each, as many as fit (random_wfst), then states that nothing
    leads to holding the remainder (they get no counts: their arcs end at weight zero, the `ok == false` branch)"""
    nb = max(1, n_arcs // deg)
    if nb * deg > n_arcs:  # fewer arcs than one state's worth
        deg, nb = n_arcs, 1
    w = synth.random_wfst(nb + 1, deg, n_sym=4, p_eps=0.1, seed=seed)
    rest = n_arcs - nb * deg
    if rest:
        rng = np.random.default_rng(seed + 77)
        src = np.concatenate([w.src, np.full(rest, nb + 1, dtype=np.uint32)])
        dst = np.concatenate([w.dst, np.full(rest, nb, dtype=np.uint32)])
        isym = np.concatenate([w.isym, rng.integers(2, 5, size=rest, dtype=np.uint32)])
        osym = np.concatenate([w.osym, rng.integers(2, 5, size=rest, dtype=np.uint32)])
        logw = np.concatenate([w.logw, np.log(rng.uniform(0.1, 1.0, rest))])
        w = Wfst(nb + 2, nb, src, dst, isym, osym, logw)
    assert w.n_arcs == n_arcs
    if deg > 1:
        c = synth.random_walk_corpus(w, 64, min_arcs=2, max_arcs=9, seed=seed, out_degree=deg)
    else:  # one arc per state: the only path is arc 0
        c = Corpus.from_lists([([int(s) for s in w.isym[:1] if s], [int(s) for s in w.osym[:1] if s])] * 3)
    return w, c


def rounds(make, env, delta=1.0, iters=2):
    """weights after the initial normalisation, then per iteration: the counts, the weights after maximize, the largest change"""
    with hip_env(env):
        fb = make()
        out = [("normalised", fb.weights())]
        for i in range(iters):
            fb.estimate()
            out.append(("counts %d" % i, fb.counts()))
            d = fb.maximize(delta)
            out.append(("weights %d" % i, fb.weights()))
            out.append(("change %d" % i, d))
        fb.close()
    return out


def same(make, env=None, **kw):
    env = dict(env or {})
    new, old = rounds(make, env, **kw), rounds(make, dict(env, **OLD), **kw)
    assert len(new) == len(old)
    for (name, a), (_, b) in zip(new, old):
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, b), (name, int(np.sum(a != b)), a.size)  # (-inf equals -inf; there is no NaN)
            assert not np.any(np.isnan(a)), name
        else:
            assert a == b, (name, a, b)
    return new


@pytest.mark.gpu
@pytest.mark.parametrize("deg,group,lock,add_count", [
    (3, NORM_CONDITIONAL, False, 0.0), (3, NORM_JOINT, True, 0.25),    # span <= 15: mask32
    (20, NORM_CONDITIONAL, True, 0.0), (20, NORM_JOINT, False, 0.25),  # 16 .. 31: mask64
    (50, NORM_CONDITIONAL, True, 0.25), (50, NORM_JOINT, False, 0.0),  # 32 .. 64: the scan
    (50, NORM_JOINT, True, 0.0),
])
def test_the_three_ways_of_finding_a_group(deg, group, lock, add_count):
    w = synth.random_wfst(301, deg, n_sym=5, p_eps=0.15, seed=deg)
    c = synth.random_walk_corpus(w, 150, min_arcs=3, max_arcs=12, seed=deg, out_degree=deg)
    if lock:
        w = locked(w)
    out = same(lambda: _fb(w, c, norm_group=group, add_count=add_count))
    assert 0.0 < out[-1][1] <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("group", [NORM_CONDITIONAL, NORM_JOINT])
@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("as_prior", [False, True])
def test_with_a_prior(group, lock, as_prior):
    w = synth.random_wfst(400, 8, n_sym=4, p_eps=0.15, seed=7)
    c = synth.random_walk_corpus(w, 200, min_arcs=3, max_arcs=12, seed=7, out_degree=8)
    if lock:
        w = locked(w)
    same(lambda: _fb(w, c, norm_group=group, add_count=0.25 if lock else 0.0, smooth_floor=0.1, weight_is_prior_count=as_prior))


# every tail of a 1024-parameter piece and of its 256-parameter rows, and more pieces than the grid has workgroups
SIZES = [1, 255, 256, 257, 1023, 1024, 1025, 4 * 1024 + 3, 2049 * 1024 + 5]


@pytest.mark.gpu
@pytest.mark.parametrize("n_arcs", SIZES)
@pytest.mark.parametrize("deg,lock", [(3, False), (20, True)])
def test_parameter_counts(n_arcs, deg, lock):
    w, c = sized_model(n_arcs, deg, seed=n_arcs % 1000)
    if lock and n_arcs > 1:
        w = locked(w)
    same(lambda: _fb(w, c, norm_group=NORM_CONDITIONAL if deg == 3 else NORM_JOINT))


@pytest.mark.gpu
@pytest.mark.parametrize("grid", ["8", "100000"])
def test_other_grids(grid):
    """mstep_wide = N: at most N workgroups -- eight of them walking 41 pieces, and one workgroup per piece"""
    w, c = sized_model(40 * 1024 + 700, 5, seed=3)
    same(lambda: _fb(locked(w), c, norm_group=NORM_JOINT), env={"CARMEL_HIP_MSTEP_WIDE": grid})


@pytest.mark.gpu
@pytest.mark.parametrize("lock", [False, True])
def test_over_relaxed_step(lock):
    """maximize(1.5): save_old 1, then the second normalisation with save_old 0, and max_change_kernel delivers the result"""
    w = synth.random_wfst(500, 6, n_sym=4, p_eps=0.15, seed=13)
    c = synth.random_walk_corpus(w, 200, min_arcs=3, max_arcs=12, seed=13, out_degree=6)
    if lock:
        w = locked(w)
    same(lambda: _fb(w, c), delta=1.5)


@pytest.mark.gpu
@pytest.mark.parametrize("lock", [False, True])
def test_without_the_mailbox(lock):
    w = synth.random_wfst(700, 6, n_sym=4, p_eps=0.15, seed=17)
    c = synth.random_walk_corpus(w, 200, min_arcs=3, max_arcs=12, seed=17, out_degree=6)
    if lock:
        w = locked(w)
    with_box = same(lambda: _fb(w, c))
    without = same(lambda: _fb(w, c), env={"CARMEL_HIP_MAILBOX": "0"})
    assert [x[1] for x in with_box if not isinstance(x[1], np.ndarray)] == [x[1] for x in without if not isinstance(x[1], np.ndarray)]


@pytest.mark.gpu
def test_tied_arcs_keep_their_own_path():
    """a model with ties is not the window kernel's (either form): it must simply still train.  (Both runs take the general
    M-step, whose tie totals are sums by floating-point atomics in whatever order the hardware serves them: not bit for bit
    from run to run, so the two are compared to 1e-9, far above the last bits a reordered sum of a few dozen terms can move.)"""
    w = synth.random_wfst(40, 8, n_sym=4, p_eps=0.15, seed=9)
    c = synth.random_walk_corpus(w, 200, min_arcs=3, max_arcs=12, seed=9, out_degree=8)
    w.logw[:] = 0.0
    rng = np.random.default_rng(3)
    grp = w.group.copy()
    tied = rng.choice(len(grp), size=max(2, len(grp) // 16), replace=False)
    grp[tied] = rng.integers(1, 3, size=len(tied)).astype(np.uint32)  # tie ids 1, 2
    w = Wfst(w.n_states, w.final, w.src, w.dst, w.isym, w.osym, w.logw, grp)
    new, old = rounds(lambda: _fb(w, c), {}), rounds(lambda: _fb(w, c), OLD)
    for (name, a), (_, b) in zip(new, old):
        np.testing.assert_allclose(np.exp(a) if isinstance(a, np.ndarray) and name[0] != "c" else a,
                                   np.exp(b) if isinstance(b, np.ndarray) and name[0] != "c" else b, rtol=1e-9, atol=1e-300, err_msg=name)
    assert np.isfinite(new[-1][1]) and 0.0 < new[-1][1] <= 1.0


def _cipher_cascade(oracle):
    lm, ch, co = synth.cipher_files(90, min_len=5, max_len=30, seed=5)
    oc = oracle.OracleCascade([lm, ch])
    a = oc.composed().arrays()
    w = Wfst(a["n_states"], a["final"], a["src"], a["dst"], a["isym"], a["osym"], a["logw"], a["group"])
    ca = oc.corpus(co).arrays()
    c = Corpus(ca["in_off"], ca["in_sym"], ca["out_off"], ca["out_sym"], ca["weight"])
    return lambda: _fb(w, c, cascade=oc.as_dict([NORM_NONE, NORM_CONDITIONAL], [0.0, 0.25]))


@pytest.mark.gpu
def test_a_member_normalised_by_none(oracle):
    """a cascade whose first member keeps its weights (code16 = 0xffff for its parameters).  The initial normalisation is
    compared bit for bit.  The iterations cannot be: a cascade's parameter counts are summed over the composed arcs by
    floating-point atomics (chain_scatter_kernel), in an order that changes from run to run, so the M-step's INPUT already
    differs in its last bits between two runs of the same library (measured when this was written: 98 of the 1486 weights
    differed between two runs of the OLD kernels after the first iteration and 218 after the second, by at most 1.1e-15 relative;
    119 and 269 between two runs of the new one).  They are compared to 1e-9 relative: the sums have at most a few thousand terms, whose
    reordering moves a result by far less, and a wrong member or a wrong branch moves it by far more."""
    make = _cipher_cascade(oracle)
    new, old = rounds(make, {}), rounds(make, OLD)
    assert np.array_equal(new[0][1], old[0][1]) and np.any(np.isfinite(new[0][1]))
    for (name, a), (_, b) in zip(new[1:], old[1:]):
        if name.startswith("weights"):
            assert np.array_equal(np.isneginf(a), np.isneginf(b)), name
            np.testing.assert_allclose(np.exp(a), np.exp(b), rtol=1e-9, atol=1e-300, err_msg=name)
        elif name.startswith("counts"):
            np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-300, err_msg=name)
        else:
            assert a == b, name  # (a cascade's maximize reports the constant of train.cc:922)


# ---------------- no GPU: what the compiler made of the kernel ----------------
def makefile_flags():
    txt = open(os.path.join(ROOT, "carmel_amd", "csrc", "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*=\s*(.*)$" % name, txt, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    rule = re.search(r"^mstep_wide\.o:.*\n\t(.*)$", txt, flags=re.M).group(1)
    flags = []
    for name in ("CXXFLAGS", "HIPFLAGS", "WIDEFLAGS"):
        if "$(%s)" % name in rule:
            flags += var(name)
    assert "--offload-arch=gfx950" in flags
    return flags


def test_the_kernel_uses_no_scratch_and_keeps_four_workgroups_per_cu():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "carmel_amd", "csrc", "mstep_wide.hip")
    r = subprocess.run([hipcc] + makefile_flags() + ["--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    found = 0
    for m in re.finditer(r"^(_Z\w*mstep_wide_kernel\w*):.*?\n\ts_endpgm(.*?)(?=^_Z\w+:|\Z)", r.stdout, flags=re.S | re.M):
        name, tail = m.group(1), m.group(2)
        scratch, occ = re.search(r"; ScratchSize: (\d+)", tail), re.search(r"; Occupancy: (\d+)", tail)
        assert scratch and occ, name
        assert int(scratch.group(1)) == 0, (name, scratch.group(0))
        assert int(occ.group(1)) >= 4, (name, occ.group(0))  # waves per SIMD = 256-thread workgroups per CU
        found += 1
    assert found == 6, found  # <NEED_LW> x <mask32, mask64, scan>
