"""GPU: every explicit-lattice sweep kernel against the f80 restatement of the E-step (sweep_ref.py), at the tolerance that
module derives from the run itself -- under 1e-10 for every case here, three orders below the 1e-7 at which
test_gpu_parity.py, test_wave_gpu.py and test_lattice_gpu.py compare the same kernels with the (f64, 36-nat) oracle.  Each
case also keeps that oracle comparison: the f80 run is a reference for precision, the oracle for structure.

Families (sweep_ref.CASES; forced with the switches the older tests use, and each test asserts from the trainer's layout
that the intended kernel was given the corpus):
    tile     tile_sweep_kernel; the three kernels on its layout (tile_sweep_kernel=0); the five kernels over 16384-position
             tiles (tile_sweep=0, lane_fused=0); lattices with no arc at all
    lane     plain groups of 1, 63, 64 and 65 lattices: sweep_lane_kernel<.., XC> (fused), sweep -> post -> tile pass
             (lane_fused_kernel=0), the 16384-position layout (lane_fused=0); windowed groups through rings of 8 .. 64 rows,
             fused and not; the gather formulation (transpose=0), plain and windowed
    wave     sweep_wave_kernel, ring and full, with and without lane lattices beside it; levels of several rows
    bundle   the 64-, 256- and 1024-thread classes of sweep_bundle_kernel (no lattice on a lane or a wavefront)
    serial   cyclic lattices
Edges, on tile, lane and wave each: pair weights 1e-300, 1e6 and 0; zero-weight arcs in 15 % of the positions; an
unnormalised model with weights up to 4; every arc near 1e-100 (ln p about -5000: the bound grows with |ln p| and the sweep
stays inside it); derivations 1e-250 apart; a sum of 70 equal terms (24 in the tile sweep, whose lattices end at 48 arcs);
a second estimate() after maximize(1.0), against the f80 run at the weights the trainer then reports.

What is compared (dense_ref.compare_counts / compare_lnp): counts relative, on the entries above 1e-200 x the total;
counts the reference has as exactly 0 exactly 0; ln p relative to max(1, |ln p|), -inf where the reference has -inf.

NOT covered, on purpose:
  * sweep_lane_kernel<R, W, PRE, Lse, WIN, XC>: launch_lane_sweep (kernels.hip) has six instantiations and the lane family
    reaches each -- <4, 2, true, .., false, true> (fused), <4, 2, true, .., true, true> (windowed, fused), <3, 1, true>
    (lane_fused_kernel=0, lane_fused=0), <4, 2, true, .., true, false> (windowed, lane_fused_kernel=0), <4, 2, false> and
    <4, 2, false, .., true> (transpose=0) -- so none is left out.  Left out are the paths inside them that a corpus of this
    size does not take: weights gathered from a table beyond the caches' threshold (the choice is made by the table's
    size), `lane_chunks` > 1 (an experiment switch) and the `lane_trace` stamps.
  * the record-free single-path sweep of a tile-sweep group, reached only by groups made of single paths alone (bench.py's
    config 4): test_tile_sweep_is_the_three_kernels_it_replaces[paths] holds it to the bits of the kernels measured here.
  * 64 equal in-arcs in the tile sweep: its lattices have at most 48 arcs; 24 are tested.
  * the wave sweep's choices of weight source and way out (wave_gather, wave_xc): test_wave_gpu.py holds all four to the same
    bits, and the default of each is what runs here.
  * the M-step and the transposition passes beyond what counts() passes through; matrix_fb.hip; the decoders (their own
    files carry f80-measured tolerances); the unrolled and dense layouts (test_dense_gpu.py)."""
import re

import numpy as np
import pytest

import dense_ref as dr
import sweep_math_cases  # noqa: F401  (asserts that numpy's longdouble is wider than a double)
import sweep_ref as sr
from carmel_amd.model import Wfst

pytestmark = pytest.mark.gpu


def _expect(case, fb, layout):
    """the kernel the case is about was given the corpus: from the trainer's own description of its layout"""
    e, ls = case.expect, fb.lattice_stats
    if "tile" in e:
        assert (fb.tile_sweep_tiles > 0) == e["tile"]
    if "fused" in e:
        assert (fb.fused_lane_tiles > 0) == e["fused"]
    if "windowed" in e:
        assert (ls.n_windowed_pairs > 0) == e["windowed"]
    waves = re.findall(r"wave class count=(\d+) max_states=(\d+) max_width=(\d+) ring=(\d+)", layout)
    bundles = re.findall(r"bundle class count=(\d+) block=(\d+) max_states=(\d+) serial=(\d+)", layout)
    if e.get("lanes_only"):  # (a corpus of lane lattices alone is built on the GPU, which prints no classes; else the layout line)
        assert ls.n_cyclic_pairs == 0 and not waves and not bundles
        assert "lattices built on the GPU" in layout or re.search(r"timing: layout .* bundles=0 ", layout)
    if e.get("waves"):
        assert waves and not bundles
        if case.options.get("wave_ring") == "0":
            assert all(x[3] == "0" for x in waves)
    if e.get("bundles"):
        assert bundles and not waves and "lane piece" not in layout
        assert sorted({int(x[1]) for x in bundles}) == sorted(e["blocks"]) and all(x[3] == "0" for x in bundles)
    if "cyclic" in e:
        assert ls.n_cyclic_pairs >= e["cyclic"] and any(x[3] == "1" for x in bundles)


def _compare(case, fb, oracle, img, what):
    w, c = case.w, case.c
    logw = fb.weights().copy()
    lp, _ = fb.estimate(per_pair=True)
    counts, lnp = fb.counts(), fb.pair_logprob.copy()
    assert np.array_equal(fb.has_deriv.astype(bool), img["has_deriv"].astype(bool))
    ref_counts, ref_lnp, tol = sr.reference(img, logw, c.n_pairs)
    assert tol.lnp < sr.CEILING and tol.counts < sr.CEILING
    e_lnp, e_counts = dr.compare_lnp(lnp, ref_lnp), dr.compare_counts(counts, ref_counts)
    print("f80 %-26s %-8s %s | observed ln p %.3g (%.4f of the bound), counts %.3g (%.4f)" % (
        case.name, what, tol, e_lnp, e_lnp / tol.lnp, e_counts, e_counts / tol.counts))
    assert e_lnp <= tol.lnp, "ln p: error %.3g above the bound %.3g" % (e_lnp, tol.lnp)
    assert e_counts <= tol.counts, "counts: relative error %.3g above the bound %.3g" % (e_counts, tol.counts)
    live = np.isfinite(ref_lnp.astype(np.float64))
    assert abs(lp - float(ref_lnp[live].sum())) <= tol.lnp * max(1.0, float(np.abs(ref_lnp[live]).sum()))
    # ... and the oracle, for gross errors
    ow, oc = oracle.OracleWfst.from_arrays(Wfst(w.n_states, w.final, w.src, w.dst, w.isym, w.osym, logw, w.group)), oracle.OracleCorpus.from_arrays(c)
    r = oracle.estimate(ow, oc)
    ok = r["has_deriv"]
    assert np.array_equal(ok, fb.has_deriv.astype(bool))
    np.testing.assert_allclose(lnp[ok], r["pair_logprob"][ok], rtol=1e-9, atol=1e-9)
    want = np.exp(r["counts_ln"])
    np.testing.assert_allclose(counts, want, rtol=1e-7, atol=1e-14 * max(1.0, want.max()))


@pytest.mark.parametrize("name", sr.NAMES)
def test_sweep_within_the_derived_tolerance_of_the_f80_run(name, hipopt, oracle, capfd):
    from carmel_amd.trainer import HipForwardBackward
    case = sr.by_name(name)
    hipopt.set("timing", "1")
    for k, v in case.options.items():
        hipopt.set(k, v)
    img = sr.image(case)
    capfd.readouterr()
    fb = HipForwardBackward(case.w, case.c, **case.kw)
    layout = capfd.readouterr().err
    try:
        _expect(case, fb, layout)
        _compare(case, fb, oracle, img, "first")
        if case.second:
            fb.maximize(1.0)
            _compare(case, fb, oracle, img, "second")
    finally:
        fb.close()
