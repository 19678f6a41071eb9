"""CPU: the f80 restatement of the explicit-lattice E-step (sweep_ref.py) and its derived tolerance, on the restatement
alone: on every case of test_sweep_f80_gpu.py the same walk in f64 (numpy's sums, the library's exp and log) stays within
the tolerance of the f80 run, the tolerance comes out under 1e-10, the image has the layout the case is meant to force, and
the f64 walk is the oracle's E-step to the 1e-7 of the older tests (the f80 run is a reference for precision, the oracle for
structure)."""
import numpy as np
import pytest

import dense_ref as dr
import helpers
import sweep_math_cases  # noqa: F401  (asserts that numpy's longdouble is wider than a double)
import sweep_ref as sr
from carmel_amd.model import NORM_CONDITIONAL


def test_dtype_argument_leaves_the_f64_walk_as_it_was():
    """the default is float64 and every value it returns is one"""
    case = sr.by_name("tile-fused")
    img = helpers.host_lattices(case.w, case.c)
    counts, plp = helpers.numpy_sweep(img, case.w.logw, case.c.n_pairs)
    assert counts.dtype == np.float64 and plp.dtype == np.float64
    c80, p80, _ = sr.reference(img, case.w.logw, case.c.n_pairs)
    assert c80.dtype == np.longdouble and p80.dtype == np.longdouble
    assert helpers._lse([0.0, 0.0]) == np.log(2.0) and helpers._lwadd(0.0, 0.0) == np.log(2.0)
    assert abs(helpers._lse([0.0, 0.0], np.longdouble) - np.log(np.longdouble(2))) < 1e-18


@pytest.mark.parametrize("name", sr.NAMES)
def test_f64_walk_within_the_derived_tolerance_of_the_f80_walk(name, hipopt, oracle):
    case = sr.by_name(name)
    for k, v in case.options.items():
        hipopt.set(k, v)
    w, c = case.w, case.c
    ow, oc = oracle.OracleWfst.from_arrays(w), oracle.OracleCorpus.from_arrays(c)
    if case.kw.get("normalize_first", True):
        ow.normalize(NORM_CONDITIONAL, 0.0)
    logw = np.array(ow.arrays()["logw"], np.float64)
    img = sr.image(case)
    ref_counts, ref_lnp, tol = sr.reference(img, logw, c.n_pairs)
    print("%s: %s" % (name, tol))
    assert tol.lnp < sr.CEILING and tol.counts < sr.CEILING
    counts, lnp = helpers.numpy_sweep(img, logw, c.n_pairs)
    e_lnp, e_counts = dr.compare_lnp(lnp, ref_lnp, tol.lnp), dr.compare_counts(counts, ref_counts, tol.counts)
    print("    f64 walk: ln p %.3g (%.3f of the bound), counts %.3g (%.3f)" % (e_lnp, e_lnp / tol.lnp, e_counts, e_counts / tol.counts))
    r = oracle.estimate(ow, oc)
    ok = r["has_deriv"]
    assert np.array_equal(ok, img["has_deriv"].astype(bool))
    np.testing.assert_allclose(lnp[ok], r["pair_logprob"][ok], rtol=1e-9, atol=1e-9)
    want = np.exp(r["counts_ln"])
    np.testing.assert_allclose(counts, want, rtol=1e-7, atol=1e-14 * max(1.0, want.max()))
