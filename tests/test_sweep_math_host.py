"""CPU: csrc/sweep_math.hpp's exp_le0, log_ge1 and Lse, evaluated on the host by the probe (tests/native/sweep_math_probe.hip
includes the product's header), against numpy's longdouble.  The bounds, against the EXACT value:
    exp_le0   1 ulp; exactly 0 at and below -745.2; exactly 1 at +-0
    log_ge1   2.5 ulp; exactly 0 at 1
    Lse       (4 n + 4) u + u |ref|            (derived in sweep_math_cases.py)
The arguments and the derivation are in sweep_math_cases.py; test_sweep_math_gpu.py runs the same arrays through the two
device builds and holds the device to the bits of what is evaluated here.  The host code of the two builds is the same
arithmetic (x86-64 without FMA contraction), which the last test pins."""
import numpy as np
import pytest

import sweep_math_cases as sm


@pytest.fixture(scope="module", params=sorted(sm.BUILDS))
def probe(request):
    return sm.probe(request.param)


def test_exp_within_one_ulp_of_the_exact_value(probe):
    x, ref, groups = sm.exp_all()
    err = sm.ulp_err(probe.exp(x, "host"), ref)
    for name, sl in groups.items():
        k = int(np.argmax(err[sl]))
        print("exp_le0 host  %-36s %8d points  worst %.4f ulp at %r" % (name, sl.stop - sl.start, err[sl][k], x[sl][k]))
    k = int(np.argmax(err))
    assert err[k] <= sm.EXP_ULP, "exp_le0(%r) is %.4f ulp from the exact value" % (x[k], err[k])


def test_exp_special_values(probe):
    z = sm.exp_zero_points()
    y = probe.exp(z, "host")
    assert (y == 0).all() and not np.signbit(y).any(), z[y != 0]
    one = probe.exp(np.array([0.0, -0.0]), "host")
    assert (one == 1.0).all()
    tiny = probe.exp(np.array([1e-9, -1e-9]), "host")
    assert tiny[0] == 1.000000001 and tiny[1] == 0.999999999  # (correctly rounded: 1 + x + x^2 / 2 is within 2^-90 of both)


def test_log_within_two_and_a_half_ulp_of_the_exact_value(probe):
    x, ref, groups = sm.log_all()
    y = probe.log(x, "host")
    err = sm.ulp_err(y, ref)
    for name, sl in groups.items():
        k = int(np.argmax(err[sl]))
        print("log_ge1 host  %-36s %8d points  worst %.4f ulp at %r" % (name, sl.stop - sl.start, err[sl][k], x[sl][k]))
    k = int(np.argmax(err))
    assert err[k] <= sm.LOG_ULP, "log_ge1(%r) is %.4f ulp from the exact value" % (x[k], err[k])
    assert (y[x == 1.0] == 0).all() and not np.signbit(y[x == 1.0]).any()
    assert (y[x > 1.0] > 0).all()


def test_lse_rows_within_the_derived_bound(probe):
    terms, off, _ = sm.lse_rows()
    ratio = sm.check_lse(*probe.lse(terms, off, "host"))
    print("Lse host  %d rows  worst error / bound %.4f" % (len(off) - 1, ratio))


def test_the_two_builds_evaluate_the_same_bits_on_the_host():
    a, b = sm.probe("contract"), sm.probe("nocontract")
    x = sm.exp_all()[0]
    assert np.array_equal(a.exp(x, "host").view(np.int64), b.exp(x, "host").view(np.int64))
    x = sm.log_all()[0]
    assert np.array_equal(a.log(x, "host").view(np.int64), b.log(x, "host").view(np.int64))
    terms, off, _ = sm.lse_rows()
    for p, q in zip(a.lse(terms, off, "host"), b.lse(terms, off, "host")):
        assert np.array_equal(p.view(np.int64), q.view(np.int64))


def test_probe_refuses_rows_that_do_not_tile_the_terms(probe):
    out = [np.zeros(2) for _ in range(3)]
    off = np.array([0, 3, 1], np.int64)
    t = np.zeros(3)
    for where in ("host", "device"):  # (refused before any GPU call: this runs without one)
        rc = getattr(probe.lib, "sweep_probe_lse_" + where)(t.ctypes.data, off.ctypes.data, 2, *(o.ctypes.data for o in out))
        assert rc == -1
