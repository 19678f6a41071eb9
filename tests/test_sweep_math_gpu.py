"""GPU: csrc/sweep_math.hpp's exp_le0, log_ge1 and Lse on the device, one thread per element, in the two ways the product
compiles them -- the flags of kernels.o / tile_sweep.o (default contraction) and those of decode_sum.o (-ffp-contract=off) --
on the arrays of test_sweep_math_host.py (sweep_math_cases.py).

exp and log: the same ulp bounds against longdouble as on the host, and the BITS of host evaluation.  Every operation of the
two functions is an exactly specified IEEE operation (explicit fma, rint, frexp, ldexp, one division, and no
multiplication feeding an addition that a compiler could contract), so a device that differs from the host in one bit has
an instruction that is not what the source says.
Lse: the derived bound for both builds.  `acc * K_EXP(m - x) + 1.0` is one fma in the first build and a product and a sum in
the second, so the two may differ in the last bits: whether they do is printed, not asserted."""
import numpy as np
import pytest

import sweep_math_cases as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=sorted(sm.BUILDS))
def build(request):
    return request.param


def _same_bits(dev, host, x, what):
    diff = np.nonzero(dev.view(np.int64) != host.view(np.int64))[0]
    assert len(diff) == 0, "%s: %d of %d results differ from host evaluation, first at %r: device %r, host %r" % (
        what, len(diff), len(x), x[diff[0]], dev[diff[0]], host[diff[0]])


def test_exp_on_the_device(build):
    p = sm.probe(build)
    x, ref, groups = sm.exp_all()
    y = p.exp(x, "device")
    err = sm.ulp_err(y, ref)
    for name, sl in groups.items():
        k = int(np.argmax(err[sl]))
        print("exp_le0 device %-10s %-36s %8d points  worst %.4f ulp at %r" % (build, name, sl.stop - sl.start, err[sl][k], x[sl][k]))
    k = int(np.argmax(err))
    assert err[k] <= sm.EXP_ULP, "exp_le0(%r) is %.4f ulp from the exact value" % (x[k], err[k])
    _same_bits(y, p.exp(x, "host"), x, "exp_le0")
    z = np.concatenate([sm.exp_zero_points(), [0.0, -0.0]])
    yz = p.exp(z, "device")
    assert (yz[:-2] == 0).all() and not np.signbit(yz[:-2]).any() and (yz[-2:] == 1.0).all()
    _same_bits(yz, p.exp(z, "host"), z, "exp_le0 (special values)")


def test_log_on_the_device(build):
    p = sm.probe(build)
    x, ref, groups = sm.log_all()
    y = p.log(x, "device")
    err = sm.ulp_err(y, ref)
    for name, sl in groups.items():
        k = int(np.argmax(err[sl]))
        print("log_ge1 device %-10s %-36s %8d points  worst %.4f ulp at %r" % (build, name, sl.stop - sl.start, err[sl][k], x[sl][k]))
    k = int(np.argmax(err))
    assert err[k] <= sm.LOG_ULP, "log_ge1(%r) is %.4f ulp from the exact value" % (x[k], err[k])
    assert (y[x == 1.0] == 0).all() and not np.signbit(y[x == 1.0]).any()
    _same_bits(y, p.log(x, "host"), x, "log_ge1")


def test_lse_on_the_device(build):
    p = sm.probe(build)
    terms, off, _ = sm.lse_rows()
    value, m, acc = p.lse(terms, off, "device")
    ratio = sm.check_lse(value, m, acc)
    hv, hm, ha = p.lse(terms, off, "host")
    assert np.array_equal(m.view(np.int64), hm.view(np.int64))
    print("Lse device %-10s %d rows  worst error / bound %.4f; %d values and %d sums differ from host evaluation" % (
        build, len(off) - 1, ratio, (value.view(np.int64) != hv.view(np.int64)).sum(), (acc.view(np.int64) != ha.view(np.int64)).sum()))


def test_lse_builds_against_each_other():
    """reported, not asserted: the contracted and the uncontracted Lse agree or differ by an fma's rounding"""
    terms, off, _ = sm.lse_rows()
    a = sm.probe("contract").lse(terms, off, "device")
    b = sm.probe("nocontract").lse(terms, off, "device")
    dv, da = (a[0].view(np.int64) != b[0].view(np.int64)), (a[2].view(np.int64) != b[2].view(np.int64))
    print("Lse contract vs nocontract on the device: %d of %d values and %d sums differ in their bits" % (dv.sum(), len(dv), da.sum()))
    assert np.array_equal(a[1].view(np.int64), b[1].view(np.int64))  # (the running maximum is a comparison: no arithmetic)
    fin = np.isfinite(a[0])
    assert np.array_equal(fin, np.isfinite(b[0]))
