"""Inputs, references and bounds shared by test_sweep_math_host.py and test_sweep_math_gpu.py: the arguments at which
csrc/sweep_math.hpp's exp_le0, log_ge1 and Lse are probed (tests/native/sweep_math_probe.hip), their values in numpy's
longdouble (64-bit mantissa: asserted), and the error measures.  Everything is computed once per process.

ulp.  An error is measured in units of the spacing of the doubles at the EXACT value: 2^(e - 53) for |exact| in
[2^(e - 1), 2^e), and 2^-1074 throughout the denormals.  The longdouble reference is itself within 2^-63 of the exact value,
1/1024 of such a unit, which the bounds' margins absorb.

Lse bound (`lse_bound`).  value() = m + log_ge1(acc), acc = sum_i exp_le0(x_i - m) with m the running maximum, u = 2^-53:
  * a term below the maximum: the difference x - m is rounded (u |d|, which the exponential turns into u |d| e^-|d| <= 0.37 u of
    the sum, the sum being at least 1), the exponential is within 1 ulp (<= 2 u of a term that is at most 1), the addition is
    rounded (u): under 4 u of the sum;
  * a new maximum: one exponential (1 ulp), one rounded product, one rounded addition on the whole sum so far, 4 u, plus the
    rounding of its argument, u |d| times the share the old sum keeps in the new one;
  * relative errors of the sum survive later rescalings unchanged and are only diluted by later terms, so they add up to 4 n u;
  * a relative error e of acc is an absolute error e of ln acc; log_ge1 is within 2.5 ulp of ln acc; the last addition rounds
    to u |value|.
That gives the form the tests assert,
    |value - ref| <= (4 n + 4) u + u |ref|,   n = the row's finite terms,
as a first-order bound.  It is not a worst case in three places, each of which only matters when every rounding falls the
same way: 1 ulp of an exponential can be 2 u of it; a new maximum t nats above a sum of k old terms costs up to
u t k e^-t / (1 + k e^-t) <= u max(ln k, 0.75) for its argument; and 2.5 ulp of ln acc is up to 5 u ln n.  The worst case
with all three is ((5 + ln n) n + 5 ln n) u + u |ref|; the tests hold the code to the tighter form above, which host
evaluation meets with a wide margin (profiles/measurement_log_sweep_math.md)."""
import ctypes as C
import functools
import os

import numpy as np

assert np.finfo(np.longdouble).eps < 1e-18, "numpy's longdouble is no wider than a double here: no reference to compare with"

LD = np.longdouble
U = 2.0 ** -53
EXP_ULP, LOG_ULP = 1.0, 2.5          # the bounds of the two functions against the exact value
EXP_ZERO_BELOW = -745.2              # exactly 0 at and below
NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
BUILDS = {"contract": "libsweepprobe.so", "nocontract": "libsweepprobe_nc.so"}
LSE_SIZES = (1, 2, 3, 63, 64, 65, 1000, 4096)


class Probe(object):
    """one build of the probe; where = "host" or "device" """

    def __init__(self, build):
        self.lib = C.CDLL(os.path.join(NATIVE, BUILDS[build]))
        for fn in ("exp", "log"):
            for where in ("host", "device"):
                f = getattr(self.lib, "sweep_probe_%s_%s" % (fn, where))
                f.argtypes, f.restype = [C.c_void_p, C.c_void_p, C.c_int64], C.c_int
        for where in ("host", "device"):
            f = getattr(self.lib, "sweep_probe_lse_" + where)
            f.argtypes, f.restype = [C.c_void_p] * 2 + [C.c_int64] + [C.c_void_p] * 3, C.c_int

    def _map(self, fn, where, x):
        x = np.ascontiguousarray(x, np.float64)
        y = np.full(len(x), np.nan)
        rc = getattr(self.lib, "sweep_probe_%s_%s" % (fn, where))(x.ctypes.data, y.ctypes.data, len(x))
        assert rc == 0, "sweep_probe_%s_%s failed: %d" % (fn, where, rc)
        return y

    def exp(self, x, where):
        return self._map("exp", where, x)

    def log(self, x, where):
        return self._map("log", where, x)

    def lse(self, terms, off, where):
        """(value, m, acc) per row"""
        terms, off = np.ascontiguousarray(terms, np.float64), np.ascontiguousarray(off, np.int64)
        out = [np.full(len(off) - 1, np.nan) for _ in range(3)]
        rc = getattr(self.lib, "sweep_probe_lse_" + where)(terms.ctypes.data, off.ctypes.data, len(off) - 1,
                                                          *(o.ctypes.data for o in out))
        assert rc == 0, "sweep_probe_lse_%s failed: %d" % (where, rc)
        return out


@functools.lru_cache(maxsize=None)
def probe(build):
    return Probe(build)


def neighbours(centres, n):
    """the n doubles around each centre (n / 2 below, n / 2 - 1 above)"""
    c = np.ascontiguousarray(centres, np.float64).view(np.int64)
    return (c[:, None] + np.arange(-(n // 2), n - n // 2, dtype=np.int64)[None, :]).ravel().view(np.float64)


def ulp_of(ref):
    """the spacing of the doubles at the exact value `ref` (longdouble)"""
    _, e = np.frexp(ref)
    return np.ldexp(LD(1), np.maximum(e.astype(np.int64) - 53, -1074).astype(np.int32))


def ulp_err(got, ref):
    """|got - ref| in ulps of the exact value, per element (float64); got must be finite"""
    assert np.isfinite(got).all(), "inf or nan among the results"
    return (np.abs(np.asarray(got, LD) - ref) / ulp_of(ref)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# exp and log: named groups of arguments, the longdouble value of each
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exp_groups():
    """[(name, x)]: every x here has a positive exp (the bound is 1 ulp); exp_zero_points() holds the ones that give 0"""
    rng = np.random.default_rng(20261)
    g = [("uniform [%g, %g]" % (lo, hi), rng.uniform(lo, hi, 1000000))
         for lo, hi in ((-1e-3, 0.0), (-1.0, 0.0), (-40.0, 0.0), (EXP_ZERO_BELOW, 0.0), (0.0, 40.0))]
    k = np.arange(1, 2101, dtype=np.float64)
    flips = neighbours(-k * (np.log(2.0) / 2), 400)  # where rint(x / ln 2) flips (odd k) and the reduced argument is 0 (even k)
    g.append(("neighbours of -k ln2 / 2", flips[flips > EXP_ZERO_BELOW]))
    den = np.concatenate([rng.uniform(EXP_ZERO_BELOW, -708.3, 400000), neighbours(np.array([-708.3964185322641, -744.4400719213812, -745.1332191019411]), 400)])
    g.append(("denormal results [-745.2, -708.3]", den[den > EXP_ZERO_BELOW]))
    g.append(("chosen points", np.array([0.0, -0.0, 1e-9, -1e-9, -1e-300, -5e-324, -np.log(2.0), -36.7368005696771, -708.0, -745.0])))
    return tuple(g)


def exp_zero_points():
    rng = np.random.default_rng(20262)
    return np.concatenate([np.array([EXP_ZERO_BELOW, -745.2000000001, -746.0, -1075 * np.log(2.0), -1099.9, -1100.0, -1100.1,
                                     -1587.0, -2000.0, -1e4, -1e308, -np.inf]), rng.uniform(-1200.0, EXP_ZERO_BELOW, 20000)])


@functools.lru_cache(maxsize=None)
def log_groups():
    rng = np.random.default_rng(20263)
    one = np.array([1.0]).view(np.int64)[0]
    g = [("the first 2e6 doubles above 1", (one + np.arange(0, 2000000, dtype=np.int64)).view(np.float64))]
    g += [("uniform [1, %g]" % hi, rng.uniform(1.0, hi, 1000000)) for hi in (1.0001, 2.0, 4096.0, 2.0 ** 32)]
    k = np.arange(0, 1023, dtype=np.float64)
    g.append(("neighbours of sqrt(2) 2^k", neighbours(np.sqrt(2.0) * 2.0 ** k, 64)))  # frexp's mantissa either side of sqrt(1/2)
    g.append(("integers 1 .. 1e5", np.arange(1, 100001, dtype=np.float64)))
    g.append(("powers of two", 2.0 ** np.arange(0, 1024, dtype=np.float64)))
    g.append(("neighbours above powers of two, the largest doubles", np.concatenate([
        neighbours(2.0 ** np.arange(1, 1024, dtype=np.float64), 16), neighbours(np.array([np.finfo(np.float64).max]), 16)[:8]])))
    assert all((x >= 1).all() and np.isfinite(x).all() for _, x in g)
    return tuple(g)


@functools.lru_cache(maxsize=None)
def exp_all():
    """(x, longdouble exp x, the group's slice per name)"""
    return _flatten(exp_groups(), np.exp)


@functools.lru_cache(maxsize=None)
def log_all():
    return _flatten(log_groups(), np.log)


def _flatten(groups, fn):
    x = np.concatenate([v for _, v in groups])
    ref = fn(x.astype(LD))
    ref.setflags(write=False)
    x.setflags(write=False)
    at, sl = 0, {}
    for name, v in groups:
        sl[name] = slice(at, at + len(v))
        at += len(v)
    return x, ref, sl


# ---------------------------------------------------------------------------------------------------------------------
# Lse rows
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lse_rows():
    """(terms, off, kinds): a CSR of rows and one label per row"""
    rng = np.random.default_rng(20264)
    rows, kinds = [], []

    def add(kind, xs):
        rows.append(np.asarray(xs, np.float64))
        kinds.append(kind)
    for n in LSE_SIZES:
        for scale in (1.0, 40.0):
            base = rng.uniform(-scale, 0.0, n)
            add("random", base)
            add("ascending", np.sort(base))          # a new maximum, and a rescaling, at every term
            add("descending", np.sort(base)[::-1])
            add("positive", base + scale + rng.uniform(0.0, 3.0))   # an unnormalised model: every term above 0
            add("near -1e4", base - 1e4)
            dead = rng.random(n) < 0.3
            add("-inf interleaved", np.where(dead, -np.inf, base))
            k = max(1, n // 3)
            add("-inf leading", np.concatenate([np.full(k, -np.inf), base]))
            add("-inf trailing", np.concatenate([base, np.full(k, -np.inf)]))
        add("ascending by ln n", np.log(float(n) + 1) * np.arange(n))  # each maximum about as large as the sum before it
        for v in (0.0, -3.25, 7.5, -1e4, -0.1):
            add("equal", np.full(n, v))
        add("all -inf", np.full(n, -np.inf))
    for v in (0.0, -0.0, -1e-300, 5e-324, -745.5, 1e300, -1e300, np.log(0.3)):
        add("one term", [v])
        add("one term among -inf", [-np.inf, v, -np.inf])
    for gap in (36.5, 40.0, 745.0, 2000.0, 36.0, 36.7368005696771, 37.5, 700.0, 744.0, 746.0, 1099.0, 1101.0, 1e5):
        for big in (0.0, -12.375, 3.0, -1e4):
            add("two terms", [big, big - gap])
            add("two terms", [big - gap, big])
    add("empty", [])
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    terms = np.concatenate(rows)
    terms.setflags(write=False)
    off.setflags(write=False)
    return terms, off, tuple(kinds)


@functools.lru_cache(maxsize=None)
def lse_reference():
    """(longdouble log-sum-exp per row, finite terms per row)"""
    terms, off, _ = lse_rows()
    ref, n = np.full(len(off) - 1, -np.inf, LD), np.zeros(len(off) - 1, np.int64)
    for r in range(len(off) - 1):
        x = terms[off[r]:off[r + 1]].astype(LD)
        x = x[x > -np.inf]
        n[r] = len(x)
        if len(x):
            m = x.max()
            ref[r] = m + np.log(np.exp(x - m).sum())
    return ref, n


def lse_bound(n, ref):
    return ((4.0 * n + 4.0) * U + U * np.abs(ref)).astype(LD)


def check_lse(value, m, acc):
    """every assertion on the rows of lse_rows(); returns the largest error / bound over the rows with a finite value"""
    terms, off, kinds = lse_rows()
    ref, n = lse_reference()
    dead = n == 0
    assert np.isneginf(value[dead]).all() and (acc[dead] == 0).all(), "a row without a finite term"
    live = ~dead
    assert np.isfinite(value[live]).all(), "inf or nan among the values"
    ratio = (np.abs(value[live].astype(LD) - ref[live]) / lse_bound(n[live], ref[live])).astype(np.float64)
    worst = int(np.argmax(ratio))
    assert ratio[worst] <= 1.0, "Lse row %d (%s, %d terms): error %.3g x its bound" % (
        np.nonzero(live)[0][worst], kinds[np.nonzero(live)[0][worst]], n[live][worst], ratio[worst])
    for r, kind in enumerate(kinds):
        x = terms[off[r]:off[r + 1]]
        fin = x[x > -np.inf]
        if len(fin):
            assert m[r] == fin.max()
        if len(fin) == 1:  # the bits of that term (the sign of a zero included)
            assert acc[r] == 1.0 and np.array([value[r]]).view(np.int64)[0] == fin.view(np.int64)[0], (r, kind)
        if kind == "equal":
            assert acc[r] == len(x), (r, acc[r])
        if kind == "two terms":
            gap = abs(float(LD(x[0]) - LD(x[1])))
            if gap > 745:
                assert value[r] == x.max() and acc[r] == 1.0, (r, x)
            elif gap <= 36.5:
                assert acc[r] > 1.0, (r, x)
    return float(ratio[worst])
