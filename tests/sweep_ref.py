"""The explicit-lattice E-step restated in extended precision, its tolerance, and the cases it is tested on
(test_sweep_ref_host.py on the CPU, test_sweep_f80_gpu.py against every sweep kernel).

Reference.  helpers.numpy_sweep walks the host builder's image of the lattices -- lane streams, wave rows, bundles, the
cyclic lattices' in-order scatter -- and test_lattice_host.py pins that walk against the oracle.  `reference` is the same
walk with dtype = numpy's longdouble (64-bit mantissa: asserted when sweep_math_cases is imported): the weights, every alpha
and beta, the sums, the posteriors, the counts and ln p.  It is a reference for PRECISION; the layout it walks need not be
the one the kernel under test was given (a sum is the same sum in every layout), and every test pairs it with the oracle
comparison that catches gross errors.  Its own error, a few 2^-64 per operation, is 1/2048 of what it measures.

Tolerance (`Tolerance`), u = 2^-53, from what the run reports (helpers.SweepStats).  A chain is one pass over one lattice:
its dependent sums one after the other (the levels; the states of a lane lattice; the pairwise adds of a cyclic one).
L is the longest chain, D the largest sum over a chain of the most terms a sum of each step has (at most L times the
largest in- or out-degree d), A the largest |ln alpha|, |ln beta|, |term| or |ln p| stored, N the most posteriors summed into
one arc.
  * A state's sum.  Each of its d terms is ln alpha + ln w, one rounded addition of values up to A: u A.  The streaming
    log-sum-exp of d terms is within (4 d + 4) u + u |value| of the exact one of its inputs (sweep_math_cases.py; exp_le0 within
    1 ulp, log_ge1 within 2.5).  A log-sum-exp moves by at most the largest error of its terms.  So a stored log value is
    off by at most
        (a A + 4 d + b) u,   a = 2, b = 4
    more than the worst of its inputs, and at the end of a chain by
        E = (L (2 A + 4) + 4 D) u.
    That bounds ln p absolutely; ln p is compared relative to max(1, |ln p|), which is no smaller.
  * beta of the goal is ln weight - ln p, one more step of one term (counted in L and D); the backward chain adds its own E.
  * A posterior is exp(ln alpha + (ln w + ln beta)): the errors of alpha and beta, two rounded additions of values up to A,
    and an exponential within 1 ulp (2 u); an absolute error e of the argument is a relative error e of the result:
    2 E + (2 A + 2) u.
  * A count sums up to N non-negative posteriors in some order: N u more.
        ln p:  E        counts:  2 E + (2 A + 2 + N) u
  * Cyclic lattices are swept with pairwise log-adds, ln(1 + e^-|d|): each is a step of two terms (library exp and log1p
    within 1 ulp fit the same 4 d + 4) that drops the smaller term beyond 36 nats.  The f80 run cuts at the same 36, but a
    difference within rounding of 36 may fall on the other side in f64: e^-36 = 2.4e-16 of the sum per add.  With c the
    most adds in one pass over a cyclic lattice, E grows by c 2.4e-16.
Every case below must come out under 1e-10 (asserted in test_sweep_ref_host.py): a case that does not is made smaller."""
import numpy as np

import helpers
from carmel_amd import synth
from carmel_amd.model import NORM_NONE, Corpus, Wfst

LD = np.longdouble
U = 2.0 ** -53
CUT = 2.4e-16  # e^-36
CEILING = 1e-10


class Tolerance(object):
    def __init__(self, st):
        self.L, self.D, self.A, self.N, self.cyclic = st.L, st.D, st.A, st.N, st.cyclic
        self.lnp = (self.L * (2.0 * self.A + 4.0) + 4.0 * self.D) * U + self.cyclic * CUT
        self.counts = 2.0 * self.lnp + (2.0 * self.A + 2.0 + self.N) * U

    def __repr__(self):
        return "L=%d D=%d A=%.4g N=%d%s: ln p %.3g, counts %.3g" % (
            self.L, self.D, self.A, self.N, " cyclic=%d" % self.cyclic if self.cyclic else "", self.lnp, self.counts)


def reference(img, logw, n_pairs, dtype=LD):
    """(counts per arc, ln p per pair, Tolerance) of the image under the weights logw"""
    st = helpers.SweepStats(len(logw))
    counts, plp = helpers.numpy_sweep(img, logw, n_pairs, dtype=dtype, stats=st)
    return counts, plp, Tolerance(st)


def image(case):
    """the host builder's image under the case's options (set them first: the hipopt fixture), and what the case expects of
    the layout as far as the image shows it"""
    img = helpers.host_lattices(case.w, case.c, lane_states=int(case.options.get("lane_states", -1)))
    e, waves, groups = case.expect, img["waves"]["descs"], img["lane_groups"]
    if e.get("lanes_only"):
        assert len(groups) and not len(img["bundles"]) and not len(waves)
    if "tile" in e and "transpose" not in case.options:  # (the image is built without that switch, which only the trainer reads)
        assert (len(img["transpose"]["tile_group"]) > 0) == e["tile"]
    if "windowed" in e:
        assert bool((groups["window"] > 0).any()) == e["windowed"]
    if e.get("waves"):
        assert len(waves) and not len(img["bundles"])
        if case.options.get("wave_ring") == "0":
            assert not waves["ring"].any()
    if e.get("wide"):  # a level of several rows of 64 records
        assert int(np.diff(img["waves"]["frow"].astype(np.int64)).max()) > 1
    if e.get("bundles"):  # (classes: first, count, block, max_states, serial)
        assert len(img["bundles"]) and not len(waves) and not len(groups) and not img["n_cyclic"]
        assert sorted(set(img["classes"][:, 2].tolist())) == sorted(e["blocks"])
    if "cyclic" in e:
        assert img["n_cyclic"] >= e["cyclic"]
    return img


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
class Case(object):
    """make() -> (w, c): the transducer and corpus (built on first use); kw: HipForwardBackward's arguments; options: the
    library's switches; expect: what the test asserts about the layout (test_sweep_f80_gpu._expect); second: a second
    estimate() after maximize(1.0)"""

    def __init__(self, name, family, make, options, expect, kw=None, second=False):
        self.name, self.family, self._make, self._wc = name, family, make, None
        self.options, self.expect, self.kw, self.second = dict(options), dict(expect), dict(kw or {}), second

    def _built(self):
        if self._wc is None:
            self._wc = self._make()
        return self._wc

    @property
    def w(self):
        return self._built()[0]

    @property
    def c(self):
        return self._built()[1]


RAW = dict(norm_group=NORM_NONE, normalize_first=False)


def _with_logw(w, logw):
    return Wfst(w.n_states, w.final, w.src, w.dst, w.isym, w.osym, logw, w.group)


def _weighted(w, c, seed, lo=0.5, hi=3.0):
    c.weight[:] = np.random.default_rng(seed).uniform(lo, hi, c.n_pairs)
    return w, c


def _live_pairs(w, c):
    """the pairs that keep a path of non-zero weight (f64 walk of the default image)"""
    with np.errstate(invalid="ignore"):  # (a dead pair's beta is ln weight + inf)
        _, plp = helpers.numpy_sweep(helpers.host_lattices(w, c), w.logw, c.n_pairs)
    keep = np.nonzero(np.isfinite(plp))[0]
    assert 0 < len(keep) < c.n_pairs
    return c.subset(keep)


def fan_model(width):
    """start -a:x-> `width` states -b:y-> the final state, every weight 1 / width: a level of `width` states and a final state
    whose sum has `width` equal terms (acc is exactly `width`)"""
    F = 1 + width
    src = [0] * width + list(range(1, 1 + width))
    dst = list(range(1, 1 + width)) + [F] * width
    sym = [2] * width + [3] * width
    w = Wfst(F + 1, F, src, dst, sym, sym, np.log(np.full(2 * width, 1.0 / width)))
    return w, Corpus.from_lists([([2, 3], [2, 3])] * 3, weights=[1.0, 0.25, 3.0])


def _walks(n_states, deg, n_sym, p_eps, n_pairs, lo, hi):
    def base(seed):
        w = synth.random_wfst(n_states, deg, n_sym=n_sym, p_eps=p_eps, seed=500 + seed)
        return w, synth.random_walk_corpus(w, n_pairs, min_arcs=lo, max_arcs=hi, seed=500 + seed, out_degree=deg)
    return base


def _edges(family, base, options, expect, fan_width, tiny_base=None):
    """the edge cases of one family on its base model: base(seed) -> (w, c); tiny_base: the model of the 1e-100 case, where the
    bound grows with |ln p| and the base model's longest pairs would take it past 1e-10"""
    def pair_weights():
        w, c = base(1)
        c.weight[:] = np.resize([1e-300, 1e6, 0.0, 2.5, 1.0], c.n_pairs)
        return w, c

    def zero_weight_arcs():
        rng = np.random.default_rng(72)
        w, c = base(2)
        w.logw[rng.random(w.n_arcs) < 0.15] = -np.inf
        return _weighted(w, _live_pairs(w, c), 72)

    def unnormalised():
        w, c = base(3)
        return _with_logw(w, np.log(np.random.default_rng(73).uniform(0.05, 4.0, w.n_arcs))), c

    def tiny():
        w, c = (tiny_base or base)(4)
        return _with_logw(w, np.log(1e-100) + np.log(np.random.default_rng(74).uniform(0.5, 1.5, w.n_arcs))), c

    def apart():
        w, c = base(5)
        return _with_logw(w, w.logw + np.where(np.random.default_rng(75).random(w.n_arcs) < 0.1, np.log(1e-250), 0.0)), c

    return [Case(family + "-pair-weights", family, pair_weights, options, expect),
            Case(family + "-zero-weight-arcs", family, zero_weight_arcs, options, expect),
            Case(family + "-unnormalised", family, unnormalised, options, expect, RAW),
            Case(family + "-arcs-near-1e-100", family, tiny, options, expect, RAW),
            Case(family + "-1e-250-apart", family, apart, options, expect, RAW),
            Case(family + "-fan-%d" % fan_width, family, lambda: fan_model(fan_width), options, expect, RAW),
            Case(family + "-second-estimate", family, lambda: _weighted(*base(6), seed=76), options, expect, second=True)]


def _no_arc_corpus():
    """lattices with no arc at all: two empty strings under a model whose start state is final, among short ambiguous pairs"""
    rng = np.random.default_rng(7)
    isym, osym = np.array([2, 3, 4, 4], np.uint32), np.array([2, 3, 2, 3], np.uint32)
    w = Wfst(1, 0, np.zeros(4, np.uint32), np.zeros(4, np.uint32), isym, osym, np.log([0.4, 0.3, 0.2, 0.1]))
    pairs = [([], [])] * 70
    for _ in range(130):
        arcs = rng.integers(0, 4, int(rng.integers(1, 9)))
        pairs.append((isym[arcs].tolist(), osym[arcs].tolist()))
    order = rng.permutation(len(pairs))
    return w, Corpus.from_lists([pairs[i] for i in order], weights=rng.uniform(0.5, 2.0, len(pairs)))


def _tile_cases():
    out = []
    base = _walks(30, 4, 3, 0.0, 200, 3, 9)
    for mode, opts in (("fused", {}), ("kernels", {"tile_sweep_kernel": "0"}), ("layout", {"tile_sweep": "0", "lane_fused": "0"})):
        expect = dict(tile=mode != "layout", fused=False, lanes_only=True)  # (layout: the five kernels over 16384-position tiles)
        out.append(Case("tile-%s" % mode, "tile", lambda: _weighted(*base(0), seed=1), opts, expect))
        out.append(Case("tile-%s-no-arc" % mode, "tile", _no_arc_corpus, opts, expect, RAW))
    # (a lattice of the tile sweep has at most 48 arcs: its widest fan is 24 equal terms)
    return out + _edges("tile", base, {}, dict(tile=True, lanes_only=True), 24)


def _lane_cases():
    out = []
    for mode, opts in (("fused", {}), ("kernels", {"lane_fused_kernel": "0"}), ("layout", {"lane_fused": "0"})):
        opts = dict(opts, wave_min_width="1e9", tile_sweep="0")  # (these lattices are small enough for the tile sweep)
        expect = dict(tile=False, fused=mode != "layout", lanes_only=True, windowed=False)
        for n in (1, 63, 64, 65):  # partial groups: one lattice per lane, 64 lanes
            out.append(Case("lane-%s-%d" % (mode, n), "lane", lambda n=n: _weighted(*_walks(40, 5, 4, 0.1, n, 10, 25)(10 + n), seed=n),
                            opts, expect))
    def narrow(window):
        return lambda: _weighted(*_walks(20, 3, 5, 0.05, 150, 20, 70)(20 + window), seed=window, lo=0.25, hi=2.0)
    for window in (8, 16, 32, 64):  # long narrow lattices through a ring of `window` rows: sweep_lane_kernel<4, 2, true, Lse, true, true>
        wopts = dict(lane_window_min="4", lane_window=str(window), wave_min_width="1e9")
        out.append(Case("lane-window-%d" % window, "lane", narrow(window), wopts, dict(tile=False, fused=True, windowed=True)))
    # (those lattices are close to single paths, whose sums read the neighbouring state from a register and not from the ring: a
    # ring mask off by one passes them at 8, 16 and 32.)  Positions x members states with members^2 arcs between positions:
    # every sum reads `members` rows of the ring, and the arcs span 2 members - 1 states, just inside the window
    def ambiguous(members, n_pairs):
        def make():
            w = synth.clustered_wfst(4 * members + 1, 3 * members, members=members, n_sym=5, p_eps=0.0, n_in_sym=3, seed=60 + members)
            c = synth.clustered_walk_corpus(w, n_pairs, 3 * members, members=members, min_arcs=8, max_arcs=24, seed=60 + members)
            return _weighted(w, c, members)
        return make
    for window, members, n_pairs in ((8, 3, 80), (16, 6, 40), (32, 12, 12)):
        out.append(Case("lane-window-%d-ambiguous" % window, "lane", ambiguous(members, n_pairs),
                        dict(lane_window_min="4", lane_window=str(window), wave_min_width="1e9"), dict(tile=False, fused=True, windowed=True)))
    # ... and <4, 2, true, Lse, true, false>: the ring without the fused way out
    out.append(Case("lane-window-16-kernels", "lane", narrow(16), dict(wopts, lane_window="16", lane_fused_kernel="0"),
                    dict(tile=False, windowed=True)))
    # the gather formulation (no weight pass: PRE = false), plain <4, 2, false> and windowed <4, 2, false, Lse, true>
    g = dict(transpose="0", tile_sweep="0", wave_min_width="1e9")
    out.append(Case("lane-gather-65", "lane", lambda: _weighted(*_walks(40, 5, 4, 0.1, 65, 10, 25)(75), seed=65), g,
                    dict(tile=False, fused=False, lanes_only=True, windowed=False)))
    out.append(Case("lane-gather-window-16", "lane", narrow(16), dict(g, lane_window_min="4", lane_window="16"),
                    dict(tile=False, fused=False, windowed=True)))
    return out + _edges("lane", _walks(40, 5, 4, 0.1, 100, 10, 25), dict(wave_min_width="1e9", tile_sweep="0"),
                        dict(tile=False, fused=True, lanes_only=True), 70, tiny_base=_walks(40, 5, 4, 0.1, 100, 10, 22))


def _wave_cases():
    out = []

    def narrow(seed):
        w = synth.random_wfst(14 + 4 * seed, 4 + seed % 3, n_sym=3 + seed % 2, p_eps=0.12, seed=90 + seed)
        return _weighted(w, synth.random_walk_corpus(w, 100, min_arcs=3, max_arcs=25, seed=90 + seed, out_degree=4 + seed % 3), seed)

    def wide():  # levels of more than 64 arcs (several rows per level), states with twelve in-arcs
        w = synth.clustered_wfst(12 * 4 + 1, 48, members=12, n_sym=6, n_in_sym=3, seed=21)
        return w, synth.clustered_walk_corpus(w, 30, 48, members=12, min_arcs=3, max_arcs=20, seed=21)
    for ring in ("1", "0"):
        for seed, lane_states in ((1, "0"), (3, "12")):
            out.append(Case("wave-ring%s-lanes%s" % (ring, lane_states), "wave", lambda seed=seed: narrow(seed),
                            dict(wave_min_width="0", wave_ring=ring, lane_states=lane_states), dict(waves=True)))
        out.append(Case("wave-ring%s-wide-levels" % ring, "wave", wide, dict(wave_min_width="0", wave_ring=ring, lane_states="0"),
                        dict(waves=True, wide=True)))
    # (the fan: a level of 70 states and 70 arcs, and a state with 70 in-arcs)
    return out + _edges("wave", _walks(22, 5, 4, 0.12, 100, 3, 25), dict(wave_min_width="0", lane_states="0"), dict(waves=True), 70)


def _bundle_cases():
    opts = dict(lane_states="0", wave_min_width="1e9")

    def big(members, length):
        # positions x members states, members^2 arcs between positions and into the goal: 2048 < states <= 8192 is the
        # 256-thread class, more the 1024-thread class
        def make():
            w = synth.clustered_wfst(2 * members + 1, 3 * members, members=members, n_sym=4, p_eps=0.0, n_in_sym=3, seed=3)
            return w, synth.clustered_walk_corpus(w, 2, 3 * members, members=members, min_arcs=length - 5, max_arcs=length, seed=3)
        return make
    return [Case("bundle-small", "bundle", lambda: _weighted(*_walks(40, 8, 4, 0.0, 150, 3, 14)(31), seed=31), opts,
                 dict(bundles=True, blocks=(64,))),
            Case("bundle-256-threads", "bundle", big(32, 75), opts, dict(bundles=True, blocks=(256,))),
            Case("bundle-1024-threads", "bundle", big(112, 78), opts, dict(bundles=True, blocks=(256, 1024)))]


def _serial_cases():
    def two():
        sym = [2, 0, 3, 0, 3]
        w = Wfst(4, 3, [0, 1, 1, 2, 2], [1, 2, 3, 1, 3], sym, sym, np.log([1.0, 0.3, 0.7, 0.4, 0.6]))
        return w, Corpus.from_lists([([2, 3], [2, 3]), ([2, 3], [2, 3])], [1.0, 2.5])

    def many():  # epsilon cycles in most lattices
        w = synth.random_wfst(6, 5, n_sym=3, p_eps=0.2, seed=21)
        return _weighted(w, synth.random_walk_corpus(w, 20, min_arcs=4, max_arcs=10, seed=21, out_degree=5), 44)
    return [Case("serial-two-cyclic", "serial", two, {}, dict(cyclic=2), RAW),
            Case("serial-epsilon-cycles", "serial", many, {}, dict(cyclic=10))]


CASES = _tile_cases() + _lane_cases() + _wave_cases() + _bundle_cases() + _serial_cases()
NAMES = [c.name for c in CASES]
assert len(set(NAMES)) == len(NAMES)


def by_name(name):
    return CASES[NAMES.index(name)]
