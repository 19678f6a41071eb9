"""GPU: the sums over all paths of the whole machine (carmel_hip_decoder_machine_sums, csrc/decode_machine_sums.hip) against the
reference of machine_sums_ref.py on every case of machine_sums_cases.py (held on the CPU by test_machine_sums_host.py): alpha and
beta per state within the bound E the reference carries along (its docstring derives it; it is computed from the reference alone),
alpha[final] against beta[0], ln gamma within its bound, the path counts as integers below 2^53 and within their rounding bound
above, U, the levels and the stats integer for integer, -inf and 0xffffffff exactly where the rule says, the same bytes from two
calls; both forms of the sum at four settings of machine_sums_wave_degree; refused machines, their error code, the state the
message names and the earlier results left intact; set_weights; alternation with decode(), best_paths() and prune(); and the
cross-checks with the tropical entry points.

The cross-check on a single-path machine.  alpha follows the path from state 0, ((0 + w1) + w2) + ...: the VALUE of
carmel_hip_decoder_best_paths at K = 1, which carmel_hip_decoder_prune_distances returns as F[final] (the prune rule defines F as
exactly that list).  What best_paths REPORTS is the fold from the end, w1 + (w2 + (... + (wn + 0))), which is beta[0].  Both are
held bit for bit."""
import numpy as np
import pytest

from machine_sums_cases import REFUSED, SINGLE_PATH, WAVE_SETTINGS, accepted, machine, reference
from machine_sums_ref import LD, NONE, MachineSums

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5
EXACT = 2 ** 53
NEG_INF = -np.inf
CLOSING = {"cycle_in_u": (5, 4), "self_loop": (1, 1), "arc_into_0": (1, 0), "arc_out_of_final": (2, 1), "final0_loop": (1, 0)}  # (src, dst)


def call(d):
    """-> everything one call returns"""
    Z, N, n_useful = d.machine_sums()
    alpha, beta, cf, cb, level = d.machine_sums_states()
    return dict(Z=Z, N=N, n_useful=n_useful, alpha=alpha, beta=beta, cf=cf, cb=cb, level=level, gamma=d.machine_sums_arcs(),
                stats=d.machine_sums_stats())


def raw(got):
    return b"".join(np.asarray(got[k]).tobytes() for k in ("Z", "N", "alpha", "beta", "cf", "cb", "level", "gamma"))


def check(where, w, ref, got):
    """the device's results against the reference; -> the largest error / bound"""
    Q, final = w.n_states, w.final
    assert got["n_useful"] == ref.n_useful and got["stats"] == ref.levels, where
    assert got["level"].tolist() == ref.level, where
    assert got["Z"].hex() == float(got["alpha"][final]).hex() and got["N"] == got["cf"][final], where
    worst = 0.0

    def within(value, want, bound, what):
        nonlocal worst
        if want == NEG_INF:  # exactly where the rule says
            assert value == NEG_INF, (where, what, value)
            return
        assert np.isfinite(value), (where, what, value)
        err = abs(LD(value) - want)
        assert err <= bound, (where, what, float(value), float(want), float(err), float(bound))
        if bound > 0:
            worst = max(worst, float(err / bound))

    def count(value, want, adds, what):
        if want < EXACT:
            assert value == want and float(value).is_integer(), (where, what, value, want)
        else:
            assert abs(LD(value) - LD(want)) <= MachineSums.count_bound(adds) * LD(want), (where, what, value, want)

    for q in range(Q):
        assert (got["level"][q] == NONE) == (not ref.useful[q])
        within(got["alpha"][q], ref.alpha[q], ref.E[q], "alpha[%d]" % q)
        within(got["beta"][q], ref.beta[q], ref.Eb[q], "beta[%d]" % q)
        count(got["cf"][q], ref.cf[q], ref.F.adds[q], "cf[%d]" % q)
        count(got["cb"][q], ref.cb[q], ref.B.adds[q], "cb[%d]" % q)
    if ref.n_useful:
        assert got["alpha"][0] == 0.0 and got["beta"][final] == 0.0 and got["cf"][0] == 1.0 and got["cb"][final] == 1.0, where
        gap = abs(LD(got["alpha"][final]) - LD(got["beta"][0]))
        assert gap <= ref.E[final] + ref.Eb[0], (where, float(gap))
    else:
        assert got["Z"] == NEG_INF and got["N"] == 0.0 and got["stats"] == (0, 0), where
    for k in range(w.n_arcs):
        within(got["gamma"][k], ref.ln_gamma[k], ref.Eg[k], "ln gamma[%d]" % k)
    print("machine sums %s: Z %.17g, N %r, |U| %d, levels %r, worst error / bound %.3f" % (where, got["Z"], got["N"], got["n_useful"], got["stats"], worst))
    return worst


@pytest.mark.parametrize("name", accepted())
def test_device_equals_the_reference_and_two_calls_give_the_same_bytes(name):
    from carmel_amd.decode import Decoder
    w, ref = machine(name), reference(name)
    d = Decoder(w)
    first = call(d)
    check(name, w, ref, first)
    assert d.last_ms() > 0.0
    assert raw(call(d)) == raw(first), name
    d.close()


@pytest.mark.parametrize("name", accepted())
def test_both_forms_at_every_setting(name):
    """option machine_sums_wave_degree at 0 (every state by a wavefront), unset (32), 8 and never: every setting stays within the
    bounds, the integers do not move, the counts below 2^53 are identical, and a setting's second call returns its first call's bytes"""
    import carmel_amd
    from carmel_amd.decode import Decoder
    w, ref = machine(name), reference(name)
    d = Decoder(w)
    results = {}
    try:
        for setting in WAVE_SETTINGS:
            carmel_amd.set_option("machine_sums_wave_degree", setting)
            got = call(d)
            check("%s wave_degree=%s" % (name, setting), w, ref, got)
            assert raw(call(d)) == raw(got), (name, setting)
            results[setting] = got
    finally:
        carmel_amd.set_option("machine_sums_wave_degree", None)
    base = results[None]
    for setting, got in results.items():
        assert got["level"].tobytes() == base["level"].tobytes() and got["stats"] == base["stats"]
        for key, exact in (("cf", ref.cf), ("cb", ref.cb)):
            small = np.array([c < EXACT for c in exact])
            assert got[key][small].tobytes() == base[key][small].tobytes(), (name, setting, key)


def test_a_refused_call_names_the_state_and_leaves_the_previous_results():
    from carmel_amd._capi import CarmelHipError, lib
    from carmel_amd.decode import Decoder
    for name, stuck in REFUSED.items():
        w = machine(name)
        assert reference(name).stuck == stuck
        d = Decoder(w)
        with pytest.raises(CarmelHipError) as e:
            d.machine_sums_states()  # nothing to read yet
        assert e.value.code == ERR_STATE
        assert lib.carmel_hip_decoder_machine_sums_arcs(d._h, None) == ERR_STATE
        for _ in range(2):
            with pytest.raises(CarmelHipError, match=r"state %d lies on or behind a cycle" % stuck) as e:
                d.machine_sums()
            assert e.value.code == ERR_UNSUPPORTED, name
        with pytest.raises(CarmelHipError) as e:
            d.machine_sums_states()  # (still nothing)
        assert e.value.code == ERR_STATE
        # with the arc that closes the cycle at weight 0 the machine is legal; its results then survive the refusal of the old weights
        cut = w.logw.copy()
        back = [k for k in range(w.n_arcs) if (int(w.src[k]), int(w.dst[k])) == CLOSING[name]]
        assert len(back) == 1
        cut[back] = NEG_INF
        d.set_weights(cut)
        from carmel_amd.model import Wfst
        legal = Wfst(w.n_states, w.final, w.src, w.dst, w.isym, w.osym, cut)
        kept = call(d)
        check(name + " cut", legal, MachineSums(legal), kept)
        d.set_weights(w.logw)
        with pytest.raises(CarmelHipError) as e:
            d.machine_sums()
        assert e.value.code == ERR_UNSUPPORTED
        alpha, beta, cf, cb, level = d.machine_sums_states()
        after = dict(kept, alpha=alpha, beta=beta, cf=cf, cb=cb, level=level, gamma=d.machine_sums_arcs())
        assert raw(after) == raw(kept) and d.machine_sums_stats() == kept["stats"], name
        d.close()


def test_error_codes_and_null_pointers():
    import ctypes as C
    from carmel_amd._capi import lib, ptr
    from carmel_amd.decode import Decoder
    w = machine("diamond")
    d = Decoder(w)
    assert lib.carmel_hip_decoder_machine_sums(None, None, None, None) == ERR_ARG
    assert lib.carmel_hip_decoder_machine_sums_states(d._h, None, None, None, None, None) == ERR_STATE
    assert lib.carmel_hip_decoder_machine_sums(d._h, None, None, None) == 0  # every pointer is nullable
    assert lib.carmel_hip_decoder_machine_sums_states(d._h, None, None, None, None, None) == 0
    beta = np.empty(w.n_states)
    assert lib.carmel_hip_decoder_machine_sums_states(d._h, None, ptr(beta), None, None, None) == 0
    assert abs(beta[0] - float(reference("diamond").Z)) < 1e-14 and beta[w.final] == 0.0
    assert lib.carmel_hip_decoder_machine_sums_arcs(d._h, None) == 0
    f = C.c_uint32()
    assert lib.carmel_hip_decoder_machine_sums_stats(d._h, C.byref(f), None) == 0 and f.value == 3
    d.close()


def test_set_weights_is_seen_by_the_next_call():
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    w = machine("grid")
    d = Decoder(w)
    before = call(d)
    rng = np.random.default_rng(77)
    logw = rng.uniform(-3.0, 0.5, w.n_arcs)
    logw[rng.integers(0, w.n_arcs, 6)] = NEG_INF  # some arcs go: U and the counts change too
    w2 = Wfst(w.n_states, w.final, w.src, w.dst, w.isym, w.osym, logw)
    ref2 = MachineSums(w2)
    assert ref2.N not in (0, reference("grid").N)
    d.set_weights(logw)
    check("grid, new weights", w2, ref2, call(d))
    d.set_weights(w.logw)
    assert raw(call(d)) == raw(before)
    d.close()


def test_alternates_with_decode_best_paths_and_prune_on_one_handle():
    from carmel_amd.decode import Decoder
    name = "random19"
    w, ref = machine(name), reference(name)
    assert ref.N > 1
    lines = [[1], [1, 1], [], [1, 1, 1], [1, 1, 1, 1]]
    alone = Decoder(w)
    best0, paths0 = alone.decode(lines)
    kbest0 = alone.best_paths(4)
    keep0 = alone.prune(1.0)
    dist0 = alone.prune_distances()
    alone.close()
    d = Decoder(w)
    first = None
    for _ in range(3):
        best, paths = d.decode(lines)
        assert best.tobytes() == best0.tobytes() and [p.tolist() for p in paths] == [p.tolist() for p in paths0]
        got = call(d)
        first = first or got
        assert raw(got) == raw(first)
        kbest = d.best_paths(4)
        assert [(v, p.tolist()) for v, p in kbest] == [(v, p.tolist()) for v, p in kbest0]
        keep = d.prune(1.0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(keep + d.prune_distances(), keep0 + dist0))
        alpha = d.machine_sums_states()[0]  # the sums' results outlive the other entry points' calls
        assert alpha.tobytes() == first["alpha"].tobytes()
    check(name + ", alternating", w, ref, first)
    d.close()


@pytest.mark.parametrize("name", SINGLE_PATH)
def test_a_single_path_gives_the_best_path_bit_for_bit(name):
    from carmel_amd.decode import Decoder
    w = machine(name)
    d = Decoder(w)
    got = call(d)
    (reported, path), = d.best_paths(1)
    assert got["N"] == 1.0 and path.tolist() == list(range(w.n_arcs))
    d.prune()
    F, R = d.prune_distances()
    assert float(got["Z"]).hex() == float(F[w.final]).hex()       # the value: the arcs added in path order
    assert float(got["beta"][0]).hex() == float(reported).hex()   # the reported weight: the arcs added from the end
    assert got["alpha"].tobytes() == F.tobytes() and got["beta"].tobytes() == R.tobytes()
    d.close()


def test_the_sum_is_at_least_the_best_path_on_the_grid():
    from carmel_amd.decode import Decoder
    w = machine("grid")
    d = Decoder(w)
    got = call(d)
    d.prune()
    F, R = d.prune_distances()
    assert got["Z"] >= F[w.final] and got["beta"][0] >= R[0]
    assert (got["alpha"] >= F).all() and (got["beta"] >= R).all()
    assert got["Z"] <= F[w.final] + np.log(252.0) + 1e-12  # and at most 252 times it
    d.close()
