"""GPU: pruning the whole machine by best-path weight (carmel_hip_decoder_prune, csrc/decode_prune.hip) against the reference of
prune_ref.py on the cases and the grid of prune_cases.py (proved on the CPU by test_prune_host.py): the masks byte for byte, the
two distance arrays bit for bit, F[final] and P* against best_paths(1); the same bytes from the lane form and the wave form; the
`ulp` case, whose best path only the exemption of P* keeps; an unreachable final state; refused machines and error codes;
set_weights; alternation with decode() and best_paths()."""
import ctypes as C

import numpy as np
import pytest

from prune_cases import LOG_RATIOS, MIN_ARC_LOGWS, REFUSED, distances, grid, machine, max_states_grid, names, reference, ulp, ulp_property
from prune_ref import NO_CAP, Distances

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5
NEVER = str(2 ** 32 - 1)
NEG_INF = -np.inf


def cap(n):
    return None if n == NO_CAP else n


def check_point(d, name, log_ratio, max_states, min_arc_logw):
    state_keep, arc_keep = d.prune(log_ratio, cap(max_states), min_arc_logw)
    want_states, want_arcs = reference(name, log_ratio, max_states, min_arc_logw)
    where = (name, log_ratio, max_states, min_arc_logw)
    assert state_keep.astype(np.uint8).tobytes() == want_states.tobytes(), where
    assert arc_keep.astype(np.uint8).tobytes() == want_arcs.tobytes(), where


@pytest.mark.parametrize("name", names())
def test_device_equals_the_reference(name):
    from carmel_amd.decode import Decoder
    w = machine(name)
    d = Decoder(w)
    for point in grid(name):
        check_point(d, name, *point)
    for min_arc_logw in MIN_ARC_LOGWS:
        ref = distances(name, min_arc_logw)
        d.prune(min_arc_logw=min_arc_logw)
        F, R = d.prune_distances()
        assert F.tobytes() == np.array(ref.F).tobytes() and R.tobytes() == np.array(ref.R).tobytes(), (name, min_arc_logw)
        assert d.prune_stats() == (ref.fwd_rounds, ref.bwd_rounds), (name, min_arc_logw)
    # F[final] is the value of best_paths(1)'s path, and P* is that path
    ref = distances(name, NEG_INF)
    d.prune()
    F, _ = d.prune_distances()
    best = d.best_paths(1)
    d.close()
    if not best:
        assert F[w.final] == NEG_INF and ref.pstar == []
        return
    arcs = [int(a) for a in best[0][1]]
    v = 0.0
    for a in arcs:
        v = v + float(w.logw[a])
    assert np.float64(v).tobytes() == F[w.final].tobytes()
    assert arcs == ref.pstar


@pytest.mark.parametrize("name", ["hub", "medium"])
def test_lane_form_and_wave_form_give_the_same_bytes(name):
    """option best_paths_wave_degree at 0 (every state by a wavefront), unset (32), 8 and never: the hub's final state has 200
    in-arcs and, reversed, its state 0 has 200; the medium machine has states on both sides of 8 in-arcs either way round"""
    import carmel_amd
    from carmel_amd.decode import Decoder
    w = machine(name)
    points = [(0.0, NO_CAP, NEG_INF), (float(np.log(2.0)), 3, NEG_INF), (float(np.log(10.0)), w.n_states - 1, float(np.log(0.25)))]
    d = Decoder(w)
    raws = {}
    try:
        for setting in ("0", None, "8", NEVER):
            carmel_amd.set_option("best_paths_wave_degree", setting)
            for p in points:
                s, a = d.prune(p[0], cap(p[1]), p[2])
                raws[setting, p] = [s.tobytes(), a.tobytes()] + [x.tobytes() for x in d.prune_distances()]
    finally:
        carmel_amd.set_option("best_paths_wave_degree", None)
    d.close()
    for p in points:
        assert all(raws[s, p] == raws[None, p] for s in ("0", "8", NEVER)), (name, p)
        ref = distances(name, p[2])
        want = [x.astype(bool).tobytes() for x in ref.masks(p[0], p[1])] + [np.array(ref.F).tobytes(), np.array(ref.R).tobytes()]
        assert raws[None, p] == want, (name, p)


def test_the_ulp_case_keeps_the_best_path_at_a_ratio_of_one():
    """some arc of P* has T(a) < F[final] by rounding: only the exemption keeps it at log_ratio = 0"""
    from carmel_amd.decode import Decoder
    w = ulp()
    ref = Distances(w)
    below = ulp_property(w)
    assert below
    d = Decoder(w)
    state_keep, arc_keep = d.prune(0.0)
    F, R = d.prune_distances()
    best = d.best_paths(1)
    d.close()
    assert [int(a) for a in best[0][1]] == ref.pstar
    assert all((F[w.src[a]] + w.logw[a]) + R[w.dst[a]] < F[w.final] for a in below)  # the device's own numbers say so too
    assert all(arc_keep[a] for a in ref.pstar) and arc_keep.sum() == len(ref.pstar)
    assert all(state_keep[w.src[a]] and state_keep[w.dst[a]] for a in ref.pstar)


def test_an_unreachable_final_state_succeeds_with_nothing_kept():
    from carmel_amd.decode import Decoder
    d = Decoder(machine("unreachable"))
    for log_ratio in LOG_RATIOS:
        state_keep, arc_keep = d.prune(log_ratio)
        assert not state_keep.any() and not arc_keep.any()
    F, R = d.prune_distances()
    assert F.tolist()[2] == NEG_INF and R.tolist() == [NEG_INF, NEG_INF, 0.0]
    d.close()


def test_a_refused_call_leaves_the_previous_results():
    from carmel_amd._capi import CarmelHipError
    from carmel_amd.decode import Decoder
    for name, (wr, arc) in REFUSED.items():
        d = Decoder(wr)
        best, paths = d.decode([[1]])
        with pytest.raises(CarmelHipError) as e:
            d.prune_distances()  # nothing to read yet
        assert e.value.code == ERR_STATE
        for _ in range(2):
            with pytest.raises(CarmelHipError, match=r"arc %d " % arc) as e:
                d.prune(0.0)
            assert e.value.code == ERR_UNSUPPORTED, name
        best2, _ = d.decode([[1]])
        assert best.tobytes() == best2.tobytes()
        d.set_weights(np.minimum(wr.logw, 0.0))  # the weight above 1 taken away: legal
        state_keep, arc_keep = d.prune(0.0)
        assert state_keep[0] and state_keep[wr.final]
        kept = [x.tobytes() for x in d.prune_distances()]
        stats = d.prune_stats()
        d.set_weights(wr.logw)
        with pytest.raises(CarmelHipError) as e:
            d.prune(0.0)
        assert e.value.code == ERR_UNSUPPORTED
        with pytest.raises(CarmelHipError) as e:
            d.prune(-1.0)
        assert e.value.code == ERR_ARG
        assert [x.tobytes() for x in d.prune_distances()] == kept and d.prune_stats() == stats
        d.close()


def test_error_codes():
    from carmel_amd._capi import lib, ptr
    from carmel_amd.decode import Decoder
    w = machine("dag3")
    d = Decoder(w)
    s, a = np.zeros(w.n_states, np.uint8), np.zeros(w.n_arcs, np.uint8)
    ns, na = C.c_uint64(77), C.c_uint64(77)
    inf, none = float("inf"), 0xFFFFFFFF
    call = lambda h, r, n, p, sp, ap: lib.carmel_hip_decoder_prune(h, r, n, p, sp, ap, C.byref(ns), C.byref(na))
    assert lib.carmel_hip_decoder_prune_distances(d._h, None, None) == ERR_STATE
    assert call(None, 0.0, none, -inf, ptr(s), ptr(a)) == ERR_ARG
    assert call(d._h, 0.0, none, -inf, None, ptr(a)) == ERR_ARG
    assert call(d._h, 0.0, none, -inf, ptr(s), None) == ERR_ARG
    assert call(d._h, float("nan"), none, -inf, ptr(s), ptr(a)) == ERR_ARG
    assert call(d._h, -0.5, none, -inf, ptr(s), ptr(a)) == ERR_ARG
    assert call(d._h, 0.0, 0, -inf, ptr(s), ptr(a)) == ERR_ARG
    assert call(d._h, 0.0, none, float("nan"), ptr(s), ptr(a)) == ERR_ARG
    assert ns.value == 77 and not s.any() and lib.carmel_hip_decoder_prune_distances(d._h, None, None) == ERR_STATE
    assert call(d._h, inf, none, -inf, ptr(s), ptr(a)) == 0 and ns.value == 4 and na.value == 5 and s.all() and a.all()
    assert lib.carmel_hip_decoder_prune(d._h, 0.0, none, -inf, ptr(s), ptr(a), None, None) == 0 and s.sum() == 3 and a.sum() == 2
    assert lib.carmel_hip_decoder_prune_distances(d._h, None, None) == 0
    assert lib.carmel_hip_decoder_prune_distances(None, None, None) == ERR_ARG
    f, b = C.c_uint32(), C.c_uint32()
    assert lib.carmel_hip_decoder_prune_stats(d._h, None, C.byref(b)) == ERR_ARG
    assert lib.carmel_hip_decoder_prune_stats(d._h, C.byref(f), C.byref(b)) == 0 and f.value >= 2 and b.value >= 2
    assert d.last_ms() > 0.0
    d.close()


def test_set_weights_is_seen_by_the_next_call():
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    w = machine("dag3")
    d = Decoder(w)
    state_keep, arc_keep = d.prune(0.0)
    assert arc_keep.tolist() == [True, False, False, True, False]  # 0 -> 1 -> 3 at 0.25
    logw = w.logw.copy()
    logw[2] = 0.0  # the direct arc 0 -> 3 becomes the best path
    logw[0] = -np.inf  # and the path through state 1 disappears
    d.set_weights(logw)
    w2 = Wfst(w.n_states, w.final, w.src, w.dst, w.isym, w.osym, logw)
    for point in [(0.0, NO_CAP, NEG_INF), (np.inf, NO_CAP, NEG_INF), (float(np.log(10.0)), 3, float(np.log(0.25)))]:
        ref = Distances(w2, point[2])
        got = d.prune(point[0], cap(point[1]), point[2])
        assert [x.tobytes() for x in got] == [x.astype(bool).tobytes() for x in ref.masks(point[0], point[1])], point
        assert [x.tobytes() for x in d.prune_distances()] == [np.array(ref.F).tobytes(), np.array(ref.R).tobytes()]
    assert d.prune(0.0)[1].tolist() == [False, False, True, False, False]
    d.set_weights(w.logw)
    check_point(d, "dag3", 0.0, NO_CAP, NEG_INF)
    d.close()


def test_alternates_with_decode_and_best_paths_on_one_handle():
    from best_paths_cases import reference as best_reference
    from carmel_amd.decode import Decoder
    w = machine("random5")
    lines = [[1, 2], [2], [], [3, 1, 1], [1]]
    alone = Decoder(w)
    best0, paths0 = alone.decode(lines)
    alone.close()
    d = Decoder(w)
    for point in grid("random5")[:6]:
        best, paths = d.decode(lines)
        check_point(d, "random5", *point)
        got = d.best_paths(5)
        assert [[int(a) for a in p] for _, p in got] == [p for _, _, p in best_reference("random5", 5)]
        check_point(d, "random5", *point)
        assert best.tobytes() == best0.tobytes() and all(np.array_equal(a, b) for a, b in zip(paths, paths0))
    d.close()
    assert len(max_states_grid(w.n_states)) == 4
