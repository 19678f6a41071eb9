"""GPU: the K best paths of the whole machine (carmel_hip_decoder_best_paths, csrc/decode_best_paths.hip) against the reference of
best_paths_ref.py on the cases of best_paths_cases.py (proved on the CPU by test_best_paths_host.py): values, reported weights and
arc sequences bit for bit; K = 1024; K = 1 against a plain Bellman-Ford; the same bytes from the lane form and the wave form of
the select kernel; the worklist's statistics on a chain; set_weights; alternation with decode(); refused calls and error codes."""
import numpy as np
import pytest

from best_paths_cases import HAND, KS, REFUSED, M, machine, names, reference
from best_paths_ref import Machine

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5
NEVER = str(2 ** 32 - 1)


def check_against_reference(w, got, ref, where):
    """got: Decoder.best_paths' list; ref: the reference's (value, reported weight, arcs)"""
    assert [[int(a) for a in p] for _, p in got] == [p for _, _, p in ref], where
    assert np.array([x for x, _ in got]).tobytes() == np.array([r for _, r, _ in ref]).tobytes(), where  # reported, bit for bit
    values = []
    for _, p in got:  # the value: the path's arcs added in path order
        v = 0.0
        for a in p:
            v = v + float(w.logw[a])
        values.append(v)
    assert np.array(values).tobytes() == np.array([v for v, _, _ in ref]).tobytes(), where


@pytest.mark.parametrize("name", names())
def test_device_equals_the_reference(name):
    from carmel_amd.decode import Decoder
    w = machine(name)
    d = Decoder(w)
    for K in KS:
        check_against_reference(w, d.best_paths(K), reference(name, K), (name, K))
    d.close()


def test_k_1024_fills_every_entry_of_the_two_state_cycle():
    """path r takes the cycle r times: 2 r + 1 arcs of weight one, so 1024 paths need 2047 rounds"""
    from carmel_amd.decode import Decoder
    d = Decoder(HAND["zero_cycle"])
    got = d.best_paths(1024)
    assert len(got) == 1024
    assert all(x == 0.0 and [int(a) for a in p] == [0] + [1, 0] * r for r, (x, p) in enumerate(got))
    rounds, selected = d.best_paths_stats()
    assert rounds <= 1024 * 2 + 1 and selected <= 2 * rounds
    d.close()


def bellman_ford(w):
    """the best value of a walk from 0 to the final state, sums in path order, Jacobi rounds"""
    m = Machine(w)
    d = [-np.inf] * m.n_states
    d[0] = 0.0
    for _ in range(m.n_states):
        new = [max([d[q]] + [d[s] + x for s, x, _ in m.ins[q] if d[s] > -np.inf]) for q in range(m.n_states)]
        if new == d:
            break
        d = new
    return d[m.final]


@pytest.mark.parametrize("name", ["medium", "hub", "chain", "positive_off_cycle", "random3", "random7", "dyadic11", "unreachable"])
def test_k_1_is_the_bellman_ford_value(name):
    from carmel_amd.decode import Decoder
    w = machine(name)
    d = Decoder(w)
    got = d.best_paths(1)
    d.close()
    want = bellman_ford(w)
    if want == -np.inf:
        assert got == []
        return
    v = 0.0
    for a in got[0][1]:
        v = v + float(w.logw[a])
    assert v == want, (name, v, want)


@pytest.mark.parametrize("name", ["hub", "medium"])
def test_lane_form_and_wave_form_give_the_same_bytes(name):
    """option best_paths_wave_degree at 0 (every state by a wavefront), unset (32), 8, 64 and never.  The hub's final state has 200
    in-arcs, so at the default and at 64 it takes the wave form while the 200 states before it take lanes; the medium machine has
    no state of more than 32 in-arcs, so there the default is all lanes, 0 all wavefronts and 8 a mixture (states on both sides
    of 8 in-arcs)."""
    import carmel_amd
    from carmel_amd.decode import Decoder
    w = machine(name)
    degree = np.bincount(w.dst[np.isfinite(w.logw)], minlength=w.n_states)
    if name == "hub":
        assert degree[w.final] == 200 and degree[:w.final].max() == 1
    else:
        assert degree.max() <= 32 and (degree > 8).sum() > 50 and (degree <= 8).sum() > 50
    d = Decoder(w)
    raws = {}
    try:
        for setting in ("0", None, NEVER, "8", "64"):
            carmel_amd.set_option("best_paths_wave_degree", setting)
            for K in (1, 5, 16):
                raws[setting, K] = [x.tobytes() for x in d.best_paths_raw(K)]
    finally:
        carmel_amd.set_option("best_paths_wave_degree", None)
    d.close()
    for K in (1, 5, 16):
        assert all(raws[s, K] == raws[None, K] for s in ("0", NEVER, "8", "64")), (name, K)
        check_against_reference(w, from_raw(raws[None, K]), reference(name, K), (name, K))


def from_raw(raw):
    logw, off, arcs = (np.frombuffer(b, t) for b, t in zip(raw, (np.float64, np.uint64, np.uint32)))
    return [(float(logw[p]), arcs[int(off[p]):int(off[p + 1])]) for p in range(len(logw))]


def test_the_worklist_recomputes_only_what_changed():
    """the chain of 256 states: state t changes in round t alone"""
    from carmel_amd.decode import Decoder
    w = machine("chain")
    d = Decoder(w)
    assert len(d.best_paths(5)) == 1
    rounds, selected = d.best_paths_stats()
    print("chain: %d rounds, %d states selected" % (rounds, selected))
    assert rounds <= w.n_states + 1 and selected <= 2 * w.n_states
    assert d.last_ms() > 0.0
    d.close()


def test_set_weights_is_seen_by_the_next_call():
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    w = machine("dag3")
    d = Decoder(w)
    assert len(d.best_paths(8)) == 3
    logw = w.logw.copy()
    logw[2] = 0.0  # the direct arc 0 -> 3 becomes the best path
    logw[0] = -np.inf  # and the path through state 1 disappears
    d.set_weights(logw)
    w2 = Wfst(w.n_states, w.final, w.src, w.dst, w.isym, w.osym, logw)
    from best_paths_ref import best_paths
    ref = best_paths(w2, 8)
    assert len(ref) == 2 and ref[0][2] == [2]
    check_against_reference(w2, d.best_paths(8), ref, "set_weights")
    d.set_weights(w.logw)
    check_against_reference(w, d.best_paths(8), reference("dag3", 8), "set_weights back")
    d.close()


def test_alternates_with_decode_on_one_handle():
    from carmel_amd.decode import Decoder
    w = machine("random5")
    lines = [[1, 2], [2], [], [3, 1, 1], [1]]
    alone = Decoder(w)
    best0, paths0 = alone.decode(lines)
    alone.close()
    d = Decoder(w)
    best1, paths1 = d.decode(lines)
    check_against_reference(w, d.best_paths(5), reference("random5", 5), "between")
    best2, paths2 = d.decode(lines)
    check_against_reference(w, d.best_paths(16), reference("random5", 16), "after")
    d.close()
    for best, paths in ((best1, paths1), (best2, paths2)):
        assert best.tobytes() == best0.tobytes()
        assert all(np.array_equal(a, b) for a, b in zip(paths, paths0))


def test_a_refused_call_leaves_the_previous_results():
    from carmel_amd._capi import CarmelHipError
    from carmel_amd.decode import Decoder
    w = machine("dag3")
    d = Decoder(w)
    d.set_weights(np.where(np.arange(w.n_arcs) == 0, 0.5, w.logw))  # positive, but off every cycle: legal
    assert len(d.best_paths(8)) == 3
    d.set_weights(w.logw)
    kept = d.best_paths_raw(8)
    stats = d.best_paths_stats()
    with pytest.raises(CarmelHipError) as e:
        d.best_paths(0)
    assert e.value.code == ERR_ARG
    after = d._last_paths(np.array([0, 3], np.uint64))[1:]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(kept, after))
    assert d.best_paths_stats() == stats
    d.close()
    # a machine that is refused for its weights: results of a decode() stay, and the handle stays usable
    for name, (wr, arc) in REFUSED.items():
        d = Decoder(wr)
        best, paths = d.decode([[1]])
        for _ in range(2):
            with pytest.raises(CarmelHipError, match=r"arc %d " % arc) as e:
                d.best_paths(3)
            assert e.value.code == ERR_UNSUPPORTED, name
        best2, paths2 = d.decode([[1]])
        assert best.tobytes() == best2.tobytes()
        ok = np.minimum(wr.logw, 0.0)
        d.set_weights(ok)  # the weight above 1 taken away: legal
        assert len(d.best_paths(3)) == 3
        d.set_weights(wr.logw)
        kept = d._last_paths(np.array([0, 3], np.uint64))[1:]
        with pytest.raises(CarmelHipError) as e:
            d.best_paths(3)
        assert e.value.code == ERR_UNSUPPORTED
        after = d._last_paths(np.array([0, 3], np.uint64))[1:]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(kept, after))
        d.close()


def test_error_codes():
    from carmel_amd._capi import lib
    from carmel_amd.decode import Decoder
    import ctypes as C
    d = Decoder(machine("dag3"))
    n = C.c_uint64(77)
    assert lib.carmel_hip_decoder_best_paths(None, 1, C.byref(n)) == ERR_ARG
    assert lib.carmel_hip_decoder_best_paths(d._h, 1, None) == ERR_ARG
    assert lib.carmel_hip_decoder_best_paths(d._h, 0, C.byref(n)) == ERR_ARG
    assert lib.carmel_hip_decoder_best_paths(d._h, 1025, C.byref(n)) == ERR_ARG
    assert n.value == 77
    assert lib.carmel_hip_decoder_best_paths(d._h, 1024, C.byref(n)) == 0 and n.value == 3
    r, s = C.c_uint32(), C.c_uint64()
    assert lib.carmel_hip_decoder_best_paths_stats(d._h, None, C.byref(s)) == ERR_ARG
    assert lib.carmel_hip_decoder_best_paths_stats(None, C.byref(r), C.byref(s)) == ERR_ARG
    assert lib.carmel_hip_decoder_best_paths_stats(d._h, C.byref(r), C.byref(s)) == 0 and r.value >= 2
    d.close()
    # |Q| k >= 2^31: refused before anything is allocated
    big = M(2 ** 21 + 1, 1, [(0, 1, -1.0)])
    d = Decoder(big)
    assert lib.carmel_hip_decoder_best_paths(d._h, 1024, C.byref(n)) == ERR_ARG
    assert lib.carmel_hip_decoder_best_paths(d._h, 1, C.byref(n)) == 0 and n.value == 1
    d.close()
    # the final state out of reach: success with no paths
    d = Decoder(HAND["unreachable"])
    assert d.best_paths(16) == [] and d.best_paths_stats()[0] >= 1
    d.close()
