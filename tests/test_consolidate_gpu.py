"""GPU: consolidating duplicate arcs (carmel_hip_consolidate, csrc/consolidate.hip; carmel -C) against the reference of
consolidate_ref.py on the cases of consolidate_cases.py (checked on the CPU by test_consolidate_host.py), every case over the
grid {sum clamped, sum unclamped, max}: n_kept, kept_id and arc_map integer for integer; max mode, single-member segments and
sums clamped to 0 bit for bit; sums within the bound below; the same bytes from two calls, in both forms of the reduction;
rejected inputs; the all-paths sums of a Decoder before and after; duplicate paths among the best paths before, none after.

The bound.  tests/sweep_math_cases.py derives |value - ref| <= (4 d + 4) u + u |ref|, u = 2^-53, for one Lse of d terms.  The lane
form (a segment of at most `consolidate_wave_members` members) is one such Lse.  The wavefront form gives lane l an Lse of its own
over members l, l + 64, ...: by the same derivation a relative error of at most 4 d_l u of its scaled sum, d_l <= d.  Six
shuffle steps then combine two (m, acc) pairs each as acc_hi + acc_lo * exp(m_lo - m_hi).  One step rounds the difference of the
maxima (u |t| e^-|t| <= 0.37 u of the result, the result being at least the larger sum), takes one exponential (1 ulp, at most
2 u), rounds one product (u) and one addition (u): under 5 u of the combined sum, and it leaves the relative errors the two
operands brought as a weighted mean, no larger than the larger of them.  Six steps add 30 u to a value's error, so a segment
summed by a wavefront is held to (4 d + 4 + 30) u + u |ref|.  The largest case, 5 000 members, has a bound of 2.3e-12, under
sweep_ref.CEILING (1e-10): asserted for every segment."""
import ctypes as C

import numpy as np
import pytest

from consolidate_cases import DECODER_SEEDS, DEFAULT_WAVE_MEMBERS, GRID, WAVE_SETTINGS, decoder_case, machine, names, reference
from consolidate_ref import LD, NONE, Consolidated
from sweep_ref import CEILING
from test_decode_sum_gpu import RTOL

pytestmark = pytest.mark.gpu

ERR_ARG = -1
U = 2.0 ** -53
WAVE_STEPS_U = 30.0  # six two-term combine steps, under 5 u each (the docstring above)


def bound(d, ref, by_wavefront):
    return ((4.0 * d + 4.0 + (WAVE_STEPS_U if by_wavefront else 0.0)) * U + U * abs(LD(ref))).astype(LD)


def check_case(name, mode, clamp, wave_members):
    """-> the raw outputs; wave_members: the setting in force (a segment of more members is summed by a wavefront)"""
    from carmel_amd.decode import consolidate_raw
    w = machine(name)
    ref = reference(name, mode, clamp)
    n_kept, kept_id, kept_logw, arc_map, ms = consolidate_raw(w.src, w.dst, w.isym, w.osym, w.logw, mode, clamp)
    where = (name, mode, clamp, wave_members)
    assert n_kept == ref.n_kept, where
    assert kept_id.tolist() == ref.kept_id.tolist(), where
    assert arc_map.tolist() == ref.arc_map.tolist(), where
    worst = 0.0
    for j in range(n_kept):
        got, want, d = kept_logw[j], ref.value[j], int(ref.size[j])
        if ref.exact[j]:  # one member, or max mode: a member's bits
            assert got.tobytes() == np.float64(want).tobytes(), (where, j)
            continue
        b = bound(d, want, d > wave_members)
        assert b < CEILING, (where, j, b)
        if ref.clamp:
            assert got <= 0.0, (where, j, got)
            if want - b > 0:  # a sum above 1 beyond doubt: clamped to 0, bit for bit
                assert got.tobytes() == np.float64(0.0).tobytes(), (where, j, got)
                continue
            want = min(want, LD(0.0))
        err = abs(LD(got) - want)
        worst = max(worst, float(err / b))
        assert err <= b, (where, j, d, float(err), float(b))
    print("consolidate %s %s clamp=%s wave_members=%s: n_kept %d of %d, worst error / bound %.3f, kernels %.3f ms"
          % (name, mode, clamp, wave_members, n_kept, w.n_arcs, worst, ms))
    return kept_id.tobytes() + kept_logw.tobytes() + arc_map.tobytes()


@pytest.mark.parametrize("name", names())
def test_device_equals_the_reference(name):
    for mode, clamp in GRID:
        check_case(name, mode, clamp, DEFAULT_WAVE_MEMBERS)


@pytest.mark.parametrize("setting", WAVE_SETTINGS)
@pytest.mark.parametrize("name", ["sizes", "count10000", "clamp", "random3"])
def test_both_forms_at_every_size_and_the_same_bytes_from_two_calls(name, setting):
    """option consolidate_wave_members at 1 (every segment of two or more members by a wavefront), unset (64) and 2^20 (every
    segment by a lane): each form runs at the sizes 63, 64, 65, 200, 5 000 and is held to its own bound; a second call returns
    the first call's bytes"""
    import carmel_amd
    try:
        carmel_amd.set_option("consolidate_wave_members", setting)
        wave_members = DEFAULT_WAVE_MEMBERS if setting is None else int(setting)
        for mode, clamp in GRID:
            first = check_case(name, mode, clamp, wave_members)
            again = check_case(name, mode, clamp, wave_members)
            assert first == again, (name, mode, clamp, setting)
    finally:
        carmel_amd.set_option("consolidate_wave_members", None)


def test_max_mode_does_not_depend_on_the_form():
    import carmel_amd
    raws = {}
    try:
        for setting in WAVE_SETTINGS:
            carmel_amd.set_option("consolidate_wave_members", setting)
            raws[setting] = check_case("sizes", "max", True, DEFAULT_WAVE_MEMBERS if setting is None else int(setting))
    finally:
        carmel_amd.set_option("consolidate_wave_members", None)
    assert raws["1"] == raws[None] == raws[WAVE_SETTINGS[2]]


def test_rejected_inputs_leave_the_buffers_alone():
    from carmel_amd._capi import lib, ptr
    w = machine("interleaved")
    n = w.n_arcs

    def call(src=w.src, logw=w.logw, mode=0, clamp=1, n_arcs=n, nulls=()):
        arc_map, kept_id, kept_logw, n_kept = np.full(n, 7, np.uint32), np.full(n, 7, np.uint32), np.full(n, 7.0), C.c_uint64(7)
        args = [ptr(np.ascontiguousarray(src, np.uint32)), ptr(w.dst), ptr(w.isym), ptr(w.osym), ptr(np.ascontiguousarray(logw, np.float64))]
        outs = [ptr(arc_map), ptr(kept_id), ptr(kept_logw)]
        for k in nulls:
            (args if k < 5 else outs)[k % 5] = None
        rc = lib.carmel_hip_consolidate(0, n_arcs, *args, mode, clamp, *outs, C.byref(n_kept), None)
        untouched = n_kept.value == 7 and (arc_map == 7).all() and (kept_id == 7).all() and (kept_logw == 7.0).all()
        return rc, untouched

    bad = w.logw.copy()
    bad[3] = np.nan
    assert call(logw=bad) == (ERR_ARG, True)
    bad[3] = np.inf
    assert call(logw=bad) == (ERR_ARG, True)
    unsorted = w.src.copy()
    unsorted[0] = 1
    assert call(src=unsorted) == (ERR_ARG, True)
    assert call(mode=2) == (ERR_ARG, True) and call(clamp=-1) == (ERR_ARG, True)
    assert call(n_arcs=0xFFFFFFFF) == (ERR_ARG, True)
    top = w.src.copy()
    top[-1] = NONE
    assert call(src=top) == (ERR_ARG, True)
    for k in (0, 4, 5, 7):
        assert call(nulls=(k,)) == (ERR_ARG, True)
    assert lib.carmel_hip_consolidate(0, n, *[ptr(a) for a in (w.src, w.dst, w.isym, w.osym, w.logw)], 0, 1, ptr(np.zeros(n, np.uint32)),
                                      ptr(np.zeros(n, np.uint32)), ptr(np.zeros(n)), None, None) == ERR_ARG
    assert call() == (0, False)


def test_entries_from_n_kept_on_are_not_written():
    from carmel_amd._capi import lib, ptr
    w = machine("interleaved")
    n = w.n_arcs
    arc_map, kept_id, kept_logw, n_kept, ms = np.full(n, 7, np.uint32), np.full(n, 7, np.uint32), np.full(n, 7.0), C.c_uint64(7), C.c_double(-1)
    rc = lib.carmel_hip_consolidate(0, n, *[ptr(a) for a in (w.src, w.dst, w.isym, w.osym, w.logw)], 0, 1, ptr(arc_map), ptr(kept_id),
                                    ptr(kept_logw), C.byref(n_kept), C.byref(ms))
    assert rc == 0 and n_kept.value == 2 and (kept_id[2:] == 7).all() and (kept_logw[2:] == 7.0).all() and ms.value > 0.0
    assert kept_id[:2].tolist() == [0, 1] and arc_map.tolist() == [0, 1, 0, 1, 0]


@pytest.mark.parametrize("seed", DECODER_SEEDS)
def test_a_decoder_on_the_consolidated_machine_sums_to_the_same(seed):
    """sum(lines) over ALL paths is what consolidation keeps: three of the random machines, their input epsilons made acyclic
    (consolidate_cases.decoder_case), on side 0, unclamped"""
    from carmel_amd.decode import Decoder, consolidate
    w, lines = decoder_case(seed)
    c, arc_map, _ = consolidate(w, "sum", False)
    ref = Consolidated(w.src, w.dst, w.isym, w.osym, w.logw, "sum", False)
    assert c.n_arcs == ref.n_kept < w.n_arcs and arc_map.tolist() == ref.arc_map.tolist()
    assert (c.group == w.group[ref.kept_id]).all() and (c.src == w.src[ref.kept_id]).all() and (c.osym == w.osym[ref.kept_id]).all()
    d0, d1 = Decoder(w, side=0), Decoder(c, side=0)
    s0, s1 = d0.sum(lines), d1.sum(lines)
    d0.close()
    d1.close()
    assert np.isfinite(s0[:-2]).all() and len(lines) >= 12, (seed, s0)  # the walks' lines have derivations
    for a, b in zip(s0, s1):
        assert (a == -np.inf and b == -np.inf) or abs(a - b) <= RTOL * max(1.0, abs(a)), (seed, a, b)


def test_max_mode_removes_the_duplicate_paths_from_the_best_paths():
    from carmel_amd.decode import Decoder, consolidate
    w = machine("parallel_paths")

    def sequences(m):
        d = Decoder(m)
        best = d.best_paths(8)
        d.close()
        return [tuple((int(m.src[a]), int(m.dst[a]), int(m.isym[a]), int(m.osym[a])) for a in arcs) for _, arcs in best], [v for v, _ in best]

    before, _ = sequences(w)
    assert len(before) == 6 and len(set(before)) == 2  # the original lists paths of equal states and symbols
    c, _, _ = consolidate(w, "max")
    after, values = sequences(c)
    assert len(after) == len(set(after)) == 2 and set(after) == set(before)
    assert values == [float(np.log(0.5) + np.log(0.5)), float(np.log(0.125) + np.log(0.5))]  # each the best of its duplicates
