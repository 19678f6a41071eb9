"""GPU: carmel_hip_compose and carmel_hip_composition_export (csrc/compose.hip) through the C ABI, against the plain product
construction of compose_ref.py, on the corpus of compose_cases.py (what every case is for, and that it gets there, is held on
the CPU in test_compose_ref_host.py).  Everything the kernel computes is exact -- integers and one f64 addition an arc -- so
nothing here has a tolerance: weights are compared by their bits.  The temporary state ids are the one thing the device is free
in (within a level they follow the order in which its atomics land), so every comparison goes through the triple
(qa, qb, filter) a state stands for, never through the id.

Asserted for every case (check()): the counts; temporary state 0 is (0, 0, 0); id -> triple is a bijection onto the reference's
triples with filter <= 2; the reference's BFS depth does not decrease along the ids (levels are contiguous); st_off starts at 0,
does not decrease and ends at n_arcs; and every state's arcs are the reference's, element for element and in order: in, out, the
destination's triple, the bits of logw, ka and kb (0xffffffff where a side took no arc).  The library's own account of the run
(`timing: compose levels= max_frontier= rebuilds= reinserted= state_capacity= table_capacity=`) must be the reference's: the
cases reach the device's internal events -- a second workgroup, a rebuild that reinserts 32 497 states, six doublings of the
state arrays -- only if the device says so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import compose_cases as cc
import compose_ref as cr
from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "carmel_amd", "bin", "carmel")
ERR_ARG = -1


class Export(object):
    pass


def compose(case, threshold=None):
    """-> the handle (a c_void_p) of the composition"""
    from carmel_amd import _capi
    A, B, a2b, n_a2b, b2a, n_b2a = case.arrays()
    h = C.c_void_p()
    rc = _capi.lib.carmel_hip_compose(C.byref(h), 0, case.A.n_states, *([_capi.ptr(x) for x in A] + [case.B.n_states] + [_capi.ptr(x) for x in B] +
                                      [_capi.ptr(a2b), n_a2b, _capi.ptr(b2a), n_b2a, case.threshold if threshold is None else threshold]))
    _capi.check(rc, "carmel_hip_compose")
    assert h.value
    return h, (A, B, a2b, b2a)  # (the arrays stay alive as long as the caller holds them)


FIELDS = (("st_off", np.uint64), ("st_qa", np.uint32), ("st_qb", np.uint32), ("st_f", np.uint8), ("arc_in", np.uint32), ("arc_out", np.uint32),
          ("arc_dst", np.uint32), ("arc_logw", np.float64), ("arc_ka", np.uint32), ("arc_kb", np.uint32))


def export(h, only=None):
    """every array of the composition (or, with `only`, those named: null pointers for the rest); arrays of no element are given
    one, unused, so that the pointer is valid"""
    from carmel_amd import _capi
    E = Export()
    E.n_states, E.n_arcs = int(_capi.lib.carmel_hip_composition_states(h)), int(_capi.lib.carmel_hip_composition_arcs(h))
    args = []
    for name, dt in FIELDS:
        n = E.n_states + 1 if name == "st_off" else E.n_states if name.startswith("st_") else E.n_arcs
        a = np.full(max(n, 1), 0xAB, dt) if only is None or name in only else None
        setattr(E, name, None if a is None else a[:n])
        args.append(_capi.ptr(a) if a is not None else None)
    _capi.check(_capi.lib.carmel_hip_composition_export(h, *args), "carmel_hip_composition_export")
    return E


def free(h):
    from carmel_amd import _capi
    _capi.check(_capi.lib.carmel_hip_composition_free(h), "carmel_hip_composition_free")


def check(case, E, R=None):
    R = R or case.reference()
    assert (E.n_states, E.n_arcs) == (R.n_states, R.n_arcs)
    qa, qb, f = E.st_qa.tolist(), E.st_qb.tolist(), E.st_f.tolist()
    assert (qa[0], qb[0], f[0]) == (0, 0, 0)
    assert max(f) <= 2
    triple = list(zip(qa, qb, f))
    assert len(set(triple)) == len(triple) and set(triple) == set(R.arcs)  # a bijection onto the reference's states
    depth = [R.depth[t] for t in triple]
    assert all(a <= b for a, b in zip(depth, depth[1:]))  # levels are contiguous runs of ids
    off = E.st_off.tolist()
    assert off[0] == 0 and off[-1] == E.n_arcs and all(a <= b for a, b in zip(off, off[1:]))
    assert E.n_arcs == 0 or int(E.arc_dst.max()) < E.n_states
    cols = list(zip(E.arc_in.tolist(), E.arc_out.tolist(), [triple[d] for d in E.arc_dst.tolist()], E.arc_logw.view(np.uint64).tolist(),
                    E.arc_ka.tolist(), E.arc_kb.tolist()))
    for s, t in enumerate(triple):
        want = [a[:3] + (cr.bits(a[3]),) + a[4:] for a in R.arcs[t]]
        got = cols[off[s]:off[s + 1]]
        if got != want:
            k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
            raise AssertionError("%s: state %d = %r: %d arcs for %d; at arc %d the device has %r, the reference %r" % (
                case.name, s, t, len(got), len(want), k, got[k] if k < len(got) else None, want[k] if k < len(want) else None))


def run_case(case, hipopt, capfd, partial=True):
    hipopt.set("timing", "1")
    capfd.readouterr()
    h, keep = compose(case)
    try:
        err = capfd.readouterr().err
        E = export(h)
        check(case, E)
        line = [l for l in err.split("\n") if l.startswith("timing: compose ")]
        print(case.name, "|", line)
        assert line == [case.reference().report.timing_line()]
        if partial:  # export with some of the pointers null: the same values for the rest
            for only in (("st_off", "arc_dst", "arc_kb"), ("st_qa", "st_qb", "st_f"), ("arc_in", "arc_out", "arc_logw", "arc_ka"), ()):
                P = export(h, only)
                for name, _ in FIELDS:
                    got = getattr(P, name)
                    assert (got is None) == (name not in only)
                    if got is not None:
                        assert np.array_equal(got.view(np.uint8), getattr(E, name).view(np.uint8)), name
    finally:
        free(h)
    return E


SMALL = [n for n in cc.NAMES if n != "rebuild"]


@pytest.mark.parametrize("name", SMALL)
def test_case_against_the_product_construction(name, hipopt, capfd):
    run_case(cc.by_name(name), hipopt, capfd)


def test_rebuild_case_twice(hipopt, capfd):
    """40 000 states: one table rebuild that reinserts 32 497 of them, six doublings of the state arrays, and arcs that lead
    back into every earlier level afterwards; a second run (other ids within the levels, maybe) gives the same result by triple"""
    case = cc.by_name("rebuild")
    rep = case.reference().report
    assert max(r[0] for r in rep.rebuilds) >= 30000 and rep.doublings >= 5
    E1 = run_case(case, hipopt, capfd)
    E2 = run_case(case, hipopt, capfd, partial=False)
    assert (E1.n_states, E1.n_arcs) == (E2.n_states, E2.n_arcs) and np.array_equal(E1.st_off[-1:], E2.st_off[-1:])


def test_random_operand_pairs(hipopt, capfd):
    """200 seeded pairs through one library load: 1 to 12 states, up to 40 arcs a state, 1 to 5 symbols on a shuffled symbol
    table, epsilon rates 0 to 0.6, thresholds 0, 1, 2, 5 and 32"""
    hipopt.set("timing", "1")
    for case in cc.random_cases():
        capfd.readouterr()
        h, keep = compose(case)
        try:
            check(case, export(h))
            assert case.reference().report.timing_line() in capfd.readouterr().err.split("\n"), case.name
        finally:
            free(h)


def test_argument_errors_leave_the_handle_alone():
    from carmel_amd import _capi
    case = cc.by_name("frontier-1")
    A, B, a2b, n_a2b, b2a, n_b2a = case.arrays()
    good = [0, case.A.n_states] + [_capi.ptr(x) for x in A] + [case.B.n_states] + [_capi.ptr(x) for x in B] + [_capi.ptr(a2b), n_a2b, _capi.ptr(b2a), n_b2a, 32]
    SENTINEL = 0x5ca1ab1e
    for at, bad in ((2, None), (8, None), (13, None), (15, None), (1, 0), (7, 0)):  # a_off, b_off, a2b, b2a null; no states in A, in B
        h = C.c_void_p(SENTINEL)
        args = list(good)
        args[at] = bad
        assert _capi.lib.carmel_hip_compose(C.byref(h), *args) == ERR_ARG, at
        assert h.value == SENTINEL
        assert b"null argument" in _capi.lib.carmel_hip_last_error()
    assert _capi.lib.carmel_hip_compose(None, *good) == ERR_ARG
    assert _capi.lib.carmel_hip_composition_export(None, *([None] * 10)) == ERR_ARG
    assert _capi.lib.carmel_hip_composition_states(None) == 0 and _capi.lib.carmel_hip_composition_arcs(None) == 0
    assert _capi.lib.carmel_hip_composition_free(None) == 0


def carmel(args, env=None):
    p = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=dict(os.environ, **(env or {})))
    return p.returncode, p.stdout, p.stderr


@pytest.mark.parametrize("name,finals", [("frontier-257", (258, 2)), ("rebuild", (0, 0))])
def test_front_end_prints_the_host_composition(name, finals, tmp_path):
    """the same two cases as text through carmel --gpu-compose: the output of the host composition, at -T 2 and -T 32.  With -d,
    which keeps the front end from reducing the first operand and the result: the operands reach the device as they are written
    (frontier-257 has dead ends on purpose) and every composed arc is printed."""
    case = cc.by_name(name)
    pa, pb = str(tmp_path / "a.fst"), str(tmp_path / "b.fst")
    open(pa, "w").write(cc.to_text(case.A, finals[0]))
    open(pb, "w").write(cc.to_text(case.B, finals[1]))
    for T in ("2", "32"):
        rc_h, out_h, err_h = carmel(["-HJ", "-q", "-d", "-T", T, pa, pb])
        rc_d, out_d, err_d = carmel(["-HJ", "-q", "-d", "-T", T, "--gpu-compose", pa, pb], env={"CARMEL_TIMING": "1"})
        assert rc_h == 0 and rc_d == 0, (err_h, err_d)
        assert out_d == out_h and out_h.count("\n") == case.reference().n_arcs + 1
        if int(T) == case.threshold:
            assert case.reference().report.timing_line() in err_d.split("\n")
