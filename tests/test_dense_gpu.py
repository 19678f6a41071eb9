"""GPU: the dense cascade sweep (carmel_amd/csrc/dense.hip) and the table-walking unrolled sweep under a cascade
(unrolled.hip), each kernel's own counts and ln p against tests/dense_ref.py in longdouble.

What is read is the sweep's output itself: the first n_slots doubles of the count buffer after one estimate() (slot k =
the k-th unlocked parameter in parameter order, engine_unrolled.cpp), no M-step and no on-demand explicit pass between.
Every comparison is made for the dense layout (2) and again with the option dense=0 (layout 1, unrolled_sweep_kernel<16|32|64>).

Tolerance: dense_ref.tol_rel(S, T_max, N) = 4 (S + 4) T_max u + N u, derived in dense_ref's docstring; relative on every
count above 1e-200 x the total, on ln p relative to max(1, |ln p|).  Counts the reference has as exactly 0 must be exactly 0.
Where a case is expected to keep EXPLICIT lattices (layout 0: beyond the length ceiling, weights that underflow) the sweep
works on logarithms: a stored ln alpha carries u |ln alpha| <= u |ln p|, which is that much RELATIVE error of alpha, so
the same count of operations gives tol_rel x max(1, max |ln p|) there.

Which case runs which kernel (padded size as printed by dense_try_build's `timing:` line, asserted in the first test):
    n_plain  S   padded  kernel                          n_plain  S   padded  kernel
    2        4   4       dense_sweep_kernel<4>           11       13  16      dense_mfma_kernel<1, 1|2>
    3        5   8       dense_sweep_kernel<8>           14       16  16      dense_mfma_kernel<1, 1|2>
    6        8   8       dense_sweep_kernel<8>           15       17  32      dense_mfma_kernel<2, 1|2>
    7        9   12      dense_sweep_kernel<12>          30       32  32      dense_mfma_kernel<2, 1|2>
    10       12  12      dense_sweep_kernel<12>          31       33  -       declined: layout 1
The other families run at S = 9 (vector, 12), S = 13 (matrix cores, 16) and S = 29 (matrix cores, 32).

NOT covered, on purpose: the source switches that no option reaches -- no_mfma = true (and with it the vector
instantiations 16 .. 32), split = false (dense_mfma_kernel<., 0>, PHASE 0), smem = false (dense_sweep_kernel<., true>) and
the debug bits of DenseArgs.

Cases the model cannot express: at S = 9 there are 7 plain states, so "16" and "17" *e*:*e* arcs are not reachable there
(every plain state stopping is run instead); at S = 13 they are made of 6 (5) stopping states and 5 (6) two-arc chains.  A
line without a derivation is added wherever the channel is sparse (with a full channel every symbol is written from
every state).

Findings of this file, in the sources now:
  * A model whose composed arcs underflow a double (A and B entries near 1e-170 each) made both unrolled sweeps return NaN
    (dense: a zero scale) or lose the derivation (table-walking: exp(ln w) = 0).  unrolled_try_build now keeps explicit
    lattices for a model with an arc below e^-700 (test_a_product_that_underflows_on_its_own_keeps_explicit_lattices).
  * Two estimates of one trainer do NOT give the same bits under the unrolled sweeps: the posteriors of a workgroup's
    wavefronts meet in LDS atomics, whose order is not fixed (test_two_estimates_agree).  DESIGN.md said otherwise."""
import ctypes as C
import re

import numpy as np
import pytest

import dense_ref as dr

pytestmark = pytest.mark.gpu

_REFS = {}  # (texts, weights) -> (ln p, counts): a case's reference is computed once for both layouts


class Run(object):
    def close(self):
        self.fb.use_external_counts(0)
        self.fb.close()
        self.buf.free()


class DeviceDoubles(object):
    """n zeroed doubles of device memory for carmel_hip_use_external_counts, as the multi-rank worker attaches a torch tensor.
    The worker imports torch first, in a process of its own; torch's wheel carries a HIP runtime of its own, which finds no
    device once the library's runtime has opened it, and a test in the suite's process cannot promise that order.  So the
    buffer comes from the runtime the library itself is linked against (named by the library's own dependency entry: the
    loader then hands back the instance already in the process)."""
    _hip = None

    @classmethod
    def hip(cls):
        if cls._hip is None:
            import carmel_amd
            name = re.search(rb"libamdhip64\.so[.0-9]*", open(carmel_amd.LIB_PATH, "rb").read()).group(0).decode()
            cls._hip = C.CDLL(name)
        return cls._hip

    def __init__(self, n):
        self.n, self.p = n, C.c_void_p()
        assert self.hip().hipMalloc(C.byref(self.p), C.c_size_t(n * 8)) == 0
        assert self.hip().hipMemset(self.p, 0, C.c_size_t(n * 8)) == 0 and self.hip().hipDeviceSynchronize() == 0

    def read(self):
        out = np.empty(self.n)
        assert self.hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(self.n * 8), 2) == 0  # device to host
        return out

    def free(self):
        if self.p:
            assert self.hip().hipFree(self.p) == 0
            self.p = C.c_void_p()


def open_run(oracle, hipopt, texts, dense=True, norms=None, add=(0.0, 0.0)):
    """the trainer of multirank_worker.build("dense") on `texts`, its count buffer zeroed device memory of our own, and the
    tables that say which (cipher symbol, state) a slot is.

    Slot order: engine_unrolled.cpp numbers the accumulator slots through the parameters in order, one per parameter whose
    group is not the locked one; parameters are the members' arcs in the order of oracle's cascade export.  Which arc of
    a FILE a parameter is comes from composing the texts once more with every weight replaced by the arc's number
    (dense_ref.retag) -- no assumption about the order in which the composer keeps a state's arcs."""
    from carmel_amd._capi import lib
    from carmel_amd.model import NORM_CONDITIONAL, NORM_NONE, Corpus, Wfst
    from carmel_amd.trainer import HipForwardBackward
    lm, ch, co = texts
    r = Run()
    r.texts, r.m = texts, dr.parse_cascade(lm, ch, co)
    hipopt.set("unrolled", "1")
    hipopt.set("dense", None if dense else "0")
    oc = r.oc = oracle.OracleCascade([lm, ch])
    a = oc.composed().arrays()
    r.w = Wfst(a["n_states"], a["final"], a["src"], a["dst"], a["isym"], a["osym"], a["logw"], a["group"])
    ca = oc.corpus(co).arrays()
    c = Corpus(ca["in_off"], ca["in_sym"], ca["out_off"], ca["out_sym"], ca["weight"])
    assert c.n_pairs == len(r.m.seqs)
    r.fb = HipForwardBackward(r.w, c, cascade=oc.as_dict(norms or [NORM_NONE, NORM_CONDITIONAL], list(add)), device=0)
    r.layout = lib.carmel_hip_lattice_layout(r.fb.h)
    r.buf = DeviceDoubles(int(lib.carmel_hip_counts_len(r.fb.h)))
    r.fb.use_external_counts(r.buf.p.value)
    tag = np.rint(np.exp(oracle.OracleCascade(list(dr.retag(lm, ch))).param_logw)).astype(np.int64) - 1
    unlocked = oc.param_group != 0  # CARMEL_HIP_LOCKED_GROUP
    assert (unlocked == (oc.param_member == 1)).all() and len(tag) == oc.n_params == r.m.n_lm_arcs + r.m.n_ch_arcs
    r.slot_param = np.nonzero(unlocked)[0]
    r.lm_param, r.ch_param = np.full(r.m.n_lm_arcs, -1), np.full(r.m.n_ch_arcs, -1)
    for p in range(oc.n_params):
        (r.ch_param if unlocked[p] else r.lm_param)[tag[p]] = p
    assert (r.lm_param >= 0).all() and (r.ch_param >= 0).all()
    where = {int(k): cs for cs, k in np.ndenumerate(r.m.b_arc) if k >= 0}
    r.slot_cs = np.array([where[int(tag[p])] for p in r.slot_param])
    return r


def reference(r):
    """dense_ref.dense_reference in longdouble at the weights the trainer holds now (carmel_hip_get_weights: natural logs)"""
    lw = r.fb.weights()
    key = (r.texts, lw.tobytes())
    if key not in _REFS:
        m = r.m
        e = np.exp(lw.astype(np.longdouble))
        A, B = np.zeros(m.A.shape, np.longdouble), np.zeros(m.B.shape, np.longdouble)
        A[m.a_arc >= 0] = e[r.lm_param[m.a_arc[m.a_arc >= 0]]]
        B[m.b_arc >= 0] = e[r.ch_param[m.b_arc[m.b_arc >= 0]]]
        eps = [(s, d, e[r.lm_param[k]]) for s, d, _, k in m.eps]
        _REFS[key] = dr.dense_reference(A, B, m.start, m.fin, eps, m.seqs, m.weights)
    return _REFS[key]


def slot_counts(r):
    """the sweep's counts per accumulator slot: the head of the count buffer under the unrolled layouts; under explicit
    lattices the buffer holds one count per composed arc, summed here per parameter through the arcs' chains"""
    r.fb.synchronize()
    buf = r.buf.read()
    if r.layout:
        return buf[:len(r.slot_param)]
    per_param = np.zeros(r.oc.n_params, np.longdouble)
    off, par = r.oc.chain_off.astype(np.int64), r.oc.chain_param.astype(np.int64)
    for a, g in enumerate(r.w.group):
        per_param[par[off[g]:off[g + 1]]] += buf[a]
    return per_param[r.slot_param]


def check(r, family):
    """one estimate, then ln p and the counts against the reference; prints the figures before it asserts"""
    m = r.m
    r.fb.estimate(per_pair=True)
    lnp, cnt = reference(r)
    live = np.isfinite(lnp.astype(np.float64))
    assert live.any() and ((r.fb.has_deriv > 0) == live).all()
    t_max = max(len(s) for s, ok in zip(m.seqs, live) if ok)
    n_pos = sum(len(s) for s, ok in zip(m.seqs, live) if ok)
    tol = dr.tol_rel(m.S, t_max, n_pos)
    if r.layout == 0:
        tol *= max(1.0, float(np.abs(lnp[live]).max()))
    e_lnp = dr.compare_lnp(r.fb.pair_logprob, lnp)
    e_cnt = dr.compare_counts(slot_counts(r), cnt[r.slot_cs[:, 0], r.slot_cs[:, 1]])
    print("dense-test family=%s layout=%d S=%d V=%d lines=%d t_max=%d err_lnp=%.3g err_counts=%.3g tol=%.3g"
          % (family, r.layout, m.S, m.V, len(m.seqs), t_max, e_lnp, e_cnt, tol))
    assert e_lnp <= tol and e_cnt <= tol
    return lnp, cnt


def lens_mixed(n, lo, hi, seed):
    """n lengths in lo .. hi with both ends present"""
    x = [int(v) for v in np.random.default_rng(seed).integers(lo, hi + 1, n)]
    x[0] = lo
    if n > 1:
        x[-1] = hi
    return x


PADDED = {2: 4, 3: 8, 6: 8, 7: 12, 10: 12, 11: 16, 14: 16, 15: 32, 30: 32, 31: None}


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("n_plain", sorted(PADDED))
def test_every_kernel_size_and_both_sides_of_every_padding_step(oracle, hipopt, capfd, n_plain, dense):
    hipopt.set("timing", "1")
    r = open_run(oracle, hipopt, dr.make_cascade(n_plain, n_plain + 3, 70, lens_mixed(70, 1, 25, n_plain), n_plain), dense)
    trace = capfd.readouterr().err
    hipopt.set("timing", None)
    sp = PADDED[n_plain]
    assert r.layout == (2 if dense and sp else 1)
    line = re.search(r"timing: dense sweep S=(\d+) padded=(\d+)", trace)
    if r.layout == 2:
        assert line and (int(line.group(1)), int(line.group(2))) == (n_plain + 2, sp)
    else:
        assert line is None
    check(r, "sizes")
    r.close()


def lane_lens(n, ragged):
    if not ragged:
        return [7] * n
    return ([300, 1] + lens_mixed(max(n - 2, 1), 2, 40, n))[:n]


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("n_lines", [1, 16, 17, 64, 65, 130])
@pytest.mark.parametrize("S", [13, 9])
def test_lane_and_wavefront_occupancy(oracle, hipopt, S, n_lines, ragged, dense):
    """S = 13: 16 strings per wavefront, four wavefronts per group of 64; S = 9: a string per lane.  Full and partly filled
    tiles, wavefronts and groups; equal lengths, and one string of 300 beside one of 1"""
    r = open_run(oracle, hipopt, dr.make_cascade(S - 2, S + 1, n_lines, lane_lens(n_lines, ragged), 1000 + n_lines), dense)
    assert r.layout == (2 if dense else 1)
    check(r, "lanes")
    r.close()


def eps_case(S, variant):
    """(n_plain, generator arguments, dense eligible)"""
    if variant == "chain":
        return S - 3, dict(eps_chain=True), True
    if variant in ("1", "5"):
        return S - 2, dict(stop_states=int(variant)), True
    if S == 29:
        return 27, dict(stop_states=int(variant)), variant == "16"
    if S == 13:  # 6 stops + 5 chains of two = 16 arcs; 5 stops + 6 chains = 17
        return (6, dict(stop_states=6, eps_chain=5), True) if variant == "16" else (5, dict(stop_states=5, eps_chain=6), False)
    return S - 2, dict(stop_states=S - 2), True  # S = 9, "all": every plain state stops


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("S,variant", [(S, v) for S in (9, 13, 29) for v in ("1", "5", "16", "17", "chain")
                                       if S != 9 or v not in ("16", "17")] + [(9, "all")])
def test_epsilon_arcs(oracle, hipopt, S, variant, dense):
    """one, five, sixteen (the limit) and seventeen (declined) *e*:*e* arcs; a chain p -> X -> END whose topological order is
    neither the states' nor the file's"""
    n_plain, kw, eligible = eps_case(S, variant)
    r = open_run(oracle, hipopt, dr.make_cascade(n_plain, n_plain + 3, 40, lens_mixed(40, 1, 25, S), 2000 + S, **kw), dense)
    assert r.m.S == S
    if variant in ("16", "17"):
        assert len(r.m.eps) == int(variant)
    assert r.layout == (2 if dense and eligible else 1)
    check(r, "epsilon")
    r.close()


def with_dead_line(texts):
    """texts with one more line, at the front, that has no derivation although all its symbols are the channel's: the
    prefix of a line, then a symbol that no state reachable there writes (failing that, that no state which can stop
    there writes).  None when the cascade has no such line."""
    lm, ch, co = texts
    m = dr.parse_cascade(lm, ch, co)
    eps = [e[:3] for e in m.eps]
    A, B = m.A > 0, m.B > 0
    for seq in m.seqs[:10]:
        for k in range(min(len(seq), 4)):
            reach = np.zeros(m.S, bool)
            reach[m.start] = True
            for c in seq[:k]:
                reach = (reach @ A) & B[c]
            nxt = reach @ A
            forward_dead = [c for c in range(m.V) if not (nxt & B[c]).any()]
            cands = [list(seq[:k]) + [c] for c in forward_dead] or [list(seq[:k]) + [c] for c in range(m.V)]
            for cand in cands:
                if np.isneginf(dr.dense_reference(m.A, m.B, m.start, m.fin, eps, [cand], [1.0])[0][0]):
                    return lm, ch, dr.corpus_text([cand], [1.5], m.cipher_names) + co
    return None


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("a,b", [(0.3, 1.0), (1.0, 0.4), (0.3, 0.4)])
@pytest.mark.parametrize("S", [13, 29])
def test_sparse_language_model_and_channel(oracle, hipopt, S, a, b, dense):
    texts = dr.make_cascade(S - 2, S + 1, 40, lens_mixed(40, 1, 25, S), 3000 + S, stop_states=2, a_density=a, b_density=b)
    dead = with_dead_line(texts) if b < 1 else None
    assert (dead is not None) == (b < 1)
    r = open_run(oracle, hipopt, dead or texts, dense)
    assert r.layout == (2 if dense else 1)
    n_plain = S - 2
    assert ((r.m.a_arc >= 0).sum() < n_plain + n_plain * n_plain) == (a < 1) and (r.m.n_ch_arcs < n_plain * (S + 1)) == (b < 1)
    lnp, _ = check(r, "sparsity")
    if dead:
        assert np.isneginf(lnp[0]) and r.fb.has_deriv[0] == 0 and np.isneginf(r.fb.pair_logprob[0])
        assert (r.fb.has_deriv[1:] == 1).all()
    r.close()


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("n_plain,n_cipher", [(11, 1), (11, 4), (7, 3), (3, 150), (11, 60)])
def test_alphabet_sizes(oracle, hipopt, n_plain, n_cipher, dense):
    r = open_run(oracle, hipopt, dr.make_cascade(n_plain, n_cipher, 40, lens_mixed(40, 1, 25, n_cipher), 4000 + n_cipher), dense)
    assert r.m.V == n_cipher and r.layout == (2 if dense else 1)
    check(r, "alphabet")
    r.close()


@pytest.mark.parametrize("over", [0, 1])
def test_both_sides_of_the_lds_ceiling_at_32_states(oracle, hipopt, over):
    """the largest V with V * 32 * 10 + 30 V * 8 <= 60 KB runs dense, one symbol more runs the table-walking sweep"""
    V = dr.dense_max_symbols(32, 30)
    assert V * 32 * 10 + 30 * V * 8 <= 61440 < (V + 1) * 32 * 10 + 30 * (V + 1) * 8
    r = open_run(oracle, hipopt, dr.make_cascade(30, V + over, 70, lens_mixed(70, 1, 25, over), 4500 + over))
    assert r.m.S == 32 and r.m.V == V + over and len(r.slot_param) == 30 * (V + over)
    assert r.layout == (1 if over else 2)
    check(r, "lds-ceiling")
    r.close()


@pytest.mark.parametrize("S,over,dense", [(13, 0, True), (13, 0, False), (13, 1, True), (29, 0, True), (29, 0, False), (29, 1, True)])
def test_both_sides_of_the_length_ceiling(oracle, hipopt, S, over, dense):
    """the longest string unrolled_waves() admits (2007 symbols at S = 13, 3689 at S = 29; ln p near -10^4) and one symbol
    more, which keeps explicit lattices"""
    texts, L = dr.length_case(S, over)
    n_slots = (S - 2) * (S + 1)
    per_wave = 4 if S <= 16 else 2
    assert (n_slots + per_wave * (L - over + 2)) * 8 <= 65536 < (n_slots + per_wave * (L - over + 3)) * 8
    r = open_run(oracle, hipopt, texts, dense)
    assert max(len(s) for s in r.m.seqs) == L
    assert r.layout == (0 if over else 2 if dense else 1)
    lnp, _ = check(r, "length")
    assert float(lnp.min()) < -5000
    r.close()


@pytest.mark.parametrize("dense", [True, False])
def test_dynamic_range_of_a_long_string(oracle, hipopt, dense):
    """an un-normalised language model near 1e-60 per arc (NORM_NONE) under a channel written near 1e-30 and normalised by
    group: 200 positions of about 1e-61 each would underflow an unscaled product thirty times over"""
    lens = [200, 150, 1] + lens_mixed(17, 2, 60, 5)
    r = open_run(oracle, hipopt, dr.make_cascade(11, 14, 20, lens, 5000, lm_scale=1e-60, channel_scale=1e-30), dense)
    assert r.layout == (2 if dense else 1) and 0 < r.m.A[r.m.A > 0].max() < 1e-60
    lnp, _ = check(r, "range")
    assert float(lnp.min()) < -200 * np.log(1e60)
    r.close()


@pytest.mark.parametrize("dense", [True, False])
def test_a_product_that_underflows_on_its_own_keeps_explicit_lattices(oracle, hipopt, dense):
    """language model and channel near 1e-170 per arc, neither normalised: every composed arc is near 1e-340, below the
    smallest double.  In the linear domain the dense sweep's scale of a position is 0 (NaN everywhere) and the
    table-walking sweep's weights are all 0; explicit lattices hold ln w and are right.  The model must keep them."""
    from carmel_amd.model import NORM_NONE
    texts = dr.make_cascade(11, 14, 12, lens_mixed(12, 1, 9, 6), 6000, lm_scale=1e-170, channel_scale=1e-170)
    r = open_run(oracle, hipopt, texts, dense, norms=[NORM_NONE, NORM_NONE])
    assert 0 < r.m.A[r.m.A > 0].max() < 1e-170 and 0 < r.m.B[r.m.B > 0].max() < 1e-170
    assert r.layout == 0
    check(r, "underflow")
    r.close()


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("S", [13, 9])
def test_tables_are_refreshed_between_iterations(oracle, hipopt, S, dense):
    """estimate, maximize, estimate: the second E-step runs on A and B as dense_tables_kernel rebuilt them, parameters
    the M-step drove to exactly 0 included (few short lines: some cipher symbols never occur)"""
    r = open_run(oracle, hipopt, dr.make_cascade(S - 2, S + 1, 8, [1, 2, 3, 4, 5, 6, 6, 3], 7000 + S), dense)
    assert r.layout == (2 if dense else 1)
    check(r, "refresh-1")
    before = r.fb.weights()
    r.fb.maximize(1.0)
    after = r.fb.weights()
    assert np.isneginf(after).any() and not np.isneginf(before).any()
    assert (after[r.lm_param] == before[r.lm_param]).all() and (after[r.ch_param] != before[r.ch_param]).any()
    check(r, "refresh-2")
    r.close()


@pytest.mark.parametrize("dense", [True, False])
def test_absolute_scale_of_the_counts_shows_under_smoothing(oracle, hipopt, dense):
    """with add_count k the trained channel is (count + k) / (sum + n k) per plain symbol: a common factor on the counts no
    longer cancels.  (A cascade's add_count is a member's, given to carmel_hip_set_cascade: carmel_hip_set_norm refuses
    cascades.)  Bound: numerator and denominator are sums of non-negative terms each within tol_rel, so the quotient is
    within 2 tol_rel; ln and exp of a weight above 1e-4 add less than 16 u."""
    k = 0.5
    r = open_run(oracle, hipopt, dr.make_cascade(11, 14, 30, lens_mixed(30, 1, 25, 8), 8000), dense, add=(0.0, k))
    assert r.layout == (2 if dense else 1)
    _, cnt = check(r, "scale")
    r.fb.maximize(1.0)
    got = np.exp(r.fb.weights()[r.slot_param].astype(np.longdouble))
    m = r.m
    c = cnt[r.slot_cs[:, 0], r.slot_cs[:, 1]]
    want = np.zeros(len(c), np.longdouble)
    for s in set(r.slot_cs[:, 1]):
        g = r.slot_cs[:, 1] == s
        want[g] = (c[g] + k) / (c[g].sum() + g.sum() * k)
    tol = 2 * dr.tol_rel(m.S, max(len(q) for q in m.seqs), sum(len(q) for q in m.seqs)) + 16 * dr.U
    err = float((np.abs(got - want) / want).max())
    print("dense-test family=scale-weights layout=%d S=%d err=%.3g tol=%.3g" % (r.layout, m.S, err, tol))
    assert want.min() > 1e-4 and err <= tol
    r.close()


@pytest.mark.parametrize("dense", [True, False])
def test_two_estimates_agree(oracle, hipopt, dense):
    """Two E-steps of one trainer at S = 13 with 130 lines.  The posteriors of the four (dense) or up to eight (table-walking)
    wavefronts of a workgroup are added with LDS atomics, in the order the wavefronts happen to arrive: the sums are not
    bit-reproducible from run to run, and on the MI355X they were seen to differ in the last bits.  What holds is the bound of
    every other test: two runs are each within tol_rel of the exact result, so within 2 tol_rel of each other; ln p, which no
    atomic touches, is the same to the bit."""
    r = open_run(oracle, hipopt, dr.make_cascade(11, 14, 130, lens_mixed(130, 1, 40, 9), 9000), dense)
    assert r.layout == (2 if dense else 1)
    check(r, "repeat-1")
    c1, l1 = slot_counts(r), r.fb.pair_logprob.copy()
    check(r, "repeat-2")
    c2, l2 = slot_counts(r), r.fb.pair_logprob.copy()
    same = bool((c1.view(np.uint64) == c2.view(np.uint64)).all())
    tol = dr.tol_rel(r.m.S, 40, sum(len(q) for q in r.m.seqs))
    err = float((np.abs(c1 - c2) / np.maximum(c1, 1e-300)).max())
    print("dense-test family=repeat-bits layout=%d identical=%s err=%.3g tol=%.3g" % (r.layout, same, err, 2 * tol))
    assert (l1.view(np.uint64) == l2.view(np.uint64)).all()
    assert err <= 2 * tol
    r.close()
