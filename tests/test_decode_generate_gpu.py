"""GPU: batch generation (carmel_hip_decoder_generate, csrc/decode_generate.hip; carmel -G / -g) against the reference of
decode_generate_ref.py on the workload of decode_generate_cases.py (both proved on the CPU by test_decode_generate_host.py): arc
ids, attempts and reported weights, path for path and bit for bit; the path counts around the wavefront and workgroup sizes; a
stream cut into calls; the same bytes under a tiny chunk budget and across runs; set_weights; the cap on a path's arcs; the
errors; the device's frequencies against the exact enumerator; the generated pairs under the pair decoders; the front end."""
import numpy as np
import pytest

from decode_generate_cases import (HAND, MODES, N_FREQ, N_PATHS, SEED, SEED_FREQ, TRIES, UNREACHABLE, check_frequencies, exact,
                                   frequency_cases, machine, model, names, reference)
from decode_generate_ref import CONDITIONAL, JOINT, Machine, frequencies, generate, path_order_weight, reported_weight
from decode_ref import decode_expected, golden_file
from test_decode_gpu import run
from test_decode_host import noe

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3
BIG = "random0"  # the machine of the size, split, chunk and run tests: 38 accepted paths within 4 arcs, both modes retry


def split_raw(raw):
    """generate_raw's arrays -> ([arc ids], weights as bytes, tries)"""
    logw, path_off, arcs, tries = raw
    return ([[int(a) for a in arcs[int(path_off[p]):int(path_off[p + 1])]] for p in range(len(logw))], logw.tobytes(),
            [int(t) for t in tries])


def check_against_reference(m, raw, ref_paths, ref_tries, where):
    paths, weights, tries = split_raw(raw)
    assert paths == ref_paths, (where, next(p for p in range(len(paths)) if paths[p] != ref_paths[p]))
    assert tries == ref_tries, where
    assert weights == np.array([reported_weight(m, p) for p in ref_paths]).tobytes(), where  # bit for bit
    assert all(m.logw[k] > -np.inf for p in paths for k in p), where  # no zero-weight arc ever appears


@pytest.mark.parametrize("name", names())
def test_device_equals_the_reference(name):
    from carmel_amd.decode import Decoder
    w, L, side = machine(name)
    d = Decoder(w, side=side)
    n_modes = 0
    for mode in MODES:
        ref = reference(name, mode)
        if ref is None:  # (some path of the workload fails within TRIES attempts: test_unreachable_final_state has that case)
            continue
        check_against_reference(model(name), d.generate_raw(N_PATHS, mode, SEED, L, TRIES), ref[0], ref[1], (name, mode))
        n_modes += 1
    d.close()
    assert n_modes or name not in HAND


@pytest.fixture(scope="module")
def big_reference():
    """4000 paths of BIG in both modes, computed once: a path depends on its index alone, so every shorter call is a prefix"""
    return {mode: generate(model(BIG), mode, 4000, 31, 4, TRIES)[:2] for mode in MODES}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4000])
def test_path_counts_around_the_wavefront_and_the_workgroup(big_reference, n):
    from carmel_amd.decode import Decoder
    d = Decoder(machine(BIG)[0])
    for mode in MODES:
        paths, tries = big_reference[mode]
        assert all(p is not None for p in paths)
        check_against_reference(model(BIG), d.generate_raw(n, mode, 31, 4, TRIES), paths[:n], tries[:n], (mode, n))
    d.close()


def test_a_stream_cut_into_calls_chunks_and_runs(big_reference, hipopt):
    """one call equals two calls split by first_path; a tiny decode_chunk_bytes (every path's writing pass alone) and a second
    run give the same bytes; another seed does not"""
    from carmel_amd.decode import Decoder
    d = Decoder(machine(BIG)[0])
    for mode in MODES:
        paths, tries = big_reference[mode]
        whole = d.generate_raw(257, mode, 31, 4, TRIES)
        head, tail = d.generate_raw(100, mode, 31, 4, TRIES), d.generate_raw(157, mode, 31, 4, TRIES, first=100)
        assert split_raw(head)[0] + split_raw(tail)[0] == split_raw(whole)[0] == paths[:257]
        assert split_raw(head)[1] + split_raw(tail)[1] == split_raw(whole)[1]
        assert split_raw(head)[2] + split_raw(tail)[2] == split_raw(whole)[2] == tries[:257]
        hipopt.set("decode_chunk_bytes", "8")
        chunked = d.generate_raw(257, mode, 31, 4, TRIES)
        hipopt.unset("decode_chunk_bytes")
        again, other = d.generate_raw(257, mode, 31, 4, TRIES), d.generate_raw(257, mode, 32, 4, TRIES)
        same = lambda a, b: all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        assert same(whole, chunked) and same(whole, again) and not same(whole, other)
        assert d.last_ms() > 0
    assert d.generate(0) == [] and d.generate_raw(0)[1].tolist() == [0]  # n_paths = 0 succeeds with no paths
    d.close()


def test_set_weights_rebuilds_the_tables():
    """after set_weights the paths are those of a fresh handle with those weights, and the reference's"""
    from carmel_amd.decode import Decoder
    from carmel_amd.model import Wfst
    w, L, _ = machine("random5")
    rng = np.random.default_rng(3)
    logw2 = np.log(rng.uniform(0.05, 1.0, w.n_arcs))
    logw2[rng.uniform(size=w.n_arcs) < 0.1] = -np.inf
    w2 = Wfst(w.n_states, w.final, w.src, w.dst, w.isym, w.osym, logw2)
    d, fresh = Decoder(w), Decoder(w2)
    for mode in MODES:
        before = d.generate_raw(300, mode, 5, L, 256)
        want = fresh.generate_raw(300, mode, 5, L, 256)
        d.set_weights(logw2)
        got = d.generate_raw(300, mode, 5, L, 256)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
        assert split_raw(got)[0] != split_raw(before)[0]
        m2 = Machine(w2.n_states, w2.final, w2.src, w2.dst, w2.isym, w2.logw)
        ref = generate(m2, mode, 300, 5, L, 256)
        check_against_reference(m2, got, ref[0], ref[1], mode)
        d.set_weights(w.logw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(d.generate_raw(300, mode, 5, L, 256), before))
    d.close()
    fresh.close()


def test_exactly_max_arcs_is_accepted_and_one_more_never():
    from carmel_amd._capi import CarmelHipError
    from carmel_amd.decode import Decoder
    w, L, _ = machine("exactly_L")
    d = Decoder(w)
    for mode in MODES:
        got = d.generate(500, mode, 9, L, TRIES)
        assert {tuple(p) for _, p in got} == {(0, 1, 2, 3)} and len(got) == 500  # the road of L + 1 arcs is drawn and rejected
        assert any(t > 1 for t in d.generate_raw(500, mode, 9, L, TRIES)[3])
        assert {tuple(p) for _, p in d.generate(500, mode, 9, L + 1, TRIES)} == {(0, 1, 2, 3), (0, 1, 2, 4, 5)}
        with pytest.raises(CarmelHipError) as e:
            d.generate(5, mode, 9, L - 1, 8)
        assert e.value.code == ERR_STATE
    d.close()


def test_unreachable_final_state_fails_and_keeps_the_previous_results():
    from carmel_amd._capi import CarmelHipError
    from carmel_amd.decode import Decoder
    d = Decoder(UNREACHABLE)
    with pytest.raises(CarmelHipError, match=r"path 17 .*16 attempts.*12 arcs") as e:
        d.generate(40, JOINT, 1, 12, 16, first=17)
    assert e.value.code == ERR_STATE
    d.close()
    # on a machine where only some paths fail the lowest failed P is named, and the handle keeps its previous results
    w, L, _ = machine("dead_end")
    m = model("dead_end")
    d = Decoder(w)
    ok = d.generate_raw(50, JOINT, 4, L, TRIES)
    kept = d._last_paths(np.array([0, 50], np.uint64))
    ref_paths, _, _, _ = generate(m, JOINT, 200, 4, L, 1, first=1000)  # one attempt: half of the paths fail
    lowest = 1000 + next(p for p, path in enumerate(ref_paths) if path is None)
    with pytest.raises(CarmelHipError, match=r"path %d " % lowest) as e:
        d.generate_raw(200, JOINT, 4, L, 1, first=1000)
    assert e.value.code == ERR_STATE
    after = d._last_paths(np.array([0, 50], np.uint64))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(kept, after))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ok, d.generate_raw(50, JOINT, 4, L, TRIES)))  # and stays usable
    d.close()


def test_argument_errors():
    from carmel_amd._capi import CarmelHipError, lib, ptr
    from carmel_amd.decode import Decoder
    d = Decoder(machine("loop_and_exit")[0])
    tries = np.zeros(8, np.uint32)
    call = lambda h, mode, n, first, arcs, tr: lib.carmel_hip_decoder_generate(h, mode, n, first, 0, arcs, tr, ptr(tries))
    assert call(None, 0, 1, 0, 10, 10) == ERR_ARG
    assert call(d._h, 2, 1, 0, 10, 10) == ERR_ARG and call(d._h, -1, 1, 0, 10, 10) == ERR_ARG
    assert call(d._h, 0, 2, 2 ** 32 - 1, 10, 10) == ERR_ARG and call(d._h, 0, 2 ** 32 + 1, 0, 10, 10) == ERR_ARG
    assert call(d._h, 0, 1, 2 ** 64 - 1, 10, 10) == ERR_ARG
    assert call(d._h, 0, 1, 0, 0, 10) == ERR_ARG and call(d._h, 0, 1, 0, 2 ** 20 + 1, 1) == ERR_ARG
    assert call(d._h, 0, 1, 0, 10, 0) == ERR_ARG and call(d._h, 0, 1, 0, 10, 65537) == ERR_ARG
    assert call(d._h, 0, 1, 0, 2 ** 20, 17) == ERR_ARG  # the product
    assert call(d._h, 0, 1, 2 ** 32 - 1, 2 ** 20, 16) == 0 and tries[0] >= 1  # the limits themselves are legal
    assert call(d._h, 1, 8, 2 ** 32 - 8, 10, 10) == 0 and all(t >= 1 for t in tries)
    assert lib.carmel_hip_decoder_generate(d._h, 0, 8, 0, 0, 10, 10, None) == 0  # tries is nullable
    with pytest.raises(KeyError):
        d.generate(1, mode="neither")
    with pytest.raises(CarmelHipError):
        d.generate(1, max_tries=0)
    d.close()


FREQ_ON_DEVICE = [c for c in frequency_cases() if c[0] in ("loop_and_exit", "dead_end", "groups", "epsilon_cycle", "random0", "random5")]


@pytest.mark.parametrize("name,mode", FREQ_ON_DEVICE)
def test_device_frequencies_against_the_enumerator(name, mode):
    from carmel_amd.decode import Decoder
    L, dist, accept = exact(name, mode)
    w, _, side = machine(name)
    d = Decoder(w, side=side)
    paths, _, tries = split_raw(d.generate_raw(N_FREQ, mode, SEED_FREQ + 1, L, TRIES))
    d.close()
    worst = check_frequencies(frequencies(paths), dist, N_FREQ, (name, mode))
    mean, se = sum(tries) / float(N_FREQ), np.sqrt((1.0 - accept) / accept ** 2 / N_FREQ)
    print("%s %s: worst |f - p| %.2f of the bound's unit; mean attempts %.4f against %.4f" % (name, mode, worst, mean, 1.0 / accept))
    assert abs(mean - 1.0 / accept) <= 5.0 * se + 1e-9


def has_00_cycle(w):
    """the arcs of weight > 0 with epsilon on both sides have a cycle"""
    nxt = {}
    for k in range(w.n_arcs):
        if w.isym[k] == 0 and w.osym[k] == 0 and w.logw[k] > -np.inf:
            nxt.setdefault(int(w.src[k]), set()).add(int(w.dst[k]))
    state = {}

    def go(q):
        state[q] = 1
        for r in nxt.get(q, ()):
            if state.get(r) == 1 or (r not in state and go(r)):
                return True
        state[q] = 2
        return False

    return any(q not in state and go(q) for q in list(nxt))


def test_generated_pairs_under_the_pair_decoders():
    """on the machines without a 00 cycle: every generated pair has a finite sum_pairs, which is >= the path's path-order weight
    within the pair-sum tests' tolerance (1e-10 max(1, |v|)), and decode_pairs' best is >= it likewise"""
    from carmel_amd.decode import Decoder
    n_pairs = n_machines = 0
    for name in names():
        w, L, side = machine(name)
        if has_00_cycle(w) or reference(name, CONDITIONAL) is None:
            continue
        m = model(name)
        d = Decoder(w, side=side)
        got = d.generate(60, CONDITIONAL, 13, L, TRIES)
        assert d.generate_pairs(60, CONDITIONAL, 13, L, TRIES) == [([int(w.isym[a]) for a in p if w.isym[a]],
                                                                    [int(w.osym[a]) for a in p if w.osym[a]]) for _, p in got]
        msym, other = (w.osym, w.isym) if side else (w.isym, w.osym)
        xs = [[int(msym[a]) for a in p if msym[a]] for _, p in got]
        ys = [[int(other[a]) for a in p if other[a]] for _, p in got]
        sums = d.sum_pairs(xs, ys)
        best, _ = d.decode_pairs(xs, ys)
        d.close()
        for (_, p), s, b in zip(got, sums, best):
            v = path_order_weight(m, p)
            tol = 1e-10 * max(1.0, abs(v))
            assert np.isfinite(s) and s >= v - tol and b >= v - tol and s >= b - tol, (name, p, v, s, b)
        n_pairs += len(got)
        n_machines += 1
    assert n_machines >= 30 and n_pairs >= 1800, (n_machines, n_pairs)
    assert has_00_cycle(machine("cycle_00")[0]) and not has_00_cycle(machine("epsilon_cycle")[0])


def scored(pairs_file, text, members):
    """carmel -S over the printed pairs -> their probabilities"""
    pairs_file.write_text(text)
    rc, out, err = run(["-S", "-q", str(pairs_file)] + members)
    assert rc == 0, err
    return [float(x) for x in out.split()]


def test_front_end_generates_from_the_cluster_machines(golden_dir, tmp_path):
    """the composition of the cluster machines has its start state final, so every walk stops where it starts: 50 empty pairs"""
    members = [golden_file(golden_dir, m, tmp_path) for m in ("cat.fsa.trained.noe", "spellout.fst.trained")]
    rc, out, err = run(["-q", "--generate-pairs=50", "-R", "7"] + members, env={"CARMEL_TIMING": "1"})
    assert rc == 0, err
    assert "timing: generate " in err
    assert len(out.split("\n")) == 101 and out.endswith("\n")
    rc2, out2, _ = run(["-q", "--generate-pairs=50", "-R", "7"] + members)
    assert rc2 == 0 and out2 == out
    # carmel -S scores every printed pair.  It refuses a corpus in which no lattice has an arc ("no arc in any lattice"), which 50
    # empty pairs are, so the corpus ends with one pair more: the first line of the tutorial's data with its recorded best path
    gold = decode_expected(golden_dir)["cluster"]
    known = "%s\n%s\n" % (gold["paths"][0], noe(golden_dir, gold["data"])[0])
    probs = scored(tmp_path / "generated.pairs", out + known, members)
    assert len(probs) == 51 and all(np.isfinite(p) and p > 0 for p in probs), probs
    rc, out_at, err = run(["-q@", "--generate-paths=50", "-R", "7"] + members)
    assert rc == 0 and len(out_at.split("\n")) == 101, err
    probs = scored(tmp_path / "generated.pairs", out_at + known, members)
    assert len(probs) == 51 and all(np.isfinite(p) and p > 0 for p in probs), probs
    rc, out_o, err = run(["-qOWE", "--generate-paths=50", "-R", "7"] + members)
    assert rc == 0 and len(out_o.split("\n")) == 51, err


def test_front_end_generates_paths_and_pairs_that_score(tmp_path):
    """a machine whose walks are not empty: a loop, an epsilon on either side, two ways out"""
    m = tmp_path / "gen.fst"
    m.write_text("F\n(S (A a x 0.5) (A b y 0.5))\n(A (A c z 0.4) (F d *e* 0.3) (F *e* w 0.3))\n")
    members = [str(m)]
    rc, out, err = run(["-q", "--generate-pairs=50", "-R", "7"] + members)
    assert rc == 0, err
    lines = out.split("\n")
    assert len(lines) == 101 and lines[-1] == "" and "*e*" not in out
    assert all(l.split(" ")[0] in ("a", "b") for l in lines[0:100:2]) and all(set(l.split()) <= {"x", "y", "z", "w"} for l in lines[1:100:2])
    assert len(set(lines[0:100:2])) > 1
    rc2, out2, _ = run(["-q", "--generate-pairs=50", "-R", "7"] + members)
    rc8, out8, _ = run(["-q", "--generate-pairs=50", "-R", "8"] + members)
    assert rc2 == 0 and out2 == out and rc8 == 0 and out8 != out
    probs = scored(tmp_path / "generated.pairs", out, members)
    assert len(probs) == 50 and all(np.isfinite(p) and p > 0 for p in probs), probs
    # --generate-paths with -@ has the same shape, and its pairs score too; -OWE prints a line a path: the same paths' output sides
    rc, out_at, err = run(["-q@", "--generate-paths=50", "-R", "7"] + members)
    assert rc == 0 and len(out_at.split("\n")) == 101, err
    probs = scored(tmp_path / "generated.pairs", out_at, members)
    assert len(probs) == 50 and all(p > 0 for p in probs), probs
    rc, out_o, err = run(["-qOWE", "--generate-paths=50", "-R", "7"] + members)
    assert rc == 0 and len(out_o.split("\n")) == 51, err
    assert out_o.split("\n")[:50] == out_at.split("\n")[1:100:2]
    rc, out_i, err = run(["-qIWE", "--generate-paths=50", "-R", "7"] + members)
    assert rc == 0 and out_i.split("\n")[:50] == out_at.split("\n")[0:100:2], err
    rc, out_w, err = run(["-qIE", "--generate-paths=50", "-R", "7"] + members)  # without -W a path ends with its weight
    assert rc == 0 and [l.rsplit(" ", 1)[0] for l in out_w.split("\n")[:50]] == out_i.split("\n")[:50], err
    # the limits reach the library: one arc is not enough for this machine
    rc, out, err = run(["-q", "--generate-pairs=5", "--generate-max-arcs=1", "--generate-tries=4"] + members)
    assert rc != 0 and out == "" and "carmel_hip_decoder_generate" in err and "path 0 " in err, err
