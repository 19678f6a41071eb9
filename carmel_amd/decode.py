"""Batch 1-best and k-best decoding, all-paths sums, posterior path samples and arc posteriors on the GPU (carmel -b -k n;
include/carmel_hip.h carmel_hip_decoder_*, csrc/decode.hip, csrc/decode_kbest.hip, csrc/decode_sum.hip, csrc/decode_sample.hip
and csrc/decode_posterior.hip, on the drivers of csrc/decode_paths.hip).

    d = Decoder(wfst, side=0)          # side 0: lines are input strings; 1: output strings (carmel -r)
    best, paths = d.decode(lines)      # lines: sequences of symbol ids of that side's alphabet
    weights, kpaths = d.decode_kbest(lines, k)
    sums = d.sum(lines)                # ln of every line's sum over ALL its derivations (carmel -b --sum; csrc/decode_sum.hip)
    weights, spaths = d.sample(lines, n, seed=0)   # n derivations per line, each drawn with probability weight / sum
    sums, counts = d.posterior(lines, weights=None)   # expected uses of every arc over all derivations of the lines
    best, paths = d.decode_pairs(lines, lines2)    # lines2: the other side's line of every pair (carmel --post-b=FILE)
    sums = d.sum_pairs(lines, lines2)              # ln of every pair's sum over all its derivations (csrc/decode_pairs.hip)
    sums, counts = d.posterior_pairs(lines, lines2, weights=None)   # expected uses of every arc over the pairs' derivations
    weights, spaths = d.sample_pairs(lines, lines2, n, seed=0)      # n derivations per pair, each drawn with probability weight / sum
    weights, kpaths = d.decode_pairs_kbest(lines, lines2, k)        # the k best alignments of every pair (csrc/decode_pairs_kbest.hip)
    paths = d.generate(n, mode="joint", seed=0)    # n random paths drawn from the machine itself (carmel -G n; csrc/decode_generate.hip)
    pairs = d.generate_pairs(n, seed=0)            # n random (input, output) strings (carmel -g n: mode "conditional")
    kbest = d.best_paths(k)                        # the k best paths of the machine itself, best first (carmel -k n; csrc/decode_best_paths.hip)
    state_keep, arc_keep = d.prune(log_ratio, max_states, min_arc_logw)   # what stays of the machine (carmel -w / -z / -p; csrc/decode_prune.hip)
    F, R = d.prune_distances()                     # the best distance from state 0 to every state and from every state to the final one
    Z, N, n_useful = d.machine_sums()              # the ln of the sum over all paths of the machine, and their number (csrc/decode_machine_sums.hip)
    alpha, beta, cf, cb, level = d.machine_sums_states(); ln_gamma = d.machine_sums_arcs()   # per state, and every arc's ln posterior
    d.set_weights(logw); d.close()
    w2, arc_map, ms = consolidate(wfst, mode="sum", clamp=True)   # duplicate arcs merged (carmel -C; csrc/consolidate.hip): no decoder needed

best[l] is the natural log of line l's best path weight (-inf: no derivation); paths[l] its arc ids in path order.
weights[l] holds the reported ln weights of line l's min(k, number of derivations) best derivations, best first, and kpaths[l]
their arc ids; rank 0 is decode's path.  sample returns the same shapes: a line with a derivation has exactly n paths, in sample
order, duplicates kept; sample s of line l depends on the machine, the line, the seed, l and s alone.  posterior returns sum's
sums, bit for bit, and counts[a] = the sum over the lines with a derivation of weights[l] (1 without weights) times the expected
number of uses of arc a over line l's derivations, each derivation weighing weight / sum (csrc/decode_posterior.hip: forward and
backward trellis); the sums are fixed to the bit, the counts up to the order of the device's atomic adds.
A pair (lines[l], lines2[l]) is a line of the decoder's side and a line of the other side, in that side's alphabet; its
derivations spell both.  decode_pairs returns decode's shapes (the Viterbi alignment of every pair), sum_pairs sum's, and
posterior_pairs posterior's: sum_pairs' sums, bit for bit, and the arcs' expected uses over the pairs' derivations
(csrc/decode_pairs_posterior.hip: the pair trellis forwards and backwards).  sample_pairs returns sample's shapes: a pair with a
derivation has exactly n alignments, in sample order, duplicates kept, each drawn from the posterior over the pair's derivations;
sample s of pair l depends on the machine, the pair, the seed, l and s alone (csrc/decode_pairs_sample.hip: the forward planes of
the arc posteriors and a backward sampling walk); sample_pairs_raw returns sample_raw's flat arrays.  decode_pairs_kbest returns
decode_kbest's shapes: per pair the reported ln weights and the arc ids of its min(k, number of derivations) best alignments,
best first, 1 <= k <= 1024; rank 0 is decode_pairs' path and weight, and an insertion loop *e*:y is legal for every k
(csrc/decode_pairs_kbest.hip: the pair trellis with a list of k values a node); decode_pairs_kbest_raw returns decode_kbest_raw's
flat arrays.
generate draws from the model, not from a line's posterior: a forward random walk from state 0 that stops the first time it
reaches the final state, an arc chosen with probability weight / (the weights leaving the state) in mode "joint", and in mode
"conditional" first one of the state's matched-side symbols uniformly, then an arc among that symbol's by weight; a walk that
meets a dead end or max_arcs arcs is drawn again, max_tries times at most (CarmelHipError otherwise).  Path p of a call is path
first + p of the stream of (seed, mode): it does not depend on how the stream is cut into calls (include/carmel_hip.h has the
rule in full)."""
import ctypes as C

import numpy as np

from ._capi import check, f64, lib, ptr, u32, u64


GENERATE_MODES = {"joint": 0, "conditional": 1}  # CARMEL_HIP_GENERATE_JOINT (carmel -G), CARMEL_HIP_GENERATE_CONDITIONAL (carmel -g)


def _pack(lines):
    """-> (off, sym): the CSR of the lines' symbols, as every decode entry point takes it"""
    lines = [np.asarray(x, dtype=np.uint32) for x in lines]
    off = u64(np.concatenate([[0], np.cumsum([len(x) for x in lines], dtype=np.uint64)]))
    sym = u32(np.concatenate(lines)) if off[-1] else np.zeros(1, np.uint32)
    return off, sym


class Decoder(object):
    def __init__(self, wfst, side=0, device=0):
        self.n_arcs, self.n_states = wfst.n_arcs, wfst.n_states
        self._h = C.c_void_p()
        self._keep = [u32(wfst.src), u32(wfst.dst), u32(wfst.isym), u32(wfst.osym)]
        check(lib.carmel_hip_decoder_create(C.byref(self._h), device, wfst.n_states, wfst.final, wfst.n_arcs,
                                            *[ptr(a) for a in self._keep], ptr(f64(wfst.logw)), int(side)),
              "carmel_hip_decoder_create")

    def set_weights(self, logw):
        logw = f64(logw)
        assert len(logw) == self.n_arcs
        check(lib.carmel_hip_decoder_set_weights(self._h, ptr(logw)), "carmel_hip_decoder_set_weights")

    def decode(self, lines):
        off, sym = _pack(lines)
        best = np.empty(len(lines))
        path_off = np.zeros(len(lines) + 1, np.uint64)
        check(lib.carmel_hip_decode(self._h, len(lines), ptr(off), ptr(sym), ptr(best), ptr(path_off)), "carmel_hip_decode")
        arcs = np.zeros(max(int(path_off[-1]), 1), np.uint32)
        check(lib.carmel_hip_decoder_get_paths(self._h, ptr(arcs)), "carmel_hip_decoder_get_paths")
        paths = [arcs[int(path_off[l]):int(path_off[l + 1])].copy() for l in range(len(lines))]
        return best, paths

    def decode_kbest_raw(self, lines, k):
        """-> (line_paths, logw, path_off, arcs): the arrays of carmel_hip_decode_kbest / carmel_hip_decoder_get_kbest"""
        off, sym = _pack(lines)
        line_paths = np.zeros(len(lines) + 1, np.uint64)
        check(lib.carmel_hip_decode_kbest(self._h, int(k), len(lines), ptr(off), ptr(sym), ptr(line_paths)),
              "carmel_hip_decode_kbest")
        return self._last_paths(line_paths)

    def sample_raw(self, lines, n, seed=0):
        """-> (line_paths, logw, path_off, arcs): the arrays of carmel_hip_decode_sample / carmel_hip_decoder_get_kbest"""
        off, sym = _pack(lines)
        line_paths = np.zeros(len(lines) + 1, np.uint64)
        check(lib.carmel_hip_decode_sample(self._h, int(n), int(seed), len(lines), ptr(off), ptr(sym), ptr(line_paths)),
              "carmel_hip_decode_sample")
        return self._last_paths(line_paths)

    def _last_paths(self, line_paths):
        n_paths, n_arcs = C.c_uint64(), C.c_uint64()
        check(lib.carmel_hip_decoder_kbest_size(self._h, C.byref(n_paths), C.byref(n_arcs)), "carmel_hip_decoder_kbest_size")
        assert n_paths.value == int(line_paths[-1])
        logw = np.zeros(max(n_paths.value, 1))
        path_off = np.zeros(n_paths.value + 1, np.uint64)
        arcs = np.zeros(max(n_arcs.value, 1), np.uint32)
        check(lib.carmel_hip_decoder_get_kbest(self._h, ptr(logw), ptr(path_off), ptr(arcs)), "carmel_hip_decoder_get_kbest")
        return line_paths, logw[:n_paths.value], path_off, arcs[:n_arcs.value]

    def decode_kbest(self, lines, k):
        return self._per_line(len(lines), *self.decode_kbest_raw(lines, k))

    def sample(self, lines, n, seed=0):
        """-> (weights, paths) shaped as decode_kbest's: per line its n sampled derivations (none: no derivation)"""
        return self._per_line(len(lines), *self.sample_raw(lines, n, seed))

    @staticmethod
    def _per_line(n_lines, line_paths, logw, path_off, arcs):
        weights, paths = [], []
        for l in range(n_lines):
            a, b = int(line_paths[l]), int(line_paths[l + 1])
            weights.append(logw[a:b].copy())
            paths.append([arcs[int(path_off[p]):int(path_off[p + 1])].copy() for p in range(a, b)])
        return weights, paths

    def sum(self, lines):
        """-> f64 array: per line, the ln of the sum over all its derivations of their weights (-inf: no derivation)"""
        off, sym = _pack(lines)
        out = np.empty(len(lines))
        check(lib.carmel_hip_decode_sum(self._h, len(lines), ptr(off), ptr(sym), ptr(out)), "carmel_hip_decode_sum")
        return out

    def decode_pairs(self, lines, lines2):
        """-> (best, paths) as decode returns them, over the derivations that spell lines[l] on this side and lines2[l] on the other"""
        assert len(lines) == len(lines2)
        off, sym = _pack(lines)
        off2, sym2 = _pack(lines2)
        best = np.empty(len(lines))
        path_off = np.zeros(len(lines) + 1, np.uint64)
        check(lib.carmel_hip_decode_pairs(self._h, len(lines), ptr(off), ptr(sym), ptr(off2), ptr(sym2), ptr(best), ptr(path_off)),
              "carmel_hip_decode_pairs")
        arcs = np.zeros(max(int(path_off[-1]), 1), np.uint32)
        check(lib.carmel_hip_decoder_get_paths(self._h, ptr(arcs)), "carmel_hip_decoder_get_paths")
        return best, [arcs[int(path_off[l]):int(path_off[l + 1])].copy() for l in range(len(lines))]

    def sum_pairs(self, lines, lines2):
        """-> f64 array: per pair, the ln of the sum over all its derivations of their weights (-inf: no derivation)"""
        assert len(lines) == len(lines2)
        off, sym = _pack(lines)
        off2, sym2 = _pack(lines2)
        out = np.empty(len(lines))
        check(lib.carmel_hip_decode_pairs_sum(self._h, len(lines), ptr(off), ptr(sym), ptr(off2), ptr(sym2), ptr(out)),
              "carmel_hip_decode_pairs_sum")
        return out

    def posterior_pairs(self, lines, lines2, weights=None):
        """-> (sums, counts): sum_pairs(lines, lines2), and per arc its expected number of uses over the derivations of the pairs
        (pair l counts weights[l] times, 1 without weights; weights are finite and >= 0); a pair without a derivation adds nothing"""
        assert len(lines) == len(lines2)
        off, sym = _pack(lines)
        off2, sym2 = _pack(lines2)
        sums = np.empty(len(lines))
        counts = np.zeros(max(self.n_arcs, 1))
        wt = None if weights is None else f64(weights)
        assert wt is None or len(wt) == len(lines)
        check(lib.carmel_hip_decode_pairs_posterior(self._h, len(lines), ptr(off), ptr(sym), ptr(off2), ptr(sym2), ptr(wt), ptr(sums),
                                                    ptr(counts)), "carmel_hip_decode_pairs_posterior")
        return sums, counts[:self.n_arcs]

    def sample_pairs_raw(self, lines, lines2, n, seed=0):
        """-> (line_paths, logw, path_off, arcs): the arrays of carmel_hip_decode_pairs_sample / carmel_hip_decoder_get_kbest"""
        assert len(lines) == len(lines2)
        off, sym = _pack(lines)
        off2, sym2 = _pack(lines2)
        line_paths = np.zeros(len(lines) + 1, np.uint64)
        check(lib.carmel_hip_decode_pairs_sample(self._h, int(n), int(seed), len(lines), ptr(off), ptr(sym), ptr(off2), ptr(sym2),
                                                 ptr(line_paths)), "carmel_hip_decode_pairs_sample")
        return self._last_paths(line_paths)

    def sample_pairs(self, lines, lines2, n, seed=0):
        """-> (weights, paths) shaped as sample's: per pair its n sampled derivations (none: no derivation)"""
        return self._per_line(len(lines), *self.sample_pairs_raw(lines, lines2, n, seed))

    def decode_pairs_kbest_raw(self, lines, lines2, k):
        """-> (line_paths, logw, path_off, arcs): the arrays of carmel_hip_decode_pairs_kbest / carmel_hip_decoder_get_kbest"""
        assert len(lines) == len(lines2)
        off, sym = _pack(lines)
        off2, sym2 = _pack(lines2)
        line_paths = np.zeros(len(lines) + 1, np.uint64)
        check(lib.carmel_hip_decode_pairs_kbest(self._h, int(k), len(lines), ptr(off), ptr(sym), ptr(off2), ptr(sym2),
                                                ptr(line_paths)), "carmel_hip_decode_pairs_kbest")
        return self._last_paths(line_paths)

    def decode_pairs_kbest(self, lines, lines2, k):
        """-> (weights, paths) shaped as decode_kbest's: per pair its min(k, number of derivations) best alignments, best first"""
        return self._per_line(len(lines), *self.decode_pairs_kbest_raw(lines, lines2, k))

    def generate_raw(self, n, mode="joint", seed=0, max_arcs=1000, max_tries=256, first=0):
        """-> (logw, path_off, arcs, tries): n random paths through the machine (carmel_hip_decoder_generate), path p being path
        first + p of the stream of (seed, mode); tries[p] the attempts it took"""
        n = int(n)
        tries = np.zeros(max(n, 1), np.uint32)
        check(lib.carmel_hip_decoder_generate(self._h, GENERATE_MODES[mode], n, int(first), int(seed), int(max_arcs), int(max_tries),
                                              ptr(tries)), "carmel_hip_decoder_generate")
        _, logw, path_off, arcs = self._last_paths(np.array([0, n], np.uint64))
        return logw, path_off, arcs, tries[:n]

    def generate(self, n, mode="joint", seed=0, max_arcs=1000, max_tries=256, first=0):
        """-> [(ln weight, [arc ids])]: n random paths (carmel -G n; mode "conditional": the paths behind carmel -g n)"""
        logw, path_off, arcs, _ = self.generate_raw(n, mode, seed, max_arcs, max_tries, first)
        return [(float(logw[p]), [int(a) for a in arcs[int(path_off[p]):int(path_off[p + 1])]]) for p in range(len(logw))]

    def generate_pairs(self, n, mode="conditional", seed=0, max_arcs=1000, max_tries=256, first=0):
        """-> [(input symbols, output symbols)]: the two strings of n random paths, epsilons dropped (carmel -g n)"""
        isym, osym = self._keep[2], self._keep[3]
        return [([int(isym[a]) for a in path if isym[a]], [int(osym[a]) for a in path if osym[a]])
                for _, path in self.generate(n, mode, seed, max_arcs, max_tries, first)]

    def best_paths_raw(self, k):
        """-> (logw, path_off, arcs): the min(k, number of paths) best paths of the whole machine from state 0 to the final state,
        best first (carmel_hip_decoder_best_paths)"""
        n = C.c_uint64()
        check(lib.carmel_hip_decoder_best_paths(self._h, int(k), C.byref(n)), "carmel_hip_decoder_best_paths")
        _, logw, path_off, arcs = self._last_paths(np.array([0, n.value], np.uint64))
        return logw, path_off, arcs

    def best_paths(self, k):
        """-> [(reported ln weight, uint32 array of arc ids)]: the k best paths of the machine (carmel -k n; csrc/decode_best_paths.hip)"""
        logw, path_off, arcs = self.best_paths_raw(k)
        return [(float(logw[p]), arcs[int(path_off[p]):int(path_off[p + 1])].copy()) for p in range(len(logw))]

    def best_paths_stats(self):
        """-> (rounds, states_selected) of the last best_paths call"""
        rounds, selected = C.c_uint32(), C.c_uint64()
        check(lib.carmel_hip_decoder_best_paths_stats(self._h, C.byref(rounds), C.byref(selected)),
              "carmel_hip_decoder_best_paths_stats")
        return rounds.value, selected.value

    def prune(self, log_ratio=np.inf, max_states=None, min_arc_logw=-np.inf):
        """-> (state_keep, arc_keep), bool arrays: the states and arcs that lie on a path from state 0 to the final state whose
        weight is within log_ratio of the best path's, at most max_states states (those of the best paths through them), no arc of
        log weight below min_arc_logw (carmel_hip_decoder_prune; include/carmel_hip.h has the rule)"""
        state_keep = np.zeros(self.n_states, np.uint8)
        arc_keep = np.zeros(max(self.n_arcs, 1), np.uint8)
        ns, na = C.c_uint64(), C.c_uint64()
        cap = 0xFFFFFFFF if max_states is None else int(max_states)
        check(lib.carmel_hip_decoder_prune(self._h, float(log_ratio), cap, float(min_arc_logw), ptr(state_keep), ptr(arc_keep),
                                           C.byref(ns), C.byref(na)), "carmel_hip_decoder_prune")
        arc_keep = arc_keep[:self.n_arcs]
        assert ns.value == int(state_keep.sum()) and na.value == int(arc_keep.sum())
        return state_keep.astype(bool), arc_keep.astype(bool)

    def prune_distances(self):
        """-> (F, R) of the last prune call: per state the best value of a path from state 0 to it and from it to the final state
        (-inf: none)"""
        fwd, bwd = np.empty(self.n_states), np.empty(self.n_states)
        check(lib.carmel_hip_decoder_prune_distances(self._h, ptr(fwd), ptr(bwd)), "carmel_hip_decoder_prune_distances")
        return fwd, bwd

    def prune_stats(self):
        """-> (forward rounds, backward rounds) of the last prune call"""
        f, b = C.c_uint32(), C.c_uint32()
        check(lib.carmel_hip_decoder_prune_stats(self._h, C.byref(f), C.byref(b)), "carmel_hip_decoder_prune_stats")
        return f.value, b.value

    def machine_sums(self):
        """-> (total_logw, n_paths, n_useful): the ln of the sum over ALL paths of the machine from state 0 to the final state
        (-inf: none), their number (an f64, exact below 2^53) and the number of states on such a path
        (carmel_hip_decoder_machine_sums; include/carmel_hip.h has the rule).  A cycle among those states: CarmelHipError"""
        z, n, u = C.c_double(), C.c_double(), C.c_uint64()
        check(lib.carmel_hip_decoder_machine_sums(self._h, C.byref(z), C.byref(n), C.byref(u)), "carmel_hip_decoder_machine_sums")
        return z.value, n.value, u.value

    def machine_sums_states(self):
        """-> (alpha, beta, paths_to, paths_from, level) of the last machine_sums call, per state: the ln of the sum over the paths
        from state 0 to it and from it to the final state, their numbers, and its level (0xffffffff: not on a path)"""
        Q = self.n_states
        alpha, beta, cf, cb, level = np.empty(Q), np.empty(Q), np.empty(Q), np.empty(Q), np.empty(Q, np.uint32)
        check(lib.carmel_hip_decoder_machine_sums_states(self._h, ptr(alpha), ptr(beta), ptr(cf), ptr(cb), ptr(level)),
              "carmel_hip_decoder_machine_sums_states")
        return alpha, beta, cf, cb, level

    def machine_sums_arcs(self):
        """-> per arc the ln of its expected number of uses on a path drawn with probability weight / sum (-inf: on no path), of
        the last machine_sums call"""
        post = np.full(max(self.n_arcs, 1), -np.inf)
        check(lib.carmel_hip_decoder_machine_sums_arcs(self._h, ptr(post)), "carmel_hip_decoder_machine_sums_arcs")
        return post[:self.n_arcs]

    def machine_sums_stats(self):
        """-> (forward levels, backward levels) of the last machine_sums call"""
        f, b = C.c_uint32(), C.c_uint32()
        check(lib.carmel_hip_decoder_machine_sums_stats(self._h, C.byref(f), C.byref(b)), "carmel_hip_decoder_machine_sums_stats")
        return f.value, b.value

    def posterior(self, lines, weights=None):
        """-> (sums, counts): sum(lines), and per arc its expected number of uses over the derivations of the lines (line l counts
        weights[l] times, 1 without weights; weights are finite and >= 0); a line without a derivation adds nothing"""
        off, sym = _pack(lines)
        sums = np.empty(len(lines))
        counts = np.zeros(max(self.n_arcs, 1))
        wt = None if weights is None else f64(weights)
        assert wt is None or len(wt) == len(lines)
        check(lib.carmel_hip_decode_posterior(self._h, len(lines), ptr(off), ptr(sym), ptr(wt), ptr(sums), ptr(counts)),
              "carmel_hip_decode_posterior")
        return sums, counts[:self.n_arcs]

    def last_ms(self):
        ms = C.c_double()
        check(lib.carmel_hip_decoder_last_ms(self._h, C.byref(ms)), "carmel_hip_decoder_last_ms")
        return ms.value

    def close(self):
        if self._h:
            lib.carmel_hip_decoder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


CONSOLIDATE_MODES = {"sum": 0, "max": 1}


def consolidate_raw(src, dst, isym, osym, logw, mode="sum", clamp=True, device=0):
    """-> (n_kept, kept_id, kept_logw, arc_map, kernel_ms): the arrays of carmel_hip_consolidate (include/carmel_hip.h has the
    rule), kept_id and kept_logw cut to n_kept entries"""
    src, dst, isym, osym, logw = u32(src), u32(dst), u32(isym), u32(osym), f64(logw)
    n = len(src)
    assert all(len(a) == n for a in (dst, isym, osym, logw))
    arc_map, kept_id, kept_logw = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1))
    n_kept, ms = C.c_uint64(), C.c_double()
    check(lib.carmel_hip_consolidate(int(device), n, ptr(src), ptr(dst), ptr(isym), ptr(osym), ptr(logw), CONSOLIDATE_MODES[mode],
                                     1 if clamp else 0, ptr(arc_map), ptr(kept_id), ptr(kept_logw), C.byref(n_kept), C.byref(ms)),
          "carmel_hip_consolidate")
    k = n_kept.value
    return k, kept_id[:k], kept_logw[:k], arc_map[:n], ms.value


def consolidate(wfst, mode="sum", clamp=True, device=0):
    """-> (Wfst, arc_map, kernel_ms): arcs of the same source, destination, input and output merged into one (carmel -C;
    csrc/consolidate.hip), of their summed weight (mode "sum"; at most 1 with clamp) or of their largest weight (mode "max":
    carmel --consolidate-max).  The new machine's arcs are the first arc of every such set, in the old order, with that arc's
    symbols and tie group; arc_map[a] is old arc a's new id, 0xffffffff for an arc of weight zero, which goes."""
    from .model import Wfst
    _, kept_id, kept_logw, arc_map, ms = consolidate_raw(wfst.src, wfst.dst, wfst.isym, wfst.osym, wfst.logw, mode, clamp, device)
    new = Wfst(wfst.n_states, wfst.final, wfst.src[kept_id], wfst.dst[kept_id], wfst.isym[kept_id], wfst.osym[kept_id], kept_logw,
               wfst.group[kept_id])
    return new, arc_map, ms
