"""The dense cascade sweep (carmel_amd/csrc/dense.hpp) restated plainly in extended precision, and a generator of the
cascades it is tested on.  No GPU and no library of the project is used here: numpy alone.

The cascade is `locked bigram language model o one-state channel`.  Its composed arcs factor as
    weight(s -> s', cipher symbol c) = A[s][s'] * B[c][s'],
A[s][s'] the language model's arc s -> s' and B[c][s'] the channel's arc "plain symbol of s'":"c".  `parse_cascade` reads A,
B and the *e*:*e* arcs straight from the three texts (not through a composer), `dense_reference` is the scaled
linear-domain forward-backward over them, one position per loop step, and `brute_force` enumerates the paths.

The reference runs in numpy's longdouble, which must be the x87 80-bit format (64-bit mantissa) or better: the module
asserts np.finfo(np.longdouble).eps < 1e-18 when it is imported.  On a platform whose longdouble is a plain double the
tests that import it fail at collection instead of comparing f64 with f64.

Tolerance (`tol_rel`).  Every addend of the sweep is non-negative, so a sum of n terms in any order is within (n - 1) u of
the exact one, u = 2^-53, and both recurrences have condition number 1.  A position is an (S + 4)-term step (S products, the
channel factor, the scale, the *e*:*e* adds), its error grows at most linearly through T_max positions, on two passes with a
product of the two in the posterior: 4 (S + 4) T_max u.  A count is a sum over the N positions of the corpus: N u more.
    tol_rel = 4 (S + 4) T_max u + N u
It bounds the relative error of every count above 1e-200 x the total and of p.  ln p is compared relative to
max(1, |ln p|): a relative error e of p is an absolute error e of ln p, and the sum of T logarithms that makes ln p carries
u |ln p| per term of its own."""
import re

import numpy as np

assert np.finfo(np.longdouble).eps < 1e-18, "numpy's longdouble is no wider than a double here: no reference to compare with"

U = 2.0 ** -53


def tol_rel(S, t_max, n_positions):
    return 4.0 * (S + 4) * t_max * U + n_positions * U


# ---------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------
def plain_name(k):
    return "P%d" % k


def cipher_name(k):
    return "c%d" % k


def _fmt(x):
    return repr(float(x))  # shortest text that reads back as the same double


def make_cascade(n_plain, n_cipher, n_lines, lens, seed, *, stop_states=1, eps_chain=False, a_density=1.0, b_density=1.0,
                 weight_range=(0.05, 1.0), lm_scale=1.0, channel_scale=1.0):
    """(lm_text, channel_text, corpus_text) in the reference's file formats, after synth.cipher_files but with every size free.

    Language model: a locked bigram acceptor over *e*:"Pk" arcs, START + n_plain states + END (S = n_plain + 2), weights
    drawn uniformly from weight_range, then normalised per source state (so is the channel, per plain symbol).  The first `stop_states` plain states have an *e*:*e* arc to END.
    eps_chain = k (True = 1) adds k locked states X0 .. Xk-1 (S grows by k) with the *e*:*e* arcs p -> Xi and Xi -> END, p the
    last plain state; the Xi are named and listed before most plain states and `Xi -> END` stands before `p -> Xi` in the file,
    so neither state numbers nor file order give the topological order of the *e*:*e* arcs.
    a_density < 1 drops bigram arcs at random but keeps START -> P0, P0 -> P0 and the ring Pi -> Pi+1: every state stays
    reachable, can reach END, and a string of every length has a derivation.  b_density < 1 drops channel arcs but keeps
    one per plain symbol and one per cipher symbol.
    Channel: one state, n_plain x n_cipher arcs "Pk":"cj", unlocked.  lm_scale / channel_scale multiply the weights of a member.
    Corpus: n_lines pairs (weight line, blank input line, quoted cipher symbols), pair weights uniform in [0.5, 2], line i
    of length lens[i]: a walk through the model itself that ends in a stopping state, so every line has a derivation."""
    rng = np.random.default_rng(seed)
    n_x = int(eps_chain)
    lens = [int(x) for x in lens]
    assert len(lens) == n_lines and min(lens) >= 1 and 1 <= stop_states <= n_plain
    lo, hi = weight_range
    start_w = rng.uniform(lo, hi, n_plain)
    big_w = rng.uniform(lo, hi, (n_plain, n_plain))
    ch_w = rng.uniform(lo, hi, (n_plain, n_cipher))
    start_has = rng.random(n_plain) < a_density
    big_has = rng.random((n_plain, n_plain)) < a_density
    ch_has = rng.random((n_plain, n_cipher)) < b_density
    start_has[0] = True
    big_has[0, 0] = True
    for k in range(n_plain):
        big_has[k, (k + 1) % n_plain] = True
        ch_has[k, k % n_cipher] = True
    for c in range(n_cipher):
        ch_has[c % n_plain, c] = True
    stop_w = rng.uniform(lo, hi, stop_states)
    chain_w = rng.uniform(lo, hi, (max(n_x, 1), 2))
    last = n_plain - 1
    # a proper bigram model and channel: what leaves a state, and what a plain symbol becomes, sums to 1
    start_w = start_w / start_w[start_has].sum()
    out_sum = np.where(big_has, big_w, 0.0).sum(axis=1)
    out_sum[:stop_states] += stop_w
    out_sum[last] += chain_w[:n_x, 0].sum()
    big_w = big_w / out_sum[:, None]
    stop_w = stop_w / out_sum[:stop_states]
    chain_w[:, 0] /= out_sum[last]
    ch_w = ch_w / np.where(ch_has, ch_w, 0.0).sum(axis=1)[:, None]
    lm = ["END"]
    lm.append('(START (%s *e* "%s" %s!))' % (plain_name(0), plain_name(0), _fmt(start_w[0] * lm_scale)))
    for i in range(n_x):  # (stop arcs and the chain's arcs carry no symbol and are not scaled: a string takes one of them once)
        lm.append("(X%d (END *e* *e* %s!))" % (i, _fmt(chain_w[i, 1])))
    for k in range(1, n_plain):
        if start_has[k]:
            lm.append('(START (%s *e* "%s" %s!))' % (plain_name(k), plain_name(k), _fmt(start_w[k] * lm_scale)))
    for a in range(n_plain):
        for k in range(n_plain):
            if big_has[a, k]:
                lm.append('(%s (%s *e* "%s" %s!))' % (plain_name(a), plain_name(k), plain_name(k), _fmt(big_w[a, k] * lm_scale)))
    for i in range(n_x):
        lm.append("(%s (X%d *e* *e* %s!))" % (plain_name(last), i, _fmt(chain_w[i, 0])))
    for k in range(stop_states):
        lm.append("(%s (END *e* *e* %s!))" % (plain_name(k), _fmt(stop_w[k])))
    ch = ["0"]
    for a in range(n_plain):
        for c in range(n_cipher):
            if ch_has[a, c]:
                ch.append('(0 (0 "%s" "%s" %s))' % (plain_name(a), cipher_name(c), _fmt(ch_w[a, c] * channel_scale)))
    # the strings: can_end[k][s] = a walk of k more symbols from plain state s can stop
    sup = np.where(big_has, big_w, 0.0)
    emit = np.where(ch_has, ch_w, 0.0)
    ends = np.zeros(n_plain, bool)
    ends[:stop_states] = True
    if n_x:
        ends[last] = True
    max_len = max(lens)
    can_end = np.zeros((max_len, n_plain), bool)
    can_end[0] = ends
    for k in range(1, max_len):
        can_end[k] = (big_has & can_end[k - 1][None, :]).any(axis=1)
    pw = rng.uniform(0.5, 2.0, n_lines)
    out = []
    for i, L in enumerate(lens):
        p = np.where(start_has & can_end[L - 1], start_w, 0.0)
        syms = []
        for t in range(L):
            cur = int(rng.choice(n_plain, p=p / p.sum()))
            e = emit[cur]
            syms.append(int(rng.choice(n_cipher, p=e / e.sum())))
            if t + 1 < L:
                p = np.where(can_end[L - 2 - t], sup[cur], 0.0)
        out.append("%s\n\n%s" % (_fmt(pw[i]), " ".join('"%s"' % cipher_name(c) for c in syms)))
    return "\n".join(lm) + "\n", "\n".join(ch) + "\n", "\n".join(out) + "\n"


def corpus_text(seqs, weights, names):
    """pairs (weight line, blank input line, quoted cipher symbols) from lists of numbers into `names` (parse_cascade's
    cipher_names: symbols are numbered in order of appearance in the channel file)"""
    return "".join("%s\n\n%s\n" % (_fmt(w), " ".join('"%s"' % names[c] for c in s)) for s, w in zip(seqs, weights))


def retag(lm_text, ch_text):
    """the two model texts with every arc's weight replaced by 1 + its position among the file's arcs: composed by anything
    that keeps parameters apart, the weight of a parameter then names the arc of the file it came from"""
    def go(text):
        n = [0]

        def sub(m):
            n[0] += 1
            return "%s%d%s" % (m.group(1), n[0], m.group(3))
        return _ARC.sub(sub, text)
    return go(lm_text), go(ch_text)


# ---------------------------------------------------------------------------------------------------------------------
# the texts as matrices
# ---------------------------------------------------------------------------------------------------------------------
_ARC = re.compile(r'(\(\S+ \(\S+ \S+ \S+ )([^\s!)]+)(!?\)\))')
_ARC_FIELDS = re.compile(r'\((\S+) \((\S+) (\S+) (\S+) ([^\s!)]+)(!?)\)\)')


class Cascade(object):
    """S states (0 = START, then in order of appearance), V cipher symbols (in order of appearance in the channel).
    A[s][s'] (0 where no arc) with a_arc[s][s'] its arc's number in the language model file (-1: none); state_plain[s'] the
    plain symbol written on the way into s' (None for START, END and the Xi); B[c][s'] = channel weight of
    state_plain[s'] : c with b_arc[c][s'] its arc's number in the channel file; eps = [(src, dst, weight, arc number)] in
    topological order of the sources; seqs / weights the corpus (a symbol the channel never writes is numbered V)."""


def parse_cascade(lm_text, ch_text, corpus=None):
    m = Cascade()
    lines = lm_text.split("\n")
    fin_name = lines[0].strip()
    arcs = [_ARC_FIELDS.match(l).groups() for l in lines[1:] if l.strip()]
    state = {arcs[0][0]: 0}
    for a in arcs:
        for nm in a[:2]:
            state.setdefault(nm, len(state))
    state.setdefault(fin_name, len(state))
    S = m.S = len(state)
    m.state_names = sorted(state, key=state.get)
    m.start, m.fin = 0, state[fin_name]
    m.A, m.a_arc = np.zeros((S, S)), np.full((S, S), -1, np.int64)
    m.state_plain = [None] * S
    eps = []
    for k, (src, dst, i, o, w, lock) in enumerate(arcs):
        assert i == "*e*" and lock == "!", "a locked acceptor over *e*:x arcs"
        s, d = state[src], state[dst]
        if o == "*e*":
            eps.append((s, d, float(w), k))
            continue
        sym = o.strip('"')
        assert m.state_plain[d] in (None, sym), "a bigram model: one symbol per destination state"
        assert m.a_arc[s, d] < 0
        m.state_plain[d] = sym
        m.A[s, d], m.a_arc[s, d] = float(w), k
    depth = [0] * S  # longest *e*-path into a state (the arcs are few: relax until nothing moves)
    for _ in range(len(eps) + 1):
        for s, d, _w, _k in eps:
            depth[d] = max(depth[d], depth[s] + 1)
    assert max(depth) <= len(eps), "*e*:*e* cycle"
    m.eps = sorted(eps, key=lambda e: depth[e[0]])
    ch = [_ARC_FIELDS.match(l).groups() for l in ch_text.split("\n")[1:] if l.strip()]
    cipher = {}
    for a in ch:
        cipher.setdefault(a[3].strip('"'), len(cipher))
    V = m.V = len(cipher)
    m.cipher_names = sorted(cipher, key=cipher.get)
    by_plain = {}
    for s in range(S):
        if m.state_plain[s] is not None:
            by_plain.setdefault(m.state_plain[s], []).append(s)
    m.B, m.b_arc = np.zeros((V, S)), np.full((V, S), -1, np.int64)
    for k, (_s, _d, i, o, w, _lock) in enumerate(ch):
        for s in by_plain.get(i.strip('"'), ()):
            c = cipher[o.strip('"')]
            assert m.b_arc[c, s] < 0
            m.B[c, s], m.b_arc[c, s] = float(w), k
    m.n_lm_arcs, m.n_ch_arcs = len(arcs), len(ch)
    m.seqs, m.weights = [], []
    if corpus is not None:
        cl = corpus.split("\n")
        if cl and cl[-1] == "":
            cl.pop()
        assert len(cl) % 3 == 0
        for k in range(0, len(cl), 3):
            assert cl[k + 1] == ""
            m.weights.append(float(cl[k]))
            m.seqs.append(np.array([cipher.get(x.strip('"'), V) for x in cl[k + 2].split()], np.int64))
    return m


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def dense_reference(A, B, start, fin, eps, seqs, weights, dtype=np.longdouble):
    """Scaled forward-backward of dense.hpp.  A [S][S], B [V][S], eps = (src, dst, weight) triples in topological order
    (applied in that order forward, in reverse backward), seqs = symbol numbers per pair, weights = pair weights.
    Returns (ln p per pair, counts [V][S]): counts[c][s'] = sum over pairs of weight x the expected number of positions at
    which the pair enters s' writing c.  A pair without a derivation has ln p = -inf and adds nothing."""
    A, B = np.asarray(A, dtype), np.asarray(B, dtype)
    S, V = A.shape[0], B.shape[0]
    eps = [(int(e[0]), int(e[1]), dtype(e[2])) for e in eps]
    counts = np.zeros((V, S), dtype)
    lnp = np.full(len(seqs), -np.inf, dtype)

    def eps_forward(a):
        for s, d, w in eps:
            a[d] += a[s] * w

    def eps_backward(b):
        for s, d, w in reversed(eps):
            b[s] += b[d] * w

    for n, (seq, pw) in enumerate(zip(seqs, weights)):
        T = len(seq)
        if T == 0 or max(seq) >= V:
            continue
        a = np.zeros(S, dtype)
        a[start] = 1
        eps_forward(a)
        pre, zs = [], []
        lp = dtype(0)
        for t in range(T):
            v = a @ A             # the values parked for the posteriors: before the channel factor
            pre.append(v)
            v = v * B[seq[t]]
            z = v.sum()
            if not z > 0:
                break
            a = v / z
            eps_forward(a)
            zs.append(z)
            lp += np.log(z)
        if len(zs) < T or not a[fin] > 0:
            continue
        lnp[n] = lp + np.log(a[fin])
        b = np.zeros(S, dtype)
        b[fin] = 1 / a[fin]
        for t in range(T - 1, -1, -1):
            eps_backward(b)
            w = B[seq[t]] * b / zs[t]
            counts[seq[t]] += pre[t] * w * dtype(pw)
            b = A @ w
    return lnp, counts


def brute_force(A, B, start, fin, eps, seqs, weights):
    """the same two results from an enumeration of every path (exact sums of path products in longdouble)"""
    ld = np.longdouble
    A, B = np.asarray(A, ld), np.asarray(B, ld)
    S, V = A.shape[0], B.shape[0]
    eps = [(int(e[0]), int(e[1]), ld(e[2])) for e in eps]
    counts = np.zeros((V, S), ld)
    lnp = np.full(len(seqs), -np.inf, ld)
    for n, (seq, pw) in enumerate(zip(seqs, weights)):
        T = len(seq)
        paths = []  # (weight, [(symbol, state entered)])

        def walk(s, t, w, visits):
            if t == T and s == fin:
                paths.append((w, list(visits)))
            for es, ed, ew in eps:
                if es == s:
                    walk(ed, t, w * ew, visits)
            if t < T:
                for j in range(S):
                    x = A[s, j] * B[seq[t], j]
                    if x > 0:
                        visits.append((seq[t], j))
                        walk(j, t + 1, w * x, visits)
                        visits.pop()
        walk(start, 0, ld(1), [])
        p = sum((w for w, _ in paths), ld(0))
        if not p > 0:
            continue
        lnp[n] = np.log(p)
        for w, visits in paths:
            for c, j in visits:
                counts[c, j] += ld(pw) * w / p
    return lnp, counts


def compare_counts(got, ref, tol=None):
    """the largest relative error of `got` over the entries whose reference exceeds 1e-200 x the total (asserted <= tol
    unless tol is None); reference zeros must be exact zeros, smaller non-zero ones finite and below that threshold"""
    got, ref = np.asarray(got, np.longdouble).ravel(), np.asarray(ref, np.longdouble).ravel()
    assert got.shape == ref.shape
    assert np.isfinite(got.astype(np.float64)).all(), "inf or nan among the counts"
    floor = ref.sum() * np.longdouble(1e-200)
    zero, big = ref == 0, ref > floor
    assert (got[zero] == 0).all(), "a count where the reference has exactly none"
    small = ~zero & ~big
    assert (np.abs(got[small]) <= floor).all()
    if not big.any():
        return 0.0
    err = float((np.abs(got[big] - ref[big]) / ref[big]).max())
    assert tol is None or err <= tol, "counts: relative error %.3g above the bound %.3g" % (err, tol)
    return err


def compare_lnp(got, ref, tol=None):
    """largest |got - ref| / max(1, |ref|) over the pairs with a derivation (asserted <= tol unless tol is None); -inf
    must be -inf"""
    got, ref = np.asarray(got, np.longdouble), np.asarray(ref, np.longdouble)
    dead = np.isneginf(ref)
    assert (np.isneginf(got[dead])).all(), "ln p of a pair without a derivation"
    live = ~dead
    assert np.isfinite(got[live].astype(np.float64)).all(), "inf or nan among ln p"
    if not live.any():
        return 0.0
    err = float((np.abs(got[live] - ref[live]) / np.maximum(1, np.abs(ref[live]))).max())
    assert tol is None or err <= tol, "ln p: error %.3g above the bound %.3g" % (err, tol)
    return err


# ---------------------------------------------------------------------------------------------------------------------
# the two ceilings of the unrolled layouts, restated from the sources (the tests sit on both sides of each)
# ---------------------------------------------------------------------------------------------------------------------
def unrolled_max_len(n_slots, S):
    """largest string length for which unrolled_waves(n_slots, max_len, S) of unrolled.hip is non-zero: one wavefront's
    accumulators and 64 / width strings of max_len + 2 doubles within 64 KB of LDS (width 16, 32 or 64 lanes per string)"""
    per_wave = 64 // (16 if S <= 16 else 32 if S <= 32 else 64)
    L = 0
    while (n_slots + per_wave * (L + 1 + 2)) * 8 <= 64 * 1024:
        L += 1
    return L


def dense_max_symbols(SP, slots_per_symbol):
    """largest V with V * SP * 10 + n_slots * 8 <= 60 KB (dense_try_build), n_slots = slots_per_symbol * V"""
    V = 0
    while (V + 1) * SP * 10 + slots_per_symbol * (V + 1) * 8 <= 60 * 1024:
        V += 1
    return V


def length_case(S, over=0):
    """three lines, the longest exactly at the length ceiling of a full cascade of S states with n_plain + 3 cipher symbols
    (+ over); returns (texts, longest length)"""
    n_plain = S - 2
    n_cipher = n_plain + 3
    L = unrolled_max_len(n_plain * n_cipher, S) + over
    return make_cascade(n_plain, n_cipher, 3, [L, 5, 40], 100 + S), L
