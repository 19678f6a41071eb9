"""The rule of carmel_hip_consolidate (include/carmel_hip.h, csrc/consolidate.hip; carmel -C) restated in Python: a dict over key
tuples, sums in numpy's longdouble (sweep_math_cases asserts its 64-bit mantissa on import).

Inputs: the arcs in arc-id order with src non-decreasing; mode "sum" or "max"; clamp, read in sum mode only.  An arc exists iff
logw > -inf; NaN, +inf or unsorted src is an error (ValueError here, CARMEL_HIP_ERR_ARG there).  A segment is all existing arcs of
equal (src, dst, in, out); its representative is its lowest arc id; a segment of one member keeps that member's weight bit for bit
in every mode; max mode copies the largest member's bits; sum mode is ln sum exp(w_i), and with clamp a result > 0 becomes 0.  New
arc j is the segment with the j-th smallest representative id."""
import numpy as np

import sweep_math_cases  # noqa: F401 (asserts that longdouble is wider than a double)

LD = np.longdouble
NONE = 0xFFFFFFFF


def lse(x):
    """ln sum exp(x) in longdouble; x: finite doubles, at least one"""
    x = np.asarray(x, np.float64).astype(LD)
    m = x.max()
    return m + np.log(np.exp(x - m).sum())


class Consolidated(object):
    """n_kept; kept_id, arc_map (uint32 arrays); size[j]: members of new arc j; value[j]: its weight, a float64 where the rule fixes
    every bit (exact[j]) and a longdouble otherwise (a sum of two or more members, not clamped away)"""

    def __init__(self, src, dst, isym, osym, logw, mode="sum", clamp=True):
        assert mode in ("sum", "max")
        src, dst, isym, osym = (np.asarray(a, np.uint32) for a in (src, dst, isym, osym))
        logw = np.asarray(logw, np.float64)
        n = len(src)
        if n >= NONE:
            raise ValueError("too many arcs")
        if np.isnan(logw).any() or (logw == np.inf).any():
            raise ValueError("a weight is NaN or +inf")
        if n and (np.diff(src.astype(np.int64)) < 0).any():
            raise ValueError("src decreases")
        members = {}  # key -> arc ids, ascending; dicts keep insertion order: the order of the representatives
        for a in range(n):
            if logw[a] > -np.inf:
                members.setdefault((int(src[a]), int(dst[a]), int(isym[a]), int(osym[a])), []).append(a)
        self.n_arcs = n
        self.n_kept = len(members)
        self.kept_id = np.array([ids[0] for ids in members.values()], np.uint32)
        self.arc_map = np.full(n, NONE, np.uint32)
        self.size = np.array([len(ids) for ids in members.values()], np.int64)
        self.value, self.exact = [], []
        for j, ids in enumerate(members.values()):
            self.arc_map[ids] = j
            w = logw[ids]
            if len(ids) == 1:
                self.value.append(w[0])
                self.exact.append(True)
            elif mode == "max":
                self.value.append(w.max())
                self.exact.append(True)
            else:
                self.value.append(lse(w))
                self.exact.append(False)
        self.clamp = bool(clamp) and mode == "sum"
        self.mode = mode

    def rounded(self):
        """-> the weights as float64, clamped where the rule clamps: what a second consolidation would be given"""
        out = np.array([np.float64(v) for v in self.value], np.float64).reshape(self.n_kept)
        if self.clamp:
            out = np.where((self.size > 1) & (out > 0.0), 0.0, out)
        return out
