"""Batch 1-best decoding on the GPU (carmel -b -k 1; include/carmel_hip.h carmel_hip_decoder_*, csrc/decode.hip).

    d = Decoder(wfst, side=0)          # side 0: lines are input strings; 1: output strings (carmel -r)
    best, paths = d.decode(lines)      # lines: sequences of symbol ids of that side's alphabet
    d.set_weights(logw); d.close()

best[l] is the natural log of line l's best path weight (-inf: no derivation); paths[l] its arc ids in path order."""
import ctypes as C

import numpy as np

from ._capi import check, f64, lib, ptr, u32, u64


class Decoder(object):
    def __init__(self, wfst, side=0, device=0):
        self.n_arcs = wfst.n_arcs
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
        lines = [np.asarray(x, dtype=np.uint32) for x in lines]
        off = u64(np.concatenate([[0], np.cumsum([len(x) for x in lines], dtype=np.uint64)]))
        sym = u32(np.concatenate(lines)) if off[-1] else np.zeros(1, np.uint32)
        best = np.empty(len(lines))
        path_off = np.zeros(len(lines) + 1, np.uint64)
        check(lib.carmel_hip_decode(self._h, len(lines), ptr(off), ptr(sym), ptr(best), ptr(path_off)), "carmel_hip_decode")
        arcs = np.zeros(max(int(path_off[-1]), 1), np.uint32)
        check(lib.carmel_hip_decoder_get_paths(self._h, ptr(arcs)), "carmel_hip_decoder_get_paths")
        paths = [arcs[int(path_off[l]):int(path_off[l + 1])].copy() for l in range(len(lines))]
        return best, paths

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
