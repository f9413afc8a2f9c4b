"""Captures whose CCK payload sits on ties, for the 802.11b receive handle (tests/test_gpu_11b_ties.py): the long-preamble 5.5 and 11 Mbps captures of
stage11b_captures.captures() at 33 and 120 bytes and one short-preamble 11 Mbps capture, with the payload overwritten from its first chip on by tied_chips of
tests/test_11b_stage_model_cpu.py, every chip held for four samples on the receiver's decimation grid.  The strict comparisons of the code-word tree then decide
bits, and since a held chip gives the four sampling phases of a block equal energies, AdjustTiming sits on its ties too.  The FCS fails, which is intended: an
E_CRC32_FAIL row still delivers every MPDU byte and the FCS word.  TEST INFRASTRUCTURE."""
import functools

import numpy as np

import rx11b_stage_model as sm
import stage11b_captures as sc
from sora_amd import capi
from test_11b_stage_model_cpu import tied_chips

NAMES = ("long-5500-33", "long-5500-120", "long-11000-33", "long-11000-120", "short-11000-33")
SEED = 1917


class _Walk(sm.ModelOps):
    """the model's bricks under capi.rx11b_stages, keeping where the payload's first chip came from"""

    def __init__(self):
        self.dc = self.sym_first = self.mi = self.pay = None

    def dc_remove(self, x, first, n, out_first, dc, out):
        self.dc = int(np.asarray(dc).view(np.uint32)[0])
        super().dc_remove(x, first, n, out_first, dc, out)

    def symtiming(self, x, first, n, out_first, state, out):
        a, k = int(self._u(first)[0]), int(self._u(n)[0])
        _, _, tr = sm.symtiming(x[a:a + 28 * k], np.array(state[0], np.int32), trace=True)
        self.sym_first = a
        self.mi = np.concatenate([[int(np.array(state[0], np.int32)[0])], tr[:-1]]).astype(np.int64)       # m_index as each block finds it
        return super().symtiming(x, first, n, out_first, state, out)

    def stream_stage(self, kind, x, first, n, out_first, state, out):
        if kind.startswith("cck"):
            a, k = int(self._u(first)[0]), int(self._u(n)[0])
            self.pay = (kind, a, k, x[a:a + sm.PER[kind] * k].copy())
        return super().stream_stage(kind, x, first, n, out_first, state, out)


def _walk(iq, mode):
    w = _Walk()
    capi.rx11b_stages(w, iq, [(0, len(iq))], mode)
    return w


def _chip_sample(w, chip):
    """-> (sample of the capture that chip number `chip` behind TSymTiming was read from, m_index of its block): Decimation (symtiming.hpp:66-83)"""
    at = 0
    for b, mi in enumerate(w.mi):
        mi = int(mi)
        idx = [max(i, 0) for i in range(mi, 28, 4)] if mi >= 0 else [0] + list(range(mi + 4, 28, 4))
        if chip < at + len(idx):
            return w.sym_first + 28 * b + idx[chip - at], mi
        at += len(idx)
    raise AssertionError("chip %d lies behind the capture" % chip)


class TieCap:
    def __init__(self, name, iq, mode, planted, frame_at):
        self.name, self.iq, self.mode, self.planted, self.frame_at = name, iq, mode, planted, frame_at


@functools.lru_cache(maxsize=None)
def captures():
    good, _ = sc.captures()
    rng = np.random.default_rng(SEED)
    out = []
    for name in NAMES:
        c = next(g for g in good if g.name == name)
        mode = 1 if c.preamble else 0
        w = _walk(c.iq, mode)
        kind, chip0, nbytes, _ = w.pay
        s0, mi = _chip_sample(w, chip0)
        assert 0 <= mi <= 4, (name, mi)                                 # (a block that Decimation enters at -1 reads sample 0 twice: no grid to hold a chip on)
        q = s0 - (mi & 3)                                               # the 4-sample cell of the payload's first chip
        assert (q - w.sym_first) % 4 == 0
        chips = tied_chips(rng, nbytes * sm.PER[kind] // 8).astype(np.int64)
        dc = np.array([np.int16(np.uint16(w.dc & 0xFFFF)), np.int16(np.uint16(w.dc >> 16))], np.int64)
        held = np.repeat(((chips + dc + 32768) % 65536 - 32768).astype(np.int16), 4, axis=0)       # TDCRemove in front of the chips takes dc off again, wrapping
        iq = c.iq.copy()
        assert q + len(held) <= len(iq), name
        iq[q:q + len(held)] = held
        frame_at = int(np.argmax(np.abs(c.iq.astype(np.int64)).sum(1) > 2000))      # the frame's first samples (96 x 127 against noise of sigma <= 20)
        out.append(TieCap(name, iq, mode, chips.astype(np.int16), frame_at))
    return out


def reaching_the_decoder(cap):
    """the chips the model's CCK decoder is given on this capture (the walk of capi.rx11b_stages with the model's bricks)"""
    return _walk(cap.iq, cap.mode).pay[3]
