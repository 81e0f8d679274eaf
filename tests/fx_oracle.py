"""A per-instance effects oracle for the effects-only chains (TBF_CHAIN_FX*): the CPU
oracle's own stage entry points (oracle/orc.h, orc_internal.h) in the order an instance is
built and run,

    srand (seed) -> allocReverb -> allocPreamp          (the draws of orc_inst_new_cfg)
    per block: preamp -> b_reverb::reverb -> whirlProc3

on caller-supplied audio.  orc_whirl_new takes no cfg, so whirl cfg keys, the whirl's MIDI
control functions and bypass are not covered here: tests of those feed the full Chain
oracle's tone-generator tap back in and compare with its other taps.

TEST INFRASTRUCTURE ONLY (like orc_bind, whose signatures it leaves alone: it sets its own).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

import scenarios as S

_fp = C.POINTER(C.c_float)

# the parameters that reach the effects (the rest face the tone generator)
FX_PARAMS = (S.P_DRUM, S.P_HORN, S.P_OVERDRIVE, S.P_CHARACTER, S.P_REVERB, S.P_WHIRL_BYPASS)


def effect_events(scen):
    """the events of a scenario that reach preamp, reverb or whirl: effect parameters and
    MIDI control functions (every hot-path control name of the scenarios is a whirl's)"""
    return [e for e in scen if (e[1] == "param" and e[2] in FX_PARAMS) or e[1] == "control"]


def _bind(lib):
    if getattr(lib, "_fx_bound", False):
        return lib
    lib.orc_srand.argtypes = [C.c_void_p, C.c_uint]
    lib.orc_reverb_alloc.restype = C.c_void_p
    lib.orc_reverb_alloc.argtypes = [C.c_void_p, C.c_double]
    lib.orc_preamp_new.restype = C.c_void_p
    lib.orc_preamp_new.argtypes = [C.c_double, C.c_uint]
    lib.orc_preamp_init.restype = None
    lib.orc_preamp_init.argtypes = [C.c_void_p, C.c_void_p, C.c_double]
    lib.orc_whirl_new.restype = C.c_void_p
    lib.orc_whirl_new.argtypes = [C.c_double]
    lib.orc_preamp_set.argtypes = [C.c_void_p, C.c_int, C.c_float]
    lib.orc_reverb_set_mix.argtypes = [C.c_void_p, C.c_float]
    lib.orc_whirl_rev_option.argtypes = [C.c_void_p, C.c_int]
    lib.orc_preamp_proc.argtypes = [C.c_void_p, _fp, _fp, C.c_int]
    lib.orc_reverb_proc.argtypes = [C.c_void_p, _fp, _fp, C.c_int]
    lib.orc_whirl_proc3.argtypes = [C.c_void_p, _fp, _fp, _fp, C.c_int]
    for f in ("orc_preamp_free", "orc_reverb_free", "orc_whirl_free"):
        getattr(lib, f).restype = None
        getattr(lib, f).argtypes = [C.c_void_p]
    lib._fx_bound = True
    return lib


class FxOracle:
    """One instance's preamp, reverb and whirl with the state of seed `seed`."""

    def __init__(self, lib, seed, sr=48000.0):
        self.lib = _bind(lib)
        rnd = C.create_string_buffer(256)  # an orc_rand (31 + 2 ints)
        lib.orc_srand(rnd, int(seed))
        self.rv = lib.orc_reverb_alloc(rnd, float(sr))
        self.pre = lib.orc_preamp_new(float(sr), 0)
        lib.orc_preamp_init(self.pre, rnd, float(sr))  # the stream after the reverb's draws
        self.wh = lib.orc_whirl_new(float(sr))
        self.clean, self.char, self.drum, self.horn = 1, 0.0, 1.0, 1.0

    def param(self, pid, v):
        """a CLAP parameter as orc_set_param / tbf_set_param applies it; one that faces the
        tone generator changes nothing"""
        lib = self.lib
        if pid == S.P_REVERB:
            lib.orc_reverb_set_mix(self.rv, float(v))
        elif pid == S.P_OVERDRIVE:
            self.clean = int(round(1.0 - v))
            lib.orc_preamp_set(self.pre, self.clean, self.char)
        elif pid == S.P_CHARACTER:
            self.char = float(v)
            lib.orc_preamp_set(self.pre, self.clean, self.char)
        elif pid in (S.P_DRUM, S.P_HORN):
            if pid == S.P_DRUM:
                self.drum = float(v)
            else:
                self.horn = float(v)
            lib.orc_whirl_rev_option(self.wh, int(math.floor(self.drum) + 3 * math.floor(self.horn)))
        elif pid == S.P_WHIRL_BYPASS:
            raise ValueError("whirl bypass is not reachable through orc_whirl_new: use the Chain oracle")

    def block(self, x):
        """128 samples -> (preamp, reverb, L, R)"""
        x = np.ascontiguousarray(x, np.float32)
        assert x.shape == (128,)
        b, c, l, r = (np.zeros(128, np.float32) for _ in range(4))
        p = lambda a: a.ctypes.data_as(_fp)
        self.lib.orc_preamp_proc(self.pre, p(x), p(b), 128)
        self.lib.orc_reverb_proc(self.rv, p(b), p(c), 128)
        self.lib.orc_whirl_proc3(self.wh, p(c), p(l), p(r), 128)
        return b, c, l, r

    def close(self):
        if self.pre:
            self.lib.orc_preamp_free(self.pre)
            self.lib.orc_reverb_free(self.rv)
            self.lib.orc_whirl_free(self.wh)
            self.pre = self.rv = self.wh = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fx_run(lib, seeds, x, scens, sr=48000.0):
    """x [n, nblocks*128] through one FxOracle per row, with the rows' scenarios ("param"
    events only; notes and tone-generator parameters pass and change nothing) applied at
    their block boundaries: [preamp, reverb, L, R], each [n, nblocks*128]."""
    x = np.ascontiguousarray(x, np.float32)
    n, ns = x.shape
    assert ns % 128 == 0 and len(seeds) == n and len(scens) == n
    out = [np.zeros_like(x) for _ in range(4)]
    for i in range(n):
        o = FxOracle(lib, seeds[i], sr)
        by = {}
        for (b, kind, a, v) in scens[i]:
            if kind == "param":
                by.setdefault(b, []).append((a, v))
            elif kind != "note":
                raise ValueError(f"fx_run: {kind} events need the Chain oracle")
        for b in range(ns // 128):
            for (a, v) in by.get(b, []):
                o.param(a, v)
            for dst, blk in zip(out, o.block(x[i, b * 128:(b + 1) * 128])):
                dst[i, b * 128:(b + 1) * 128] = blk
        o.close()
    return out
