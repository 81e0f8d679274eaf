"""Effects-only chains (TBF_CHAIN_FX*), the parts that need no GPU: which entry point works
on which engine, and the effects oracle of the GPU tests (fx_oracle) pinned against the full
chain oracle."""
import ctypes as C

import numpy as np
import pytest

import scenarios as S
import tunebfree_amd as T
from tunebfree_amd import params as P


def _host_engine(chain):
    return T.Engine(sample_rate=48000.0, device=-1, chain=chain)


def test_fx_constants_match_header():
    import re
    from pathlib import Path
    src = (Path(__file__).resolve().parents[1] / "include" / "tbf.h").read_text()
    defs = dict(re.findall(r"#define (TBF_CHAIN_\w+)\s+(\d+)", src))
    assert (int(defs["TBF_CHAIN_FX"]), int(defs["TBF_CHAIN_FX_TAP_PREAMP"]), int(defs["TBF_CHAIN_FX_TAP_REVERB"])) == \
        (P.CHAIN_FX, P.CHAIN_FX_TAP_PREAMP, P.CHAIN_FX_TAP_REVERB) == (4, 5, 6)
    assert int(defs["TBF_CHAIN_FULL"]) == P.CHAIN_FULL == 0
    assert re.search(r"#define TBF_ABI_VERSION 1\b", src)


def test_fx_return_codes_host_only():
    """tbf_process* belong to the effects-only engines (-22 elsewhere; -19 without a device),
    the tbf_render* calls and tbf_synth_sound to the others (-22 on an effects-only engine,
    with an error text that names tbf_process)."""
    lib = T.load_library()
    buf = np.zeros(3 * 128, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    for chain in (P.CHAIN_FX, P.CHAIN_FX_TAP_PREAMP, P.CHAIN_FX_TAP_REVERB):
        fx = _host_engine(chain)
        assert lib.tbf_process_device(fx._h, 1, p, 128, C.c_void_p(buf.ctypes.data + 512),
                                      C.c_void_p(buf.ctypes.data + 1024), 128, None) == -19
        assert lib.tbf_process_events(fx._h, 1, None, 0, p, 128, C.c_void_p(buf.ctypes.data + 512),
                                      C.c_void_p(buf.ctypes.data + 1024), 128, None) == -19
        ofs = lambda k: C.cast(buf.ctypes.data + 512 * k, C.POINTER(C.c_float))
        assert lib.tbf_process(fx._h, 1, fp, 128, ofs(1), ofs(2), 128) == -19
        for rc in (lib.tbf_render_device(fx._h, 1, p, p, 128, None),
                   lib.tbf_render_events(fx._h, 1, None, 0, p, p, 128, None),
                   lib.tbf_render(fx._h, 1, fp, fp, 128),
                   lib.tbf_synth_sound(fx._h, 128, fp, fp, 128)):
            assert rc == -22
            assert b"tbf_process" in lib.tbf_last_error()
        fx.close()
    for chain in (P.CHAIN_FULL, P.CHAIN_TONEGEN, P.CHAIN_TAP_PREAMP, P.CHAIN_TAP_REVERB):
        full = _host_engine(chain)
        assert lib.tbf_process_device(full._h, 1, p, 128, C.c_void_p(buf.ctypes.data + 512),
                                      C.c_void_p(buf.ctypes.data + 1024), 128, None) == -22
        assert lib.tbf_render_device(full._h, 1, p, p, 128, None) == -19  # as before
        full.close()


def test_fx_engine_keeps_the_control_plane():
    """An effects-only engine takes the whole control surface: the instance protocol, effect
    parameters, MIDI control functions, cfg keys, and the tone-generator-facing calls
    (accepted, not given error paths of their own)."""
    fx = _host_engine(P.CHAIN_FX)
    assert fx.config_set("reverb.mix", 0.3) == 0
    tid = fx.template(seed=7)
    assert fx.add_instances([tid, tid], [11, 12]) == 0 and fx.n_instances == 2
    fx.set_param(0, P.OVERDRIVE, 1)
    fx.set_param(1, P.CHARACTER, 0.7)
    fx.set_param(1, P.REVERB, 0.4)
    fx.set_param(0, P.HORN, 2)
    fx.note(0, 60, 1)
    fx.set_param(0, P.DRAWBAR_MIN + 2, 5)
    fx.set_param(0, P.VIBRATO, 1)
    assert fx.midi_control(1, "whirl.horn.brakepos", 64)
    fx.retune(1, fx.template(seed=8))
    assert fx.launches() == {k: 0 for k in T.engine.LAUNCH_KINDS}
    with pytest.raises(T.TbfError):
        fx.process(np.zeros((2, 128), np.float32))  # no device
    fx.close()


def _fx_sweep(i):
    """sweep_scenario with overdrive toggles and a character change past its own events"""
    return S.sweep_scenario(i) + [(33, "param", S.P_CHARACTER, 0.45), (35, "param", S.P_OVERDRIVE, 0),
                                  (38, "param", S.P_OVERDRIVE, 1)]


def test_fx_oracle_pins_itself(oracle):
    """The effects oracle guards itself: fed the chain oracle's tone-generator tap, with the
    scenario's effect events, it gives the chain oracle's preamp, reverb, L and R taps bit for
    bit (3 seeds x 40 blocks: rotor changes, overdrive on / off, character, mix sweeps; the
    tap has the silences that reach the preamp's denormal guard)."""
    from enginerun import assert_bits
    from fx_oracle import effect_events, fx_run
    from orc_bind import Chain, Template
    tpl = Template(oracle, 48000.0, seed=1)
    nb = 40
    for i, seed in ((0, 11), (1, 12345), (6, 99)):  # sweep_scenario (6) starts clean
        sc = _fx_sweep(i)
        L, R, A, B, Cc = S.run(Chain(oracle, tpl, seed), sc, nb, stages=True)
        pre, rev, l, r = fx_run(oracle, [seed], A[None, :], [effect_events(sc)])
        for got, ref, what in ((pre, B, "preamp"), (rev, Cc, "reverb"), (l, L, "L"), (r, R, "R")):
            assert_bits(got[0], ref, f"fx_oracle seed {seed} {what}")
        assert float(np.abs(L).max()) > 1e-3 and (A == 0).any()
