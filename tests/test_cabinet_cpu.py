"""The cabinet convolver without a GPU: the numpy model of its scheme (tests/cab_model.py)
against a float64 direct sum, and the host side of the feature on host-only engines --
tbf_cabinet_set's return codes, the cabinet calls' refusals, convolution.mix by cfg key, by
control function and by event id, and the mix and the cabinet fingerprint through clone, save
and load."""
import ctypes as C

import numpy as np
import pytest

import cab_model as M

T = pytest.importorskip("tunebfree_amd")

FULL, TONEGEN, TAP_REVERB, FX = 0, 1, 3, 4
TAPS = (1, 128, 129, 300, 2048, 8192)
# every control function name that had an id before convolution.mix was appended, in id order
OLD_NAMES = tuple(f"{m}.drawbar{b}" for m in ("upper", "lower", "pedal")
                  for b in ("16", "513", "8", "4", "223", "2", "135", "113", "1")) + (
    "percussion.enable", "percussion.decay", "percussion.harmonic", "percussion.volume",
    "swellpedal1", "swellpedal2", "vibrato.knob", "vibrato.routing", "vibrato.upper", "vibrato.lower",
    "overdrive.enable", "overdrive.character", "reverb.mix",
    "rotary.speed-preset", "rotary.speed-select", "rotary.speed-toggle",
    "whirl.horn.filter.a.type", "whirl.horn.filter.a.hz", "whirl.horn.filter.a.q", "whirl.horn.filter.a.gain",
    "whirl.horn.filter.b.type", "whirl.horn.filter.b.hz", "whirl.horn.filter.b.q", "whirl.horn.filter.b.gain",
    "whirl.horn.brakepos", "whirl.drum.brakepos", "whirl.horn.acceleration", "whirl.horn.deceleration",
    "whirl.drum.acceleration", "whirl.drum.deceleration")


def _engine(chain=FULL, n=0, cab=None, cfg=None):
    eng = T.Engine(sample_rate=48000.0, device=-1, chain=chain)
    eng.config(cfg or {})
    if cab is not None:
        eng.set_cabinet(cab)
    if n:
        tid = eng.template(seed=7)
        eng.add_instances([tid] * n, [100 + i for i in range(n)])
    return eng


def _set(eng, irL, irR, taps):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return eng._lib.tbf_cabinet_set(eng._h, p(irL), p(irR), taps)


def _err(eng):
    return eng._lib.tbf_last_error().decode()


def _wet(eng, i=0):
    return np.float32(eng.cabinet_info(i)["wet"])


# ---------------------------------------------------------------- the model
@pytest.mark.parametrize("taps", TAPS)
def test_model_accuracy(taps):
    """err <= 4 * 2^-24 against the float64 direct sum on seeded noise through a decaying-noise
    response (a CPU prototype of the scheme measured 0.10 .. 2.91)"""
    nb = 72
    x = np.random.default_rng(1000 + taps).standard_normal(nb * 128).astype(np.float32)
    h = M.decaying_noise(taps, taps)
    e = M.err(M.convolve(x, h), x, h)
    print(f"taps {taps}: err = {e / M.EPS:.3f} * 2^-24")
    assert e <= 4 * M.EPS


@pytest.mark.parametrize("taps", (300, 8192))
def test_model_cut_invariant(taps):
    nb = 70
    x = np.random.default_rng(7).standard_normal(nb * 128).astype(np.float32)
    h = M.decaying_noise(taps, 5)
    one = M.convolve(x, h)
    for cuts in ([1] * nb, [1, 5, 64], [64, 6]):
        assert np.array_equal(one.view(np.uint32), M.convolve(x, h, cuts).view(np.uint32)), cuts


# ---------------------------------------------------------------- tbf_cabinet_set
def test_cabinet_set_codes():
    ir = M.decaying_noise(300, 1)
    eng = _engine()
    assert eng.cabinet_info() == {"taps": 0, "partitions": 0, "instance_bytes": 0, "launches": 0, "wet": None}
    assert _set(eng, None, ir, 300) == -22 and _set(eng, ir, None, 300) == -22
    big = np.zeros(T.params.CAB_MAX_TAPS + 1, np.float32)
    assert _set(eng, big, big, len(big)) == -22
    for bad in (np.nan, np.inf):
        nan = ir.copy()
        nan[123] = bad
        assert _set(eng, ir, nan, 300) == -22 and "123" in _err(eng)
    assert eng.cabinet_info()["taps"] == 0  # a refused call sets nothing
    assert _set(eng, ir, ir, 300) == 0
    info = eng.cabinet_info()
    assert (info["taps"], info["partitions"]) == (300, 3) and info["instance_bytes"] >= 2 * 2 * 128 * 4
    assert _set(eng, big, big, T.params.CAB_MAX_TAPS) == 0 and eng.cabinet_info()["partitions"] == 64
    assert _set(eng, ir, ir, 1) == 0 and eng.cabinet_info()["partitions"] == 1
    assert _set(eng, None, None, 0) == 0 and eng.cabinet_info()["taps"] == 0  # taps 0 clears
    assert _set(eng, ir, ir, 300) == 0
    tid = eng.template(seed=7)
    eng.add_instances([tid], [1])
    assert _set(eng, ir, ir, 300) == -16 and _set(eng, None, None, 0) == -16
    assert eng.cabinet_info()["taps"] == 300
    eng.remove([0])
    assert _set(eng, ir, ir, 300) == -16  # once an instance was added, for good
    eng.close()
    for chain in (TONEGEN, TAP_REVERB):
        eng = _engine(chain)
        assert _set(eng, ir, ir, 300) == -22 and "whirl" in _err(eng)
        eng.close()
    eng = _engine(FX)
    assert _set(eng, ir, ir, 300) == 0
    eng.close()


def test_cabinet_calls_refused_on_host_engines():
    """-19 on a host-only engine with a cabinet, -22 without a cabinet (and on the wrong chain, a
    missing pointer, half a wet pair, a short stride)"""
    ir = M.decaying_noise(300, 1)
    nb, per = 2, 256
    bufs = [np.zeros((2, per), np.float32) for _ in range(9)]
    ptr = [b.ctypes.data for b in bufs]
    co = T.engine.CabinetOut(ptr[0], ptr[1], ptr[2], ptr[3], per)
    ro = T.engine.RotorOut(ptr[4], ptr[5], ptr[6], ptr[7], per)
    for chain in (FULL, FX):
        eng = _engine(chain, n=2, cab=ir)
        lib, h = eng._lib, eng._h
        fx = chain == FX

        def call(co, ro, device=False, nb=nb):
            co = None if co is None else C.byref(co)
            ro = None if ro is None else C.byref(ro)
            if fx:
                return (lib.tbf_process_cabinet_device(h, nb, None, 0, ptr[8], per, co, ro, None) if device else
                        lib.tbf_process_cabinet(h, nb, ptr[8], per, co, ro))
            return (lib.tbf_render_cabinet_device(h, nb, None, 0, co, ro, None) if device else
                    lib.tbf_render_cabinet(h, nb, co, ro))
        for device in (False, True):
            assert call(co, ro, device) == -19
            assert call(co, None, device) == -19
            assert call(None, ro, device) == -22
            assert call(T.engine.CabinetOut(ptr[0], None, None, None, per), None, device) == -22
            assert call(T.engine.CabinetOut(ptr[0], ptr[1], ptr[2], None, per), None, device) == -22
            assert call(T.engine.CabinetOut(ptr[0], ptr[1], None, None, per - 1), None, device) == -22
            assert call(co, T.engine.RotorOut(ptr[4], ptr[5], None, ptr[7], per), device) == -22
            assert call(co, T.engine.RotorOut(ptr[4], ptr[5], ptr[6], ptr[7], per - 1), device) == -22
            assert call(T.engine.CabinetOut(ptr[0], ptr[0], None, None, per), None, device) == -22  # L overlaps R
            assert "overlap" in _err(eng)
            assert call(T.engine.CabinetOut(ptr[0], ptr[1], None, None, per), T.engine.RotorOut(
                ptr[4], ptr[5], ptr[6], ptr[1], per), device) == -22  # a rotor plane overlaps R
        # the other family's calls: wrong chain
        if fx:
            assert lib.tbf_render_cabinet(h, nb, C.byref(co), None) == -22
        else:
            assert lib.tbf_process_cabinet(h, nb, ptr[8], per, C.byref(co), None) == -22
        eng.close()
        eng = _engine(chain, n=2)  # no cabinet
        lib, h = eng._lib, eng._h
        assert call(co, ro) == -22 and "cabinet" in _err(eng)
        assert call(co, ro, True) == -22
        eng.close()


# ---------------------------------------------------------------- convolution.mix
def test_mix_by_cfg_control_and_event_id():
    f32 = np.float32
    want = {0: f32(0.0), 64: f32(64 / 127.0), 127: f32(1.0)}
    assert want[64] == f32(np.float64(64) / np.float64(127)) and want[127] == 1.0
    for cab in (None, M.decaying_noise(300, 1)):  # stored with or without a cabinet
        eng = _engine(n=2, cab=cab)
        assert _wet(eng, 0) == 1.0 and _wet(eng, 1) == 1.0  # the default: a caller who sets a cabinet hears it
        cid = eng.control_id("convolution.mix")
        assert cid == len(OLD_NAMES)
        assert [eng.control_id(nm) for nm in OLD_NAMES] == list(range(len(OLD_NAMES)))
        for v, w in want.items():
            assert eng.midi_control(1, "convolution.mix", v)  # True: applied (the call returned 0)
            assert _wet(eng, 1) == w and _wet(eng, 0) == 1.0
        assert eng.midi_control(1, "convolution.mix", 500) and _wet(eng, 1) == 1.0  # clamped like every control
        # the control changes nothing the chain sees: the 57 fields of tbf_debug_control stay
        out = (C.c_double * 64)()
        eng._lib.tbf_debug_control.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        assert eng._lib.tbf_debug_control(eng._h, 1, out, 64) == 57
        base = list(out)
        assert eng.midi_control(1, "convolution.mix", 40)
        assert eng._lib.tbf_debug_control(eng._h, 1, out, 64) == 57 and list(out) == base
        eng.close()
    # the cfg key: instances added afterwards
    eng = _engine(cfg={"convolution.mix": 0.25})
    tid = eng.template(seed=7)
    eng.add_instances([tid], [1])
    eng.config({"convolution.mix": 1.0})
    eng.add_instances([tid], [2])
    assert _wet(eng, 0) == f32(0.25) and _wet(eng, 1) == 1.0
    for bad in ("-0.1", "1.5", "x"):
        assert eng._lib.tbf_config_set(eng._h, b"convolution.mix", bad.encode()) == -22
    eng.close()


def test_mix_through_clone_save_load_and_cabinet_fingerprint():
    irA, irB = M.decaying_noise(300, 1), M.decaying_noise(301, 1)
    irC = irA.copy()
    irC[17] += np.float32(0.5)  # same length, other taps
    eng = _engine(n=2, cab=irA)
    eng.midi_control(1, "convolution.mix", 64)
    first = eng.clone([1, 0])
    assert _wet(eng, first) == np.float32(64 / 127.0) and _wet(eng, first + 1) == 1.0
    blob = eng.save([1])
    eng.midi_control(1, "convolution.mix", 3)
    eng.load([1], blob)
    assert _wet(eng, 1) == np.float32(64 / 127.0)
    eng.remove([0])
    assert _wet(eng, 0) == np.float32(64 / 127.0) and _wet(eng, 1) == np.float32(64 / 127.0) and _wet(eng, 2) == 1.0
    twin = _engine(n=2, cab=irA)
    twin.load([0], blob)  # an equal cabinet: a migration
    assert _wet(twin, 0) == np.float32(64 / 127.0)
    twin.close()
    for other in (irB, irC, None):
        o = _engine(n=2, cab=other)
        buf = np.frombuffer(blob, np.uint8) if not isinstance(blob, np.ndarray) else blob
        idx = (C.c_uint32 * 1)(0)
        rc = o._lib.tbf_instances_load(o._h, 1, idx, buf.ctypes.data_as(C.c_void_p), buf.nbytes)
        assert rc == -22 and "cabinet" in _err(o), _err(o)
        assert _wet(o, 0) == 1.0
        o.close()
    eng.close()
