"""Whirl outputs beyond the mic mix, CPU side: the committed rotor vectors
(tests/golden/rotor_vectors.npz, the reference's whirlProc2 with all six outputs) tie to the
committed ref_vectors, and the C ABI's whirl_out field and tbf_*_rotors* calls refuse what they
must, on host-only engines."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

T = pytest.importorskip("tunebfree_amd")

GOLD = Path(__file__).resolve().parent / "golden"
FULL, TONEGEN, TAP_PREAMP, TAP_REVERB, FX, FX_TAP_PREAMP, FX_TAP_REVERB = range(7)


def load_rotor_vectors():
    with np.load(GOLD / "rotor_vectors.npz") as z:
        out = {k: z[k] for k in z.files if k != "cases"}
        return out, json.loads(str(z["cases"]))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def mic_mix(m, HL, HR, DL, DR):
    """whirlProc3's mix (src/whirl.cpp:1676-1680) in float32, left to right; m = hll hlr dll dlr
    hrl hrr drl drr"""
    m = np.asarray(m, np.float32)
    L = ((HL * m[0] + HR * m[1]) + DL * m[2]) + DR * m[3]
    R = ((HL * m[4] + HR * m[5]) + DL * m[6]) + DR * m[7]
    return L.astype(np.float32), R.astype(np.float32)


def test_rotor_vectors_tie_to_ref_vectors():
    """The mic mix of the archive's four rotor streams is the committed whirlProc3 output of the
    same case, bit for bit (for the case with its own cfg there is none: its streams are finite,
    audible and not the base case's); one case per ring window, one with a rotary change."""
    from golden.make_ref_vectors import load_vectors, scenario
    import scenarios as S
    vec, cases = load_rotor_vectors()
    ref = load_vectors()
    table = {t["name"]: t for t in json.loads(str(ref["cases"]))}
    assert sorted(c["window"] for c in cases if not c["cfg"]) == [512, 1024, 2048]
    assert any(c["cfg"] for c in cases)
    changes = 0
    for c in cases:
        name, base = c["name"], table[c["base"]]
        six = [vec[f"{name}/{k}"] for k in ("L", "R", "HL", "HR", "DL", "DR")]
        assert all(a.dtype == np.float32 and a.shape == (base["nblocks"] * 128,) for a in six), name
        assert all(np.isfinite(a).all() and float(np.abs(a).max()) > 1e-3 for a in six), name
        eng = T.Engine(sample_rate=base["sr"], device=-1)
        eng.config(c["cfg"])
        assert eng.layout()["wring_len"] == c["window"], name
        eng.close()
        L, R = mic_mix(c["mic"], *six[2:])
        if not c["cfg"]:
            assert np.array_equal(bits(L), bits(ref[f"{c['base']}/L"])), name
            assert np.array_equal(bits(R), bits(ref[f"{c['base']}/R"])), name
        else:
            assert base["sr"] == 48000.0 and set(c["cfg"]) == {"whirl.horn.level", "whirl.horn.leak"}
            assert not np.array_equal(bits(L), bits(ref[f"{c['base']}/L"])), name
        # whirlProc's direct sum is not the default-width mic mix: the association differs
        assert (bits(six[0]) != bits(L)).sum() > len(L) // 10, name
        changes += sum(1 for (b, k, a, _v) in scenario(*base["scenario"]) if b > 0 and k == "param" and a == S.P_HORN)
    assert changes > 0


def _create(device=-1, chain=FULL, whirl_out=0):
    lib = T.load_library()
    cfg = T.engine._Config(48000.0, device, chain, 0, whirl_out)
    h = C.c_void_p()
    rc = lib.tbf_engine_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        lib.tbf_engine_destroy(h)
    return rc


def test_whirl_out_field_and_refusals():
    assert C.sizeof(T.engine._Config) == 32  # double + 3 words + the 3 words that were reserved[3]
    assert T.engine._Config.whirl_out.offset == 20 and T.engine._Config.reserved.offset == 24
    assert (T.params.WHIRL_OUT_MIC, T.params.WHIRL_OUT_DIRECT) == (0, 1)
    assert _create(whirl_out=0) == 0
    assert _create(whirl_out=1) == 0 and _create(chain=FX, whirl_out=1) == 0  # host-only engines take the field
    assert _create(whirl_out=2) == -22 and _create(whirl_out=0xFFFFFFFF) == -22
    for chain in (TONEGEN, TAP_PREAMP, TAP_REVERB, FX_TAP_PREAMP, FX_TAP_REVERB):
        assert _create(chain=chain, whirl_out=0) == 0
        assert _create(chain=chain, whirl_out=1) == -22, chain
    with pytest.raises(T.TbfError, match="-22"):
        T.Engine(device=-1, chain=TONEGEN, whirl_out=1)


def _rotor_calls(eng, nb, L, R, stride, ro, x=None):
    """the four rotor calls' return codes on the engine's chain kind: (host call, device call)"""
    lib, h = eng._lib, eng._h
    ro = None if ro is None else C.byref(ro)
    if x is None:
        return (lib.tbf_render_rotors(h, nb, L, R, stride, ro),
                lib.tbf_render_rotors_device(h, nb, None, 0, L, R, stride, ro, None))
    return (lib.tbf_process_rotors(h, nb, x, stride, L, R, stride, ro),
            lib.tbf_process_rotors_device(h, nb, None, 0, x, stride, L, R, stride, ro, None))


@pytest.mark.parametrize("chain", [FULL, FX])
def test_rotor_calls_validate_before_anything_else(chain):
    """On a host-only engine every malformed call is -22 and a well-formed one -19: the
    arguments are judged before the engine is asked whether it can render."""
    RotorOut = T.engine.RotorOut
    eng = T.Engine(device=-1, chain=chain, whirl_out=1)
    tid = eng.template(seed=3)
    eng.add_instances([tid] * 2, [5, 6])
    nb, per = 3, 3 * 128
    bufs = [np.zeros((2, per), np.float32) for _ in range(7)]
    p = [b.ctypes.data for b in bufs]
    x = p[6] if chain == FX else None
    good = RotorOut(p[2], p[3], p[4], p[5], per)
    assert _rotor_calls(eng, nb, p[0], p[1], per, good, x) == (-19, -19)
    assert _rotor_calls(eng, nb, None, None, per, good, x) == (-19, -19)  # L / R: both or neither
    assert _rotor_calls(eng, nb, p[0], None, per, good, x) == (-22, -22)
    assert _rotor_calls(eng, nb, None, p[1], per, good, x) == (-22, -22)
    assert _rotor_calls(eng, nb, p[0], p[1], per, None, x) == (-22, -22)
    for k in range(4):
        q = p[2:6]
        q[k] = None
        assert _rotor_calls(eng, nb, p[0], p[1], per, RotorOut(*q, per), x) == (-22, -22), k
    assert _rotor_calls(eng, nb, p[0], p[1], per, RotorOut(*p[2:6], per - 1), x) == (-22, -22)
    assert _rotor_calls(eng, nb, p[0], p[1], per - 1, good, x) == (-22, -22)
    assert "stride" in eng._lib.tbf_last_error().decode()
    # the other chain kind's calls
    other = _rotor_calls(eng, nb, p[0], p[1], per, good, None if chain == FX else p[6])
    assert other == (-22, -22)
    if chain == FX:  # an input range overlapping any of the six outputs
        for k in range(6):
            assert _rotor_calls(eng, nb, p[0], p[1], per, good, p[k] + 4 * (per - 1)) == (-22, -22), k
        assert "overlap" in eng._lib.tbf_last_error().decode()
        assert _rotor_calls(eng, nb, None, None, per, good, p[0]) == (-19, -19)  # no L / R: nothing to overlap there
    eng.close()


@pytest.mark.parametrize("chain", [TONEGEN, TAP_PREAMP, TAP_REVERB, FX_TAP_PREAMP, FX_TAP_REVERB])
def test_rotor_calls_need_the_whirl(chain):
    eng = T.Engine(device=-1, chain=chain)
    bufs = [np.zeros((1, 128), np.float32) for _ in range(7)]
    p = [b.ctypes.data for b in bufs]
    ro = T.engine.RotorOut(p[2], p[3], p[4], p[5], 128)
    assert _rotor_calls(eng, 1, p[0], p[1], 128, ro) == (-22, -22)
    assert _rotor_calls(eng, 1, p[0], p[1], 128, ro, p[6]) == (-22, -22)
    assert "whirl" in eng._lib.tbf_last_error().decode()
    eng.close()
