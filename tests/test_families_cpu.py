"""The cabinet convolver and the rate converter set on one engine, without a GPU, on host-only
engines: a blob loads only into an engine with the same two features, a refused load changes
nothing, and the two features' host state (the mix and the position P) travels together through
clone, save / load and remove."""
import ctypes as C

import numpy as np
import pytest

import cab_model as CM

T = pytest.importorskip("tunebfree_amd")

IR = (CM.decaying_noise(300, 600), CM.decaying_noise(300, 601))
FO = 22050
KINDS = {"neither": (None, None), "cabinet": (IR, None), "converter": (None, FO), "both": (IR, FO)}


def _engine(kind, n=2):
    ir, fo = KINDS[kind]
    eng = T.Engine(sample_rate=48000.0, device=-1)
    if ir is not None:
        eng.set_cabinet(*ir)
    if fo is not None:
        eng.set_output_rate(fo)
    tid = eng.template(seed=7)
    eng.add_instances([tid] * n, [100 + i for i in range(n)])
    return eng


def _load(eng, inst, blob):
    a = np.array([inst], np.uint32)
    b = np.ascontiguousarray(blob, np.uint8)
    return eng._lib.tbf_instances_load(eng._h, 1, a.ctypes.data_as(C.POINTER(C.c_uint32)), b.ctypes.data, b.nbytes)


def _err(eng):
    return eng._lib.tbf_last_error().decode()


def _wet(eng, i):
    return np.float32(eng.cabinet_info(i)["wet"])


def blob(eng, i):
    return eng.save([i]).tobytes()


def test_a_blob_loads_only_into_the_engine_that_wrote_it():
    """4 x 4 pairings: the own blob loads; every other one is refused with the first differing
    header field in the error text, and leaves the target's P and mix as they were"""
    f32 = np.float32
    engines = {k: _engine(k) for k in KINDS}
    blobs = {}
    for k, eng in engines.items():
        eng.resampler_pos(0, 1000 + len(k))
        assert eng.midi_control(0, "convolution.mix", 30)
        blobs[k] = eng.save([0])
    for dst, eng in engines.items():
        eng.resampler_pos(1, 77)
        assert eng.midi_control(1, "convolution.mix", 90)
        before = blob(eng, 1)
        for src in KINDS:
            if src == dst:
                continue
            assert _load(eng, 1, blobs[src]) == -22, (src, dst)
            cab_differs = (KINDS[src][0] is None) != (KINDS[dst][0] is None)
            field = "cabinet response length (tbf_cabinet_set)" if cab_differs else "resampler output rate (tbf_resampler_set)"
            assert _err(eng) == "blob does not match this engine: " + field, (src, dst, _err(eng))
            assert blob(eng, 1) == before and _wet(eng, 1) == f32(90 / 127.0), (src, dst)  # P is in the blob
        assert _load(eng, 1, blobs[dst]) == 0, (dst, _err(eng))
        assert blob(eng, 1) == blobs[dst].tobytes() != before and _wet(eng, 1) == f32(30 / 127.0)
    for eng in engines.values():
        eng.close()


def test_position_and_mix_travel_together_on_the_engine_with_both():
    """as test_resample_cpu's test_position_travels_with_clone_save_load_and_remove, with a cabinet
    set beside the converter: P is visible through the blob, the mix through tbf_debug_cabinet"""
    f32 = np.float32
    eng = _engine("both", n=3)
    eng.resampler_pos(1, 12345)
    assert eng.midi_control(1, "convolution.mix", 40)
    c = eng.clone([1])
    assert c == 3 and blob(eng, c) == blob(eng, 1) != blob(eng, 0)
    assert _wet(eng, c) == f32(40 / 127.0) and _wet(eng, 0) == f32(1.0)
    saved = eng.save([1])
    eng.resampler_pos(1, 5)
    assert blob(eng, 1) != saved.tobytes()          # P alone changes the blob
    eng.resampler_pos(1, 12345)
    assert blob(eng, 1) == saved.tobytes()
    assert eng.midi_control(1, "convolution.mix", 100)
    assert blob(eng, 1) != saved.tobytes()          # and so does the mix alone
    eng.resampler_pos(1, 5)
    eng.load([1], saved)
    assert blob(eng, 1) == saved.tobytes() and _wet(eng, 1) == f32(40 / 127.0)
    assert eng.remove([0]).tolist() == [-1, 0, 1, 2]
    assert blob(eng, 0) == saved.tobytes() == blob(eng, 2) and _wet(eng, 0) == f32(40 / 127.0)
    assert _wet(eng, 1) == f32(1.0) and blob(eng, 1) != saved.tobytes()
    eng.close()
