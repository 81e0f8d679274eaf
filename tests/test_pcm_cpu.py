"""The PCM output stage without a GPU: the host restatement of the definition
(tbf_debug_pcm_ref, built from the header k_pcm is built from) against the numpy model in bytes
and meters, the dither's statistics and its 64-bit frame counter, and the refusals of the PCM
calls on host-only engines."""
import ctypes as C

import numpy as np
import pytest

import pcm_model as M

T = pytest.importorskip("tunebfree_amd")
E = T.engine

FULL, TONEGEN, FX = 0, 1, 4


def _engine(chain=FULL, n=2):
    eng = T.Engine(sample_rate=48000.0, device=-1, chain=chain)
    if n:
        tid = eng.template(seed=7)
        eng.add_instances([tid] * n, [100 + i for i in range(n)])
    return eng


def _err(eng):
    return eng._lib.tbf_last_error().decode()


def _meter(m):
    return (np.float32(m["peakL"]), np.float32(m["peakR"]), int(m["clipL"]), int(m["clipR"]))


def _same_meter(got, want, what):
    got = _meter(got)
    assert (got[0].view(np.uint32), got[1].view(np.uint32), got[2], got[3]) == (
        np.float32(want[0]).view(np.uint32), np.float32(want[1]).view(np.uint32), want[2], want[3]), (what, got, want)


# ---------------------------------------------------------------- 1. the restatement against the model
def test_constants_mirror_the_header():
    assert (T.params.PCM_S16, T.params.PCM_S24_3LE, T.params.PCM_F32, T.params.PCM_DITHER) == (M.S16, M.S24, M.F32, M.DITHER)
    assert tuple(T.params.PCM_FRAME_BYTES) == tuple(M.FRAME_BYTES) == tuple(E.PCM_FRAME_BYTES)
    assert E.METER_DTYPE.itemsize == 16 and C.sizeof(E.PcmOut) == 56


@pytest.mark.parametrize("fmt,flags", M.FORMATS)
def test_ref_against_model_on_crafted_rows(fmt, flags):
    L, R = M.crafted()
    assert len(L) > 1000 and np.isnan(L).sum() == 3 and np.isinf(L).sum() == 2
    for n in (len(L), len(L) - 1, 5, 2, 1, 0):  # odd and even counts: the packed 24-bit tail
        for row, frame0, seed in ((0, 0, 0), (3, 12345, 0xDEADBEEF)):
            got, meter = T.Engine.pcm_ref(fmt, L[:n], R[:n], flags, seed, row, frame0)
            want, wmeter = M.convert(fmt, L[:n], R[:n], flags, seed, row, frame0)
            assert got.view(np.uint8).reshape(-1).tobytes() == want.tobytes(), (fmt, flags, n, row)
            _same_meter(meter, wmeter, (fmt, flags, n, row))


def test_ref_values_of_the_edge_cases():
    """what the definition says outright, independent of the model: 1.0 clips to max, -1.0 is
    min unclipped, ties go to even, NaN is 0 and a clip, F32 keeps every bit"""
    S = 32768.0
    x = np.array([1.0, -1.0, 1.0 - 2.0 ** -15, 0.5 / S, 1.5 / S, 2.5 / S, -0.5 / S, 1.22, np.inf, -np.inf, np.nan, -0.0],
                 np.float32)
    z = np.zeros_like(x)
    got, m = T.Engine.pcm_ref(M.S16, x, z)
    assert got[:, 0].tolist() == [32767, -32768, 32767, 0, 2, 2, 0, 32767, 32767, -32768, 0, 0]
    assert not got[:, 1].any()
    assert _meter(m) == (np.float32(np.inf), np.float32(0), 5, 0)  # 1.0, 1.22, +inf, -inf, NaN
    got, m = T.Engine.pcm_ref(M.S24, z, x)
    b = got.reshape(-1, 6)[:, 3:].astype(np.int32)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    v = np.where(v >= 1 << 23, v - (1 << 24), v)
    assert v.tolist() == [8388607, -8388608, 8388352, 128, 384, 640, -128, 8388607, 8388607, -8388608, 0, 0]
    assert _meter(m)[2:] == (0, 5)
    L, R = M.crafted()
    got, m = T.Engine.pcm_ref(M.F32, L, R)
    assert got.view(np.uint32)[:, 0].tobytes() == L.tobytes() and got.view(np.uint32)[:, 1].tobytes() == R.tobytes()
    with np.errstate(invalid="ignore"):
        assert int(m["clipL"]) == int((~(np.abs(L) <= 1)).sum()) == int(m["clipR"]) == 8  # +-1.22, +-inf, three NaNs, -(1 + 2^-16)


def test_ref_refuses_bad_formats_and_flags():
    lib = T.load_library()
    x = np.zeros(4, np.float32)
    out = np.zeros(64, np.uint8)

    def ref(fmt, flags):
        f = lib.tbf_debug_pcm_ref
        f.restype = C.c_int
        f.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                      C.c_void_p, C.c_void_p]
        return f(fmt, flags, 0, 0, 0, x.ctypes.data, x.ctypes.data, 4, out.ctypes.data, None)
    assert ref(M.S16, 0) == 0 and ref(M.S16, M.DITHER) == 0
    assert ref(3, 0) == -22 and ref(M.S16, 2) == -22
    assert ref(M.S24, M.DITHER) == -22 and ref(M.F32, M.DITHER) == -22


# ---------------------------------------------------------------- 2. dither
def test_dither_statistics_on_silence():
    """2^16 frames of silence: q = rint (d) with |d| < 1, a triangular density: values in
    {-1, 0, 1}, P(+-1) = 1/8 each, so the variance of a sample is 1/4; the mean within 3 standard
    errors of 0; the two channels carry different streams"""
    n = 1 << 16
    z = np.zeros(n, np.float32)
    got, m = T.Engine.pcm_ref(M.S16, z, z, M.DITHER, seed=2024, row=1, frame0=0)
    want, _ = M.convert(M.S16, z, z, M.DITHER, seed=2024, row=1, frame0=0)
    assert got.view(np.uint8).reshape(-1).tobytes() == want.tobytes()
    assert _meter(m) == (np.float32(0), np.float32(0), 0, 0)
    se = 0.5 / np.sqrt(n)
    for c in (0, 1):
        v = got[:, c].astype(np.int64)
        assert set(np.unique(v).tolist()) == {-1, 0, 1}
        print(f"channel {c}: mean {v.mean():+.5f} (3 standard errors: {3 * se:.5f}), share of +-1 {np.mean(v != 0):.4f}")
        assert abs(v.mean()) <= 3 * se
        assert abs(np.mean(v != 0) - 0.25) < 0.02
    assert np.mean(got[:, 0] != got[:, 1]) > 0.2
    other, _ = T.Engine.pcm_ref(M.S16, z, z, M.DITHER, seed=2024, row=2, frame0=0)
    assert np.mean(other[:, 0] != got[:, 0]) > 0.2  # another row, another stream


def test_dither_frame_counter_is_64_bit():
    """frame0 straddling 2^32: the same bytes as the model, the same bytes when the row is cut
    at the crossing with frame0 carried, and other bytes than the stream 2^32 frames earlier"""
    n, f0 = 512, (1 << 32) - 200
    x = (np.random.default_rng(9).standard_normal(n) * 0.01).astype(np.float32)
    y = x[::-1].copy()
    got, _ = T.Engine.pcm_ref(M.S16, x, y, M.DITHER, seed=77, row=5, frame0=f0)
    want, _ = M.convert(M.S16, x, y, M.DITHER, seed=77, row=5, frame0=f0)
    assert got.view(np.uint8).reshape(-1).tobytes() == want.tobytes()
    parts = [T.Engine.pcm_ref(M.S16, x[a:b], y[a:b], M.DITHER, seed=77, row=5, frame0=f0 + a)[0]
             for a, b in ((0, 199), (199, 200), (200, 201), (201, n))]
    assert np.array_equal(np.concatenate(parts), got)
    wrapped, _ = T.Engine.pcm_ref(M.S16, x[200:], y[200:], M.DITHER, seed=77, row=5, frame0=(f0 + 200) & 0xFFFFFFFF)
    assert np.mean(wrapped != got[200:]) > 0.1  # hi32 (f) takes part


# ---------------------------------------------------------------- 3. refusals on host-only engines
def _pcm_out(n, frames, fmt=M.S16, flags=0, meters=True):
    out = np.zeros((n, frames * M.FRAME_BYTES[fmt] + 16), np.uint8)
    m = np.zeros(n, E.METER_DTYPE)
    po = E.PcmOut(out.ctypes.data, out.shape[1], m.ctypes.data if meters else None, fmt, flags, 0, 0, None)
    return po, (out, m)


def test_pcm_calls_refused_on_host_engines():
    """-22 for a bad format or flag, dither on another format, a missing pointer, a bad stride,
    overlapping ranges and the wrong family for the chain; then -19: validation comes first"""
    lib = T.load_library()
    nb, n = 2, 2
    frames = nb * 128
    x = np.zeros((n, frames), np.float32)
    for chain in (FULL, TONEGEN, FX):
        fx = chain == FX
        eng = _engine(chain, n)

        def call(po, fx=fx, eng=eng):
            if fx:
                return lib.tbf_process_pcm(eng._h, nb, x.ctypes.data, frames, C.byref(po))
            return lib.tbf_render_pcm(eng._h, nb, C.byref(po))

        def call_dev(po, fx=fx, eng=eng):
            if fx:
                return lib.tbf_process_pcm_device(eng._h, nb, None, 0, x.ctypes.data, frames, C.byref(po), None)
            return lib.tbf_render_pcm_device(eng._h, nb, None, 0, C.byref(po), None)
        for fmt, flags in M.FORMATS:
            for meters in (True, False):
                po, keep = _pcm_out(n, frames, fmt, flags, meters)
                assert call(po) == -19 and "host-only" in _err(eng)
                assert call_dev(po) == -19
        po, keep = _pcm_out(n, frames)
        if fx:
            assert lib.tbf_render_pcm(eng._h, nb, C.byref(po)) == -22 and "tbf_process_pcm" in _err(eng)
            assert lib.tbf_render_pcm_device(eng._h, nb, None, 0, C.byref(po), None) == -22
            assert lib.tbf_process_pcm(eng._h, nb, None, frames, C.byref(po)) == -22 and "null" in _err(eng)
            assert lib.tbf_process_pcm(eng._h, nb, x.ctypes.data, frames - 1, C.byref(po)) == -22 and "in_stride" in _err(eng)
            po.out = x.ctypes.data + 8  # the frames inside the input rows
            assert call(po) == -22 and "overlap" in _err(eng)
        else:
            assert lib.tbf_process_pcm(eng._h, nb, x.ctypes.data, frames, C.byref(po)) == -22 and "effects-only" in _err(eng)
            assert lib.tbf_process_pcm_device(eng._h, nb, None, 0, x.ctypes.data, frames, C.byref(po), None) == -22
        rowb = frames * 4
        for mutate, word in [(lambda p: setattr(p, "format", 3), "format"),
                             (lambda p: setattr(p, "flags", 2), "flags"),
                             (lambda p: setattr(p, "flags", 3), "flags"),
                             (lambda p: (setattr(p, "format", M.S24), setattr(p, "flags", M.DITHER)), "dither"),
                             (lambda p: (setattr(p, "format", M.F32), setattr(p, "flags", M.DITHER)), "dither"),
                             (lambda p: setattr(p, "out", None), "null"),
                             (lambda p: setattr(p, "out_stride_bytes", rowb + 2), "multiple of 4"),
                             (lambda p: setattr(p, "out_stride_bytes", rowb - 4), "smaller"),
                             (lambda p: (setattr(p, "format", M.S24), setattr(p, "out_stride_bytes", frames * 6 - 4)), "smaller"),
                             (lambda p: setattr(p, "meters", p.out + 16), "overlap"),
                             (lambda p: setattr(p, "out", p.meters + 12), "overlap")]:
            po, keep = _pcm_out(n, frames)
            mutate(po)
            assert call(po) == -22 and word in _err(eng), (word, _err(eng))
            if word != "overlap":
                assert call_dev(po) == -22 and word in _err(eng), (word, _err(eng))
        po, keep = _pcm_out(n, frames)
        po.out += 2
        assert call_dev(po) == -22 and "aligned" in _err(eng)  # device pointers are 4-byte aligned
        assert call(po) == -19                                  # a host buffer need not be
        assert lib.tbf_render_pcm(None, nb, C.byref(po)) == -22 and lib.tbf_render_pcm(eng._h, nb, None) == -22
        ev = eng.events([(1, 0, 0, 60, 1.0), (0, 0, 0, 62, 1.0)])[::-1].copy()  # out of order
        po, keep = _pcm_out(n, frames)
        if not fx:
            assert lib.tbf_render_pcm_device(eng._h, nb, ev.ctypes.data, len(ev), C.byref(po), None) == -22
            assert lib.tbf_render_pcm_device(eng._h, nb, None, 2, C.byref(po), None) == -22
        eng.close()


def test_pcm_convert_refused_on_host_engines():
    lib = T.load_library()
    eng = _engine(n=0)
    rows, frames = 3, 100
    L = np.zeros((rows, frames + 1), np.float32)
    R = np.zeros_like(L)
    counts = np.array([0, 1, 100], np.uint32)

    def call(po, l=L.ctypes.data, r=R.ctypes.data, stride=frames + 1, cnt=counts.ctypes.data, fr=frames):
        return lib.tbf_pcm_convert_device(eng._h, rows, l, r, stride, fr, cnt, C.byref(po), None)
    for fmt, flags in M.FORMATS:
        po, keep = _pcm_out(rows, frames, fmt, flags)
        assert call(po) == -19 and call(po, cnt=None) == -19
        assert call(po, r=L.ctypes.data) == -19  # a mono source: the same plane twice
    po, keep = _pcm_out(rows, frames)
    assert call(po, l=None) == -22 and call(po, r=None) == -22
    assert call(po, l=L.ctypes.data + 2) == -22 and "aligned" in _err(eng)
    assert call(po, stride=frames - 1) == -22 and "in_stride" in _err(eng)
    assert call(po, fr=99) == -22 and "counts[2]" in _err(eng)
    po.out = L.ctypes.data + 4 * (frames + 1)
    assert call(po) == -22 and "overlap" in _err(eng)
    po, keep = _pcm_out(rows, frames)
    po.meters = R.ctypes.data
    assert call(po) == -22 and "overlap" in _err(eng)
    for mutate, word in [(lambda p: setattr(p, "format", 7), "format"), (lambda p: setattr(p, "flags", 4), "flags"),
                         (lambda p: (setattr(p, "format", M.S24), setattr(p, "flags", 1)), "dither"),
                         (lambda p: setattr(p, "out_stride_bytes", 4 * frames - 4), "smaller"),
                         (lambda p: setattr(p, "out_stride_bytes", 4 * frames + 1), "multiple of 4"),
                         (lambda p: setattr(p, "meters", p.meters + 2), "aligned")]:
        po, keep = _pcm_out(rows, frames)
        mutate(po)
        assert call(po) == -22 and word in _err(eng), (word, _err(eng))
    eng.close()
