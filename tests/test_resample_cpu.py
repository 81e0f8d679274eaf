"""The output rate converter without a GPU, on host-only engines: the prototype table against the
numpy double design, its frequency response, the count law, the host restatement
(tbf_debug_resample_ref) against a float64 evaluation of the same sum and against itself fed in
pieces, and the refusals of tbf_resampler_set, the resampled calls and a blob from another
converter."""
import ctypes as C

import numpy as np
import pytest

import resample_model as M

T = pytest.importorskip("tunebfree_amd")

FULL, TONEGEN, FX = 0, 1, 4
RESPONSE_PAIRS = [(48000, 16000), (48000, 22050), (48000, 8000), (48000, 32000), (48000, 44100), (44100, 48000),
                  (44100, 16000), (192000, 8000)]
GPU_PAIRS = [(fi, fo) for (fi, fo, *_r) in M.PAIRS]


def _engine(fi=48000, fo=None, chain=FULL, n=0):
    eng = T.Engine(sample_rate=float(fi), device=-1, chain=chain)
    if fo is not None:
        eng.set_output_rate(fo)
    if n:
        tid = eng.template(seed=7)
        eng.add_instances([tid] * n, [100 + i for i in range(n)])
    return eng


def _err(eng):
    return eng._lib.tbf_last_error().decode()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def blob(eng, i):
    return eng.save([i]).tobytes()


@pytest.fixture(scope="module")
def tables():
    """(info of the engine's hook, the numpy double design) per pair, computed once"""
    out = {}
    for fi, fo in sorted(set(RESPONSE_PAIRS + GPU_PAIRS)):
        eng = _engine(fi, fo)
        out[fi, fo] = (eng.resampler_info(), M.design(fi, fo))
        eng.close()
    return out


# ---------------------------------------------------------------- 1. the table
def test_pairs_have_the_stated_ratios(tables):
    """the engine's hook reports the issue's L, M, T for the four pairs of the GPU tests"""
    for fi, fo, L, Mm, Tt in M.PAIRS:
        info = tables[fi, fo][0]
        assert (info["L"], info["M"], info["T"]) == (L, Mm, Tt) == M.ratio(fi, fo)


@pytest.mark.parametrize("fi,fo", RESPONSE_PAIRS)
def test_table_matches_the_double_design(tables, fi, fo):
    """each tap within 2^-24 |g64| + 2^-40 max |g64|: float rounding plus the absolute error of
    two double evaluations"""
    info, g64 = tables[fi, fo]
    L, Mm, Tt = M.ratio(fi, fo)
    assert (info["L"], info["M"], info["T"]) == (L, Mm, Tt)
    assert info["table"].dtype == np.float32 and len(info["table"]) == L * Tt
    assert info["latency"] == (L * Tt - 1) / (2.0 * L)
    err = np.abs(info["table"].astype(np.float64) - g64)
    bound = 2.0 ** -24 * np.abs(g64) + 2.0 ** -40 * np.abs(g64).max()
    worst = float((err / bound).max())
    print(f"{fi} -> {fo}: worst tap error {worst:.3f} of its bound")
    assert worst <= 1.0


def test_no_converter_reports_zeros():
    eng = _engine()
    info = eng.resampler_info()
    assert (info["L"], info["M"], info["T"], info["latency"], len(info["table"])) == (0, 0, 0, 0.0, 0)
    eng.close()


# ---------------------------------------------------------------- 2. frequency response
@pytest.mark.parametrize("fi,fo", RESPONSE_PAIRS)
def test_frequency_response(tables, fi, fo):
    """from the hook's float32 table, evaluated in float64: passband [0, 0.8 ny] within
    +-2e-4 dB, everything from ny = min (Fi, Fo) / 2 up at or below -98 dB"""
    info, _g64 = tables[fi, fo]
    L, Mm = info["L"], info["M"]
    f, db = M.response_db(info["table"], L)
    ny = 0.5 / max(L, Mm)  # in cycles per sample of the L-times upsampled rate
    pb, sb = db[f <= 0.8 * ny], db[f >= ny]
    print(f"{fi} -> {fo}: passband {pb.min():+.2e} .. {pb.max():+.2e} dB, stopband peak {sb.max():.2f} dB")
    assert len(pb) > 8 and len(sb) > 8
    assert np.abs(pb).max() <= 2e-4
    assert sb.max() <= -98.0


# ---------------------------------------------------------------- 3. the count law
@pytest.mark.parametrize("fi,fo", GPU_PAIRS)
def test_count_law(fi, fo):
    """over random cut sequences the per-call counts are C (P + N) - C (P), sum to C (total) and
    never exceed tbf_resampled_frames; the ref hook reports the same counts"""
    eng = _engine(fi, fo)
    L, Mm, _T = M.ratio(fi, fo)
    rng = np.random.default_rng(fi + fo)
    for _ in range(4):
        P, total = 0, 0
        for nb in rng.integers(1, 40, size=25):
            nb = int(nb)
            want = M.count(P + nb * 128, L, Mm) - M.count(P, L, Mm)
            frames = eng.resampled_frames(nb)
            assert frames == M.count(nb * 128, L, Mm)
            assert want <= frames
            assert len(eng.resample_ref(np.zeros(nb * 128, np.float32), pos0=P)) == want
            P += nb * 128
            total += want
        assert total == M.count(P, L, Mm)
    eng.close()


# ---------------------------------------------------------------- 4. the host restatement
def _near(fi, fo, cross):
    """a position P (a multiple of 128) whose next two blocks' outputs have n M pass `cross`"""
    L, Mm, _T = M.ratio(fi, fo)
    P = (cross // L) // 128 * 128 - 128
    n0, n1 = M.count(P, L, Mm), M.count(P + 256, L, Mm)
    assert n0 * Mm < cross <= (n1 - 1) * Mm
    return P


@pytest.mark.parametrize("fi,fo", GPU_PAIRS)
@pytest.mark.parametrize("where", ["start", "2^32"])
def test_ref_hook_against_float64(fi, fo, where):
    """per sample |y - y64| <= 1.01 T 2^-24 sum_t |g_t x_t|, the bound of a sequential fma sum,
    against the same float32 taps in float64"""
    eng = _engine(fi, fo)
    info = eng.resampler_info()
    L, Mm, Tt = info["L"], info["M"], info["T"]
    rng = np.random.default_rng(3)
    pos0 = 0 if where == "start" else _near(fi, fo, 1 << 32)
    x = (rng.standard_normal(6 * 128) * 0.25).astype(np.float32)
    hist = None if where == "start" else (rng.standard_normal(Tt - 1) * 0.25).astype(np.float32)
    y = eng.resample_ref(x, hist, pos0)
    y64, mag = M.ref64(info["table"], L, Mm, Tt, x, hist, pos0)
    eng.close()
    assert len(y) == len(y64) > 0 and float(np.abs(y).max()) > 1e-3
    worst = float((np.abs(y.astype(np.float64) - y64) / (1.01 * Tt * M.EPS * mag + 1e-300)).max())
    print(f"{fi} -> {fo} at {where}: worst error {worst:.4f} of the fma bound")
    assert np.all(np.abs(y.astype(np.float64) - y64) <= 1.01 * Tt * M.EPS * mag)


@pytest.mark.parametrize("fi,fo", GPU_PAIRS)
@pytest.mark.parametrize("where", ["start", "2^32"])
def test_ref_hook_in_pieces_equals_one_shot(fi, fo, where):
    """hist and pos0 carried from piece to piece: the same bits, n M crossing 2^32 included"""
    eng = _engine(fi, fo)
    Tt = eng.resampler_info(table=False)["T"]
    rng = np.random.default_rng(5)
    pos0 = 0 if where == "start" else _near(fi, fo, 1 << 32) - 640  # the crossing in blocks 5 and 6
    x = (rng.standard_normal(12 * 128) * 0.25).astype(np.float32)
    whole = eng.resample_ref(x, None, pos0)
    for cuts in ([128] * 12, [128, 640, 768], [1, 127, 300, 1108]):
        assert sum(cuts) == len(x)
        hist, at, parts = np.zeros(Tt - 1, np.float32), 0, []
        for c in cuts:
            parts.append(eng.resample_ref(x[at:at + c], hist, pos0 + at))
            hist = np.concatenate([hist, x[at:at + c]])[-(Tt - 1):]
            at += c
        got = np.concatenate(parts)
        assert got.shape == whole.shape and np.array_equal(bits(got), bits(whole)), cuts
    eng.close()


# ---------------------------------------------------------------- 5. refusals
def test_resampler_set_codes():
    lib = T.load_library()
    eng = _engine()
    assert lib.tbf_resampler_set(eng._h, 48000) == -22 and "equals" in _err(eng)
    assert lib.tbf_resampler_set(eng._h, 44101) == -22 and "cap" in _err(eng)  # L = 44101 > 1024
    assert lib.tbf_resampler_set(eng._h, 7) == -22 and "cap" in _err(eng)      # L T > 2^18
    assert lib.tbf_resampler_set(eng._h, 16000) == 0
    assert eng.resampler_info(table=False)["T"] == 192
    assert lib.tbf_resampler_set(eng._h, 0) == 0  # none again
    assert eng.resampler_info(table=False)["L"] == 0
    assert lib.tbf_resampler_set(eng._h, 22050) == 0
    tid = eng.template(seed=7)
    eng.add_instances([tid], [1])
    assert lib.tbf_resampler_set(eng._h, 16000) == -16
    assert lib.tbf_resampler_set(eng._h, 0) == -16
    eng.remove([0])
    assert lib.tbf_resampler_set(eng._h, 16000) == -16  # an instance was added once
    assert eng.resampler_info(table=False)["L"] == 147
    eng.close()
    frac = T.Engine(sample_rate=48000.5, device=-1)
    assert lib.tbf_resampler_set(frac._h, 16000) == -22 and "integer" in _err(frac)
    frac.close()


def _out(n, frames, per, raw=True):
    a = [np.zeros((n, frames), np.float32) for _ in range(2)] + [np.zeros((n, per), np.float32) for _ in range(2)]
    counts = np.full(n, 77, np.uint32)
    ro = T.engine.ResampledOut(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data if raw else None,
                               a[3].ctypes.data if raw else None, frames, per, counts.ctypes.data)
    return ro, a, counts


def test_resampled_calls_refused_on_host_engines():
    """-19 on a host-only engine with a converter; -22 without one, for the wrong family, a
    missing pointer, half a raw pair, a short stride and overlapping ranges"""
    lib = T.load_library()
    nb, n = 2, 2
    x = np.zeros((n, nb * 128), np.float32)
    for chain in (FULL, TONEGEN, FX):
        fx = chain == FX
        eng = _engine(48000, 16000, chain, n)
        frames = eng.resampled_frames(nb)
        assert frames == 86

        def call(ro, e=eng, fx=fx):
            if fx:
                return lib.tbf_process_resampled(e._h, nb, x.ctypes.data, nb * 128, C.byref(ro))
            return lib.tbf_render_resampled(e._h, nb, C.byref(ro))

        ro, keep, counts = _out(n, frames, nb * 128)
        assert call(ro) == -19
        ro, keep, counts = _out(n, frames, nb * 128, raw=False)
        assert call(ro) == -19
        assert lib.tbf_render_resampled_device(eng._h, nb, None, 0, C.byref(ro), None) == (-22 if fx else -19)
        assert lib.tbf_process_resampled_device(eng._h, nb, None, 0, x.ctypes.data, nb * 128, C.byref(ro), None) == (
            -19 if fx else -22)
        # the wrong family for the chain
        if fx:
            assert lib.tbf_render_resampled(eng._h, nb, C.byref(ro)) == -22 and "tbf_process_resampled" in _err(eng)
        else:
            assert lib.tbf_process_resampled(eng._h, nb, x.ctypes.data, nb * 128, C.byref(ro)) == -22
            assert "effects-only" in _err(eng)
        for mutate, word in [(lambda r: setattr(r, "L", None), "null"), (lambda r: setattr(r, "R", None), "null"),
                             (lambda r: setattr(r, "counts", None), "null"),
                             (lambda r: setattr(r, "rawR", None), "both or neither"),
                             (lambda r: setattr(r, "rawL", None), "both or neither"),
                             (lambda r: setattr(r, "stride", frames - 1), "stride"),
                             (lambda r: setattr(r, "raw_stride", nb * 128 - 1), "raw_stride"),
                             (lambda r: setattr(r, "R", r.L + 4 * (frames - 1)), "overlap"),
                             (lambda r: setattr(r, "rawL", r.rawR + 4), "overlap")]:
            ro, keep, counts = _out(n, frames, nb * 128)
            mutate(ro)
            assert call(ro) == -22 and word in _err(eng), (word, _err(eng))
        eng.close()
        none = _engine(48000, None, chain, n)
        ro, keep, counts = _out(n, frames, nb * 128)
        assert call(ro, none) == -22 and "no resampler" in _err(none)
        m = C.c_uint64()
        assert lib.tbf_resampled_frames(none._h, nb, C.byref(m)) == -22
        none.close()


def test_blob_from_another_converter_is_refused():
    """a blob saved under one output rate loaded into an engine with another, or none: -22
    naming the resampler, and nothing changed; into an equal converter it loads"""
    lib = T.load_library()
    eng = _engine(48000, 16000, n=2)
    eng.resampler_pos(1, 640)
    saved = eng.save([1])
    eng.close()
    buf = np.frombuffer(saved.tobytes(), np.uint8)
    idx = (C.c_uint32 * 1)(0)
    twin = _engine(48000, 16000, n=1)
    twin.note(0, 60, 1)
    twin.load([0], saved)
    assert blob(twin, 0) == saved.tobytes()
    twin.close()
    for other in (22050, 8000, None):
        o = _engine(48000, other, n=1)
        o.note(0, 60, 1)
        before = blob(o, 0)
        rc = lib.tbf_instances_load(o._h, 1, idx, buf.ctypes.data_as(C.c_void_p), buf.nbytes)
        assert rc == -22 and "resampler" in _err(o), _err(o)
        assert blob(o, 0) == before
        o.close()


def test_position_travels_with_clone_save_load_and_remove():
    """P is host state of the instance: on a host-only engine it is visible through the blob, which
    differs exactly when P differs"""
    eng = _engine(48000, 22050, n=3)
    eng.resampler_pos(1, 12345)
    c = eng.clone([1])
    assert c == 3 and blob(eng, c) == blob(eng, 1) != blob(eng, 0)
    saved = eng.save([1])
    eng.resampler_pos(1, 5)
    assert blob(eng, 1) != saved.tobytes()
    eng.load([1], saved)
    assert blob(eng, 1) == saved.tobytes()
    eng.remove([0])
    assert blob(eng, 0) == saved.tobytes()
    eng.close()
