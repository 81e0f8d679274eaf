"""The loudness meter without a GPU: the coefficients against the standard's table and the model's
formulas, the host restatement of the recurrence (tbf_debug_loudness_ref, built from the header
k_loud is built from) against the plain-Python model in bits, the order of the operations made
observable, cuts into calls, EBU Tech 3341 style compliance figures, the gating alone
(tbf_debug_loudness_result) against a numpy restatement, the literal NaN / Inf cases, and the
refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import loudness_model as M

T = pytest.importorskip("tunebfree_amd")
E = T.engine

bits = M.bits


def _err():
    return T.load_library().tbf_last_error().decode()


def _special(n, seed):
    """noise with a negative zero and a subnormal in it"""
    x = M.noise(seed, n)
    x[7], x[11] = -0.0, np.float32(1e-41)
    return x


INPUTS = {
    (8000, "noise"): lambda: (M.noise(1, 6000), M.noise(2, 6000)),
    (44100, "noise"): lambda: (M.noise(3, 6000), M.noise(4, 6000)),
    (8000, "special"): lambda: (_special(6000, 5), _special(6000, 6)),
    (44100, "special"): lambda: (_special(6000, 7), _special(6000, 8)),
}
_cache = {}


def _both(rate, kind):
    """(inputs, loudness_ref's results, the model's), computed once"""
    if (rate, kind) not in _cache:
        L, R = INPUTS[rate, kind]()
        _cache[rate, kind] = (L, R, T.Engine.loudness_ref(L, R, rate), M.row(L, R, rate))
    return _cache[rate, kind]


# ---------------------------------------------------------------- 1. coefficients and mirrors
def test_coefficients_at_48k_are_the_standards_table():
    c = T.Engine.loudness_coeffs(48000)
    err = np.abs(c - np.array(M.TABLE_48K))
    print("48 kHz coefficients against the table:", err.max())
    assert err.max() <= 5e-15


@pytest.mark.parametrize("rate", [8000, 22050, 44100, 96000, 192000])
def test_coefficients_follow_the_formula(rate):
    c, m = T.Engine.loudness_coeffs(rate), M.coeffs(rate)
    d = M.ulps(c, m)
    print(f"{rate}: ulps {d.tolist()}")
    assert (np.sign(c) == np.sign(m)).all() and d.max() <= 4


def test_structs_mirror_the_header():
    assert C.sizeof(E.LoudnessConfig) == 8 and C.sizeof(E.LoudnessResult) == 40
    assert T.params.LOUDNESS_RESULT_DTYPE.itemsize == 40 and T.params.LOUDNESS_RESULT_DTYPE == M.RESULT_DTYPE
    assert [f[0] for f in E.LoudnessResult._fields_] == list(M.RESULT_DTYPE.names)
    rpg, tile, lds = T.Engine.loudness_grid(1)
    assert rpg >= 1 and tile >= 1 and lds <= 160 * 1024


# ---------------------------------------------------------------- 2. the restatement in bits
@pytest.mark.parametrize("rate,kind", list(INPUTS))
def test_ref_equals_the_model_in_bits(rate, kind):
    L, R, (e, st), (me, mst) = _both(rate, kind)
    assert e.shape == me.shape == (6000 // (rate // 10), 2)
    assert np.array_equal(bits(e), bits(me))
    assert np.array_equal(bits(st), bits(mst))
    assert st[5] == st[11] == 6000 % (rate // 10)


# ---------------------------------------------------------------- 3. the order is observable
@pytest.mark.parametrize("variant", ["s1", "half"])
def test_order_is_observable(variant):
    """another association of s1's terms, or a hop's sum taken in two halves, moves most hop
    energies, so a kernel that re-associated or contracted could not equal the restatement by
    accident"""
    L, R, (e, _), _ = _both(8000, "noise")
    ve, _ = M.row(L, R, 8000, variant=variant)
    differ = int((bits(ve) != bits(e)).sum())
    print(f"{variant}: {differ} of {e.size} hop energies differ")
    assert ve.shape == e.shape and differ > e.size // 2
    assert np.allclose(ve, e, rtol=1e-9)   # the same quantity, another rounding


# ---------------------------------------------------------------- 4. cuts
@pytest.mark.parametrize("rate", [8000, 44100])
def test_cuts_equal_one_call(rate):
    L, R, (e, st), _ = _both(rate, "noise")
    Hp = rate // 10
    total = 6000 if rate == 8000 else 3 * Hp     # three hops at least, so that the last cut lies in the third
    if rate != 8000:
        L, R = M.noise(21, total), M.noise(22, total)
        e, st = T.Engine.loudness_ref(L, R, rate)
    at = [0, 1, Hp - 1, Hp, Hp + 1, 2 * Hp + 37, total]
    state, got = None, []
    for a, b in zip(at[:-1], at[1:]):
        ge, state = T.Engine.loudness_ref(L[a:b], R[a:b], rate, state=state)
        got.append(ge)
    got = np.concatenate(got)
    assert np.array_equal(bits(got), bits(e)) and np.array_equal(bits(state), bits(st))
    # an empty call leaves the state as it is
    ge, s2 = T.Engine.loudness_ref(L[:0], R[:0], rate, state=state)
    assert len(ge) == 0 and np.array_equal(bits(s2), bits(state))


# ---------------------------------------------------------------- 5. compliance
COMPLIANCE = {
    "48k -23 dBFS 20 s": (48000, [(-23.0, 20.0)], -23.0),
    "48k -33 dBFS 20 s": (48000, [(-33.0, 20.0)], -33.0),
    "48k -36/-23/-36 dBFS 10/60/10 s": (48000, [(-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0)], -23.0),
    "48k -72/-36/-23/-36/-72 dBFS": (48000, [(-72.0, 10.0), (-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0), (-72.0, 10.0)], -23.0),
    "48k -26/-20/-26 dBFS 20/20.1/20 s": (48000, [(-26.0, 20.0), (-20.0, 20.1), (-26.0, 20.0)], -23.0),
    "44.1k -23 dBFS 20 s": (44100, [(-23.0, 20.0)], -23.0),
    "16k -23 dBFS 5 s": (16000, [(-23.0, 5.0)], -23.0),
}
_energies = {}


def _compliance_energies(name):
    if name not in _energies:
        rate, segments, _ = COMPLIANCE[name]
        x = M.sine(rate, segments)
        _energies[name] = T.Engine.loudness_ref(x, x, rate)[0]
    return _energies[name]


@pytest.mark.parametrize("name", list(COMPLIANCE))
def test_compliance_with_a_1khz_sine(name):
    """a 1 kHz sine, equal in both channels, at a level in dBFS peak reads that level in LUFS within
    EBU Tech 3341's 0.1 LU, through the relative and the absolute gate"""
    rate, segments, want = COMPLIANCE[name]
    e = _compliance_energies(name)
    res = T.Engine.loudness_result(rate, e)
    print(f"{name}: integrated {res['integrated']:.4f}, {res['gated']} of {res['blocks']} blocks gated, "
          f"momentary max {res['momentary_max']:.4f}, short-term max {res['short_term_max']:.4f}")
    assert res["hops"] == len(e) == int(round(sum(s for _d, s in segments) * 10))
    assert res["blocks"] == len(e) - 3
    assert abs(res["integrated"] - want) <= 0.1
    if any(db <= -36.0 for db, _s in segments):   # more than 10 LU below the rest: the gates remove blocks
        assert 0 < res["gated"] < res["blocks"]
    else:
        assert res["gated"] == res["blocks"]


# ---------------------------------------------------------------- 6. the gating alone
@pytest.mark.parametrize("name", list(COMPLIANCE))
def test_result_equals_the_numpy_gating(name):
    rate = COMPLIANCE[name][0]
    e = _compliance_energies(name)
    got, want = T.Engine.loudness_result(rate, e), M.gating(rate, e)
    for f in ("integrated", "momentary_max", "short_term_max"):
        assert abs(got[f] - want[f]) <= 1e-9, (f, got[f], want[f])
    for f in ("hops", "blocks", "gated"):
        assert got[f] == want[f], (f, got[f], want[f])
    assert got["reserved"] == 0


def test_result_edges():
    e = _compliance_energies("48k -23 dBFS 20 s")
    for n in range(4):   # fewer than 4 hops: no block
        r = T.Engine.loudness_result(48000, e[:n])
        assert r["hops"] == n and r["blocks"] == 0 and r["gated"] == 0
        assert r["integrated"] == r["momentary_max"] == r["short_term_max"] == -np.inf
    r = T.Engine.loudness_result(48000, np.zeros((50, 2)))   # silence
    assert r["blocks"] == 47 and r["gated"] == 0 and r["integrated"] == -np.inf
    r29, r30 = T.Engine.loudness_result(48000, e[:29]), T.Engine.loudness_result(48000, e[:30])
    assert r29["short_term_max"] == -np.inf and np.isfinite(r29["momentary_max"]) and np.isfinite(r29["integrated"])
    assert np.isfinite(r30["short_term_max"]) and abs(r30["short_term_max"] - r30["integrated"]) < 0.01


def test_a_pair_of_equal_channels_reads_3_db_above_one_channel():
    e = _compliance_energies("48k -23 dBFS 20 s")
    left = e.copy()
    left[:, 1] = 0.0     # the same L beside a silent R
    pair, one = T.Engine.loudness_result(48000, e), T.Engine.loudness_result(48000, left)
    d = pair["integrated"] - one["integrated"]
    print("pair above one channel:", d)
    assert abs(d - 10.0 * math.log10(2.0)) <= 1e-9 and abs(d - 3.01) < 0.001
    # and the recurrence of a silent channel gives exactly zero energies
    x = M.sine(48000, [(-23.0, 1.0)])
    e2, _ = T.Engine.loudness_ref(x, np.zeros_like(x), 48000)
    assert not bits(e2[:, 1]).any() and np.array_equal(bits(e2[:, 0]), bits(e[:10, 0]))


# ---------------------------------------------------------------- 7. the literal cases
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nan_and_inf_poison_their_channel_only(bad):
    L, R, (e, _), _ = _both(8000, "noise")
    Lb = L.copy()
    Lb[100] = bad
    eb, st = T.Engine.loudness_ref(Lb, R, 8000)
    assert np.isnan(eb[:, 0]).all() and np.isnan(st[:5]).all()
    assert np.array_equal(bits(eb[:, 1]), bits(e[:, 1])) and np.isfinite(st[6:]).all()
    # in the second hop: the first one is clean
    Lb = L.copy()
    Lb[900] = bad
    eb, _ = T.Engine.loudness_ref(Lb, R, 8000)
    assert bits(eb[0, 0]) == bits(e[0, 0]) and np.isnan(eb[1:, 0]).all()
    res = T.Engine.loudness_result(8000, eb)
    assert res["gated"] == 0 and res["integrated"] == -np.inf   # a NaN block passes no gate


# ---------------------------------------------------------------- 8. refusals
def _create(eng, n_rows, rate, max_hops, cfg_null=False, out_null=False):
    cfg, h = E.LoudnessConfig(rate, max_hops), C.c_void_p()
    return eng._lib.tbf_loudness_create(eng._h, n_rows, None if cfg_null else C.byref(cfg), None if out_null else C.byref(h))


def test_host_only_engine_validates_then_refuses():
    eng = T.Engine(sample_rate=48000.0, device=-1)
    assert _create(eng, 4, 48000, 100) == -19 and "host-only" in _err()
    with pytest.raises(T.TbfError, match="-19"):
        eng.loudness(4)
    bad = [
        (dict(n_rows=4, rate=7990, max_hops=10), "rate_hz"),
        (dict(n_rows=4, rate=192010, max_hops=10), "rate_hz"),
        (dict(n_rows=4, rate=44101, max_hops=10), "rate_hz"),
        (dict(n_rows=4, rate=0, max_hops=10), "rate_hz"),
        (dict(n_rows=4, rate=48000, max_hops=0), "max_hops"),
        (dict(n_rows=0, rate=48000, max_hops=10), "n_rows"),
        (dict(n_rows=4, rate=48000, max_hops=10, cfg_null=True), "cfg"),
        (dict(n_rows=4, rate=48000, max_hops=10, out_null=True), "out"),
    ]
    for kw, word in bad:   # validation comes before the -19
        assert _create(eng, **kw) == -22, kw
        assert word in _err(), (kw, _err())
    cfg, h = E.LoudnessConfig(48000, 10), C.c_void_p()
    assert eng._lib.tbf_loudness_create(None, 4, C.byref(cfg), C.byref(h)) == -22 and "engine" in _err()
    eng.close()


def test_null_meter_and_hook_refusals():
    lib = T.load_library()
    n = C.c_uint32()
    res = np.zeros(1, M.RESULT_DTYPE)
    assert lib.tbf_loudness_reset(None, 0, None, None) == -22 and "lm" in _err()
    assert lib.tbf_loudness_device(None, None, None, 0, 0, None, None) == -22 and "lm" in _err()
    assert lib.tbf_loudness_read(None, 0, None, res.ctypes.data) == -22 and "lm" in _err()
    assert lib.tbf_loudness_hops(None, 0, None, 0, C.byref(n)) == -22 and "lm" in _err()
    assert lib.tbf_loudness_destroy(None) == 0
    for rate in (7999, 48001, 200000):
        with pytest.raises(T.TbfError, match="-22.*rate_hz"):
            T.Engine.loudness_coeffs(rate)
        with pytest.raises(T.TbfError, match="-22.*rate_hz"):
            T.Engine.loudness_result(rate, np.zeros((4, 2)))
        with pytest.raises(T.TbfError, match="-22.*rate_hz"):
            T.Engine.loudness_ref(np.zeros(8, np.float32), np.zeros(8, np.float32), rate)
    x = np.zeros(8, np.float32)
    for k in (-1.0, 800.0, 1.5, np.nan):
        st = np.zeros(12)
        st[11] = k
        with pytest.raises(T.TbfError, match="-22.*state"):
            T.Engine.loudness_ref(x, x, 8000, state=st)
    f = lib.tbf_debug_loudness_ref
    f.restype = C.c_int
    f.argtypes = [C.POINTER(E.LoudnessConfig), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                  C.POINTER(C.c_uint32)]
    cfg, st, e = E.LoudnessConfig(8000, 1), np.zeros(12), np.zeros(2)
    assert f(C.byref(cfg), x.ctypes.data, x.ctypes.data, 8, None, e.ctypes.data, 1, C.byref(n)) == -22 and "state" in _err()
    assert f(C.byref(cfg), None, x.ctypes.data, 8, st.ctypes.data, e.ctypes.data, 1, C.byref(n)) == -22 and "L is NULL" in _err()
    assert f(C.byref(cfg), x.ctypes.data, x.ctypes.data, 8, st.ctypes.data, e.ctypes.data, 1, None) == -22 and "n_hops" in _err()
    g = lib.tbf_debug_loudness_result
    g.restype, g.argtypes = C.c_int, [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    assert g(48000, np.zeros(8).ctypes.data, 4, None) == -22 and "out" in _err()
    assert g(48000, None, 4, res.ctypes.data) == -22 and "e is NULL" in _err()


def test_ref_with_too_small_a_cap_writes_nothing():
    L, R, (e, st), _ = _both(8000, "noise")
    assert len(e) == 7
    with pytest.raises(T.TbfError, match="-28.*cap_hops"):
        T.Engine.loudness_ref(L, R, 8000, cap_hops=6)
    lib = T.load_library()
    f = lib.tbf_debug_loudness_ref
    f.restype = C.c_int
    f.argtypes = [C.POINTER(E.LoudnessConfig), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                  C.POINTER(C.c_uint32)]
    cfg, state, out, n = E.LoudnessConfig(8000, 1), np.full(12, 0.0), np.full((8, 2), -5.0), C.c_uint32(99)
    state[5] = state[11] = 400.0    # half a hop in: 6400 frames complete 8 hops
    assert f(C.byref(cfg), L.ctypes.data, R.ctypes.data, 6000, state.ctypes.data, out.ctypes.data, 7, C.byref(n)) == -28
    assert (out == -5.0).all() and n.value == 99 and state[5] == 400.0 and not state[:5].any()
    assert f(C.byref(cfg), L.ctypes.data, R.ctypes.data, 6000, state.ctypes.data, out.ctypes.data, 8, C.byref(n)) == 0
    assert n.value == 8 and state[5] == 0.0
