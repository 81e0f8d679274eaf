"""The bus equaliser without a GPU: the host restatement of the definition (tbf_debug_eq_ref) against
the plain-Python model in bits, cuts, the pass-through of a row without bands, the designer
(tbf_debug_eq_coeffs) against the model's formulas and against the gains it is designed for, the
whirl's filters through the same designer, the refusals, and the values that must not move.

The stage is this project's own definition (include/tbf.h); the kernel is held
to the restatement in bits by tests/test_gpu_eq.py."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

import eq_model as M

T = pytest.importorskip("tunebfree_amd")
E = T.engine
P = T.params
bits = M.bits
RATES = (8000, 44100, 48000, 192000)
ROOT = Path(__file__).resolve().parents[1]


def _bands(k, seed, rate=8000):
    """k stable bands of rotating types, as (records, library coefficients [k, 5])"""
    rng = np.random.default_rng(seed)
    recs = [P.eq_band(int((seed + j) % 9), float(rng.uniform(0.004, 0.45) * rate), float(rng.uniform(0.4, 3.0)),
                      float(rng.uniform(-9.0, 9.0))) for j in range(k)]
    return recs, np.array([T.Engine.eq_coeffs(b, rate) for b in recs], np.float64).reshape(-1, 5)


def _err():
    return T.load_library().tbf_last_error().decode()


def _special(n, seed):
    """noise with -0, subnormal floats and a stretch of tiny values among it"""
    x = M.noise(seed, n)
    if n > 60:
        x[5], x[6], x[7] = -0.0, np.float32(1e-42), np.float32(-3e-45)
        x[40:60] *= np.float32(1e-38)
    return x


# ---------------------------------------------------------------- the restatement against the model
@pytest.mark.parametrize("nb", [0, 1, 3, 8])
def test_ref_equals_the_model_in_bits(nb):
    """states carried over three calls, with -0 and subnormal floats among the frames"""
    _, c = _bands(nb, 10 + nb)
    st = mst = None
    for k, n in enumerate((211, 1, 300)):
        L, R = _special(n, 20 + k), _special(n, 30 + k)
        oL, oR, st = T.Engine.eq_ref(L, R, c, st)
        mL, mR, mst = M.row(L, R, c, mst)
        assert np.array_equal(bits(oL), bits(mL)) and np.array_equal(bits(oR), bits(mR)), (nb, k)
        assert st.tobytes() == mst.tobytes(), (nb, k)
    assert st.shape == (2, nb, 2)


def test_ref_with_equal_channels():
    _, c = _bands(3, 3)
    L = M.noise(4, 257)
    oL, oR, st = T.Engine.eq_ref(L, L, c)
    mL, _ = M.cascade(L, c)
    assert np.array_equal(bits(oL), bits(mL)) and np.array_equal(bits(oR), bits(mL))
    assert st[0].tobytes() == st[1].tobytes()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nan_and_inf_are_literal_and_poison_until_the_state_is_zeroed(bad):
    _, c = _bands(3, 5)
    L, R = M.noise(6, 200), M.noise(7, 200)
    Lb = L.copy()
    Lb[50] = bad
    oL, oR, st = T.Engine.eq_ref(Lb, R, c)
    mL, mR, mst = M.row(Lb, R, c)
    assert np.array_equal(bits(oL), bits(mL)) and np.array_equal(bits(oR), bits(mR)) and st.tobytes() == mst.tobytes()
    assert np.isfinite(oL[:50]).all() and not np.isfinite(oL[50]) and np.isfinite(oR).all()
    assert np.isnan(st[0]).any() and np.isfinite(st[1]).all()
    # the row stays poisoned over clean frames, and recovers only from a zeroed state
    nL, _, st2 = T.Engine.eq_ref(L, R, c, st)
    assert np.isnan(nL).all() and np.isnan(st2[0]).any()
    cL, cR, _ = T.Engine.eq_ref(L, R, c, np.zeros_like(st))
    fL, fR, _ = T.Engine.eq_ref(L, R, c)
    assert np.array_equal(bits(cL), bits(fL)) and np.array_equal(bits(cR), bits(fR)) and np.isfinite(cL).all()


def test_cuts_equal_one_call():
    """3000 frames in one run against the same frames cut at 1, 7, 128, 129 and random points"""
    _, c = _bands(8, 77)
    L, R = M.noise(1, 3000), M.noise(2, 3000)
    oL, oR, st = T.Engine.eq_ref(L, R, c)
    rng = np.random.default_rng(9)
    for cuts in ([1], [7], [128], [129], [1, 7, 128, 129], sorted(rng.integers(1, 3000, 12).tolist())):
        at, s, gl, gr = [0] + list(cuts) + [3000], None, [], []
        for a, b in zip(at[:-1], at[1:]):
            l, r, s = T.Engine.eq_ref(L[a:b], R[a:b], c, s)
            gl.append(l), gr.append(r)
        assert np.array_equal(bits(np.concatenate(gl)), bits(oL)) and np.array_equal(bits(np.concatenate(gr)), bits(oR)), cuts
        assert s.tobytes() == st.tobytes(), cuts


def test_a_row_without_bands_passes_every_pattern_through():
    """nb = 0: the output's bits are the input's for every non-NaN float pattern tried (all 2^16 upper
    halves with three lower halves each, so every exponent, both zeros, the subnormals and the
    infinities), and a NaN goes in and a NaN comes out"""
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    pat = np.concatenate([hi, hi | 1, hi | 0xFFFF, np.random.default_rng(3).integers(0, 1 << 32, 50000, dtype=np.uint64).astype(np.uint32)])
    x = pat.view(np.float32)
    with np.errstate(all="ignore"):
        oL, oR, st = T.Engine.eq_ref(x, x, np.zeros((0, 5)))
    nan = np.isnan(x)
    assert nan.sum() > 500 and (~nan).sum() > 200000 and st.size == 0
    assert np.array_equal(bits(oL)[~nan], pat[~nan]) and np.array_equal(bits(oR)[~nan], pat[~nan])
    assert np.isnan(oL[nan]).all() and np.isnan(oR[nan]).all()


# ---------------------------------------------------------------- the designer
def _corners(rate):
    """bands at the corners of the accepted ranges, just inside the open ends"""
    for hz in (0.0002 * rate * (1 + 1e-9) + 1e-9, 0.25 * rate, 0.4998 * rate * (1 - 1e-9)):
        for q in (0.1 + 1e-9, 1.0 / math.sqrt(2.0), 6.0 - 1e-9):
            for g in (-24.0, 0.0, 24.0):
                yield hz, q, g


@pytest.mark.parametrize("rate", RATES)
def test_coefficients_follow_the_formulas(rate):
    """each of the nine types at the corners of the accepted ranges: |d| <= 2^-46 max (1, |c|), a
    bound that allows libm's last place in sin, cos and pow behind 1 - cos w at the smallest w"""
    worst = 0.0
    for kind in M.TYPES:
        for hz, q, g in _corners(rate):
            c, m = T.Engine.eq_coeffs(P.eq_band(kind, hz, q, g), rate), M.coeffs(kind, hz, q, g, rate)
            d = np.abs(c - m)
            worst = max(worst, float(d.max()))
            assert (d <= 2.0 ** -46 * np.maximum(1.0, np.abs(m))).all(), (rate, kind, hz, q, g, c, m)
    print(f"{rate}: largest coefficient difference {worst}")


@pytest.mark.parametrize("rate", RATES)
def test_designed_gain_at_the_band_frequency(rate):
    """|H| at hz from the five doubles: gain_db for PEQ, 0 dB for APF, below -200 dB for the notch,
    -3.0103 dB at q = 1 / sqrt 2 for LPF and HPF; 1e-9 dB"""
    half = 20.0 * math.log10(1.0 / math.sqrt(2.0))
    for hz in (0.001 * rate, 0.01 * rate, 0.1 * rate, 0.25 * rate, 0.4 * rate):
        for q in (0.3, 1.0 / math.sqrt(2.0), 4.0):
            for g in (-24.0, -3.0, 0.0, 6.0, 24.0):
                peq = M.gain_db(T.Engine.eq_coeffs(P.eq_band(P.EQ_PEQ, hz, q, g), rate), hz, rate)
                assert abs(peq - g) <= 1e-9, (rate, hz, q, g, peq)
            apf = M.gain_db(T.Engine.eq_coeffs(P.eq_band(P.EQ_APF, hz, q), rate), hz, rate)
            assert abs(apf) <= 1e-9, (rate, hz, q, apf)
            notch = M.gain_db(T.Engine.eq_coeffs(P.eq_band(P.EQ_NOTCH, hz, q), rate), hz, rate)
            assert notch < -200.0, (rate, hz, q, notch)
        for kind in (P.EQ_LPF, P.EQ_HPF):
            got = M.gain_db(T.Engine.eq_coeffs(P.eq_band(kind, hz, 1.0 / math.sqrt(2.0)), rate), hz, rate)
            assert abs(got - half) <= 1e-9 and abs(half + 3.0103) < 1e-5, (rate, kind, hz, got)


def test_the_whirl_filters_come_from_the_same_designer(oracle):
    """the horn's two filters of the oracle's whirl, which is pinned to the reference's setIIRFilter:
    wherever their type, Hz, Q and gain lie inside the equaliser's ranges, tbf_debug_eq_coeffs of
    them, rounded to float, gives the floats of the whirl's biquad.  At three rates, at the default
    settings (filter a, a low-pass, whose default gain of -30 dB lies outside the range and enters
    nothing: 0 is passed) and over the type and gain controls of both filters, so that all nine
    types are met."""
    from orc_bind import Chain, Template
    seen = set()
    for sr in (44100.0, 48000.0, 96000.0):
        ch = Chain(oracle, Template(oracle, sr=sr, seed=7), 1)

        def compare(what):
            f = np.zeros(24, np.float64)
            assert oracle.orc_whirl_fields(ch.ptr, f.ctypes.data_as(C.POINTER(C.c_double))) == 24
            for o in (0, 9):
                kind, hz, q, g = int(f[o]), f[o + 1], f[o + 2], f[o + 3]
                if kind < 6 and what == "default":
                    g = 0.0
                if abs(g) > 24.0:
                    continue
                c = T.Engine.eq_coeffs(P.eq_band(kind, hz, q, g), int(sr))
                want = f[o + 4:o + 9].astype(np.float32)   # a1, a2, b0, b1, b2
                got = np.array([c[3], c[4], c[0], c[1], c[2]]).astype(np.float32)
                assert np.array_equal(bits(got), bits(want)), (sr, what, o, kind, hz, q, g, got, want)
                seen.add((sr, kind))

        compare("default")
        for ab in "ab":
            for gv in (40, 64, 90):
                ch.control(f"whirl.horn.filter.{ab}.gain", gv)
                for tv in range(0, 128, 7):
                    ch.control(f"whirl.horn.filter.{ab}.type", tv)
                    compare((ab, gv, tv))
    assert seen == {(sr, k) for sr in (44100.0, 48000.0, 96000.0) for k in range(9)}


# ---------------------------------------------------------------- refusals
def test_every_range_edge_is_refused_naming_row_and_band():
    lib = T.load_library()
    ok = dict(kind=P.EQ_PEQ, hz=1000.0, q=1.0, gain_db=3.0)
    rate = 48000
    T.Engine.eq_coeffs(P.eq_band(**ok), rate)
    edges = [
        (dict(kind=-1), "type"), (dict(kind=9), "type"),
        (dict(q=0.1), "q"), (dict(q=6.0), "q"), (dict(q=float("nan")), "q"),
        (dict(hz=0.0002 * rate), "hz"), (dict(hz=0.4998 * rate), "hz"), (dict(hz=float("nan")), "hz"), (dict(hz=-5.0), "hz"),
        (dict(gain_db=24.000001), "gain_db"), (dict(gain_db=-24.000001), "gain_db"), (dict(gain_db=float("nan")), "gain_db"),
    ]
    for kw, word in edges:
        with pytest.raises(T.TbfError, match=rf"-22.*row 0 band 0.*{word}"):
            T.Engine.eq_coeffs(P.eq_band(**{**ok, **kw}), rate)
    for kw in (dict(q=0.1000001), dict(q=5.999999), dict(gain_db=24.0), dict(gain_db=-24.0), dict(hz=0.00020001 * rate),
               dict(hz=0.49979 * rate)):
        assert np.isfinite(T.Engine.eq_coeffs(P.eq_band(**{**ok, **kw}), rate)).all()
    for bad_rate in (7999, 192001, 0):
        with pytest.raises(T.TbfError, match="-22.*rate_hz"):
            T.Engine.eq_coeffs(P.eq_band(**ok), bad_rate)
    c5 = np.zeros(5)
    b = np.array(P.eq_band(**ok)).reshape(1)
    f = lib.tbf_debug_eq_coeffs
    f.restype, f.argtypes = C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p]
    assert f(rate, None, c5.ctypes.data) == -22 and "band is NULL" in _err()
    assert f(rate, b.ctypes.data, None) == -22 and "c5 is NULL" in _err()


def test_host_only_engine_validates_then_refuses():
    lib = T.load_library()
    eng = T.Engine(sample_rate=48000.0, device=-1)
    h = C.c_void_p()

    def create(n, rate, mb, e=eng._h, out=C.byref(h)):
        cfg = E.EqConfig(rate, mb)
        return lib.tbf_eq_create(e, n, C.byref(cfg), out)

    assert create(4, 48000, 8) == -19 and "host-only" in _err()
    with pytest.raises(T.TbfError, match="-19"):
        eng.equalizer(4)
    for args, word in (((0, 48000, 8), "n_rows"), ((4, 7999, 8), "rate_hz"), ((4, 192001, 8), "rate_hz"), ((4, 48000, 0), "max_bands"),
                       ((4, 48000, 9), "max_bands")):
        assert create(*args) == -22 and word in _err(), args
    assert create(4, 48000, 8, e=None) == -22 and create(4, 48000, 8, out=None) == -22
    assert lib.tbf_eq_create(eng._h, 4, None, C.byref(h)) == -22 and "cfg" in _err()
    assert h.value is None
    eng.close()


def test_null_equalizer_and_hook_refusals():
    lib = T.load_library()
    n = C.c_uint32()
    assert lib.tbf_eq_destroy(None) == 0
    assert lib.tbf_eq_reset(None, 0, None, None) == -22
    assert lib.tbf_eq_set(None, 0, None, None, None, None) == -22
    assert lib.tbf_eq_bands(None, 0, None, 0, C.byref(n)) == -22
    assert lib.tbf_eq_device(None, None, None, 0, 0, None, None, 0, None, None) == -22
    assert lib.tbf_debug_eq_time(None, 0, None, None) == -22
    x = np.zeros(4, np.float32)
    f = lib.tbf_debug_eq_ref
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    c, st = np.zeros(45), np.zeros(36)
    assert f(c.ctypes.data, 9, x.ctypes.data, x.ctypes.data, 4, st.ctypes.data, x.ctypes.data, x.ctypes.data) == -22
    assert f(None, 1, x.ctypes.data, x.ctypes.data, 4, st.ctypes.data, x.ctypes.data, x.ctypes.data) == -22
    assert f(c.ctypes.data, 1, x.ctypes.data, x.ctypes.data, 4, None, x.ctypes.data, x.ctypes.data) == -22
    assert f(c.ctypes.data, 1, None, x.ctypes.data, 4, st.ctypes.data, x.ctypes.data, x.ctypes.data) == -22
    assert f(None, 0, None, None, 0, None, None, None) == 0


# ---------------------------------------------------------------- what must not move
def test_abi_version_grid_and_structs():
    header = (ROOT / "include" / "tbf.h").read_text()
    assert re.search(r"#define\s+TBF_ABI_VERSION\s+1\b", header) and T.load_library().tbf_abi_version() == 1
    assert C.sizeof(E.EqConfig) == 8 and P.EQ_BAND_DTYPE.itemsize == 32
    assert (P.EQ_LPF, P.EQ_HPF, P.EQ_BPF0, P.EQ_BPF1, P.EQ_NOTCH, P.EQ_APF, P.EQ_PEQ, P.EQ_LOW, P.EQ_HIGH) == M.TYPES
    for name, v in zip(("LPF", "HPF", "BPF0", "BPF1", "NOTCH", "APF", "PEQ", "LOW", "HIGH"), M.TYPES):
        assert re.search(rf"#define\s+TBF_EQ_{name}\s+{v}\b", header)
    want = {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 6: 8, 7: 8, 8: 8}
    for mb, p in want.items():
        lanes, rows, tile, lds = T.Engine.eq_grid(mb)
        assert lanes == p and rows == 32 // p and tile >= 8 and 0 < lds <= 160 * 1024
    for mb in (0, 9):
        with pytest.raises(T.TbfError, match="-22.*max_bands"):
            T.Engine.eq_grid(mb)
