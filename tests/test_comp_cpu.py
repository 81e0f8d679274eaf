"""The bus compressor without a GPU: the host restatement of the definition (tbf_debug_comp_ref) against
the plain-Python model in bits, the curve lookup, the designer against the dB formula, the step
response, the pass-through of a flat curve, cuts, the order of the recurrence, and the refusals.

The stage is this project's own definition (include/tbf.h); the kernel is held
to the restatement in bits by tests/test_gpu_comp.py."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

import comp_model as M

T = pytest.importorskip("tunebfree_amd")
E = T.engine
P = T.params
bits = M.bits
F32 = np.float32
ROOT = Path(__file__).resolve().parents[1]
FLAT = np.ones(M.POINTS, F32)
NEAR1 = float(np.nextafter(F32(1.0), F32(0.0)))


def _err():
    return T.load_library().tbf_last_error().decode()


def _special(n, seed):
    """noise that spans the grid and leaves it at both ends, with +-0, subnormal floats, +-Inf and NaN"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * np.exp2(rng.uniform(-20.0, 9.5, n))).astype(F32)
    if n > 60:
        x[3:13] = [0.0, -0.0, 1e-42, -3e-45, 2.0 ** -16, np.nextafter(F32(2.0 ** -16), F32(0)), 256.0, np.nextafter(F32(256), F32(0)),
                   3e38, -300.0]
        x[30], x[31], x[45] = np.inf, -np.inf, np.nan
    return x


# ---------------------------------------------------------------- the restatement against the model
@pytest.mark.parametrize("a,r", [(0.0, 0.0), (0.0, NEAR1), (1e-3, 0.5), (NEAR1, 1e-3), (0.9, 0.999), (NEAR1, NEAR1)])
def test_ref_equals_the_model_in_bits(a, r):
    """g carried over three calls; levels below 2^-16, at and above 2^8, +-0, denormals, Inf and NaN"""
    pts = P.comp_curve(-30.0, 4.0, 6.0)
    g = mg = F32(1.0)
    for k, n in enumerate((211, 1, 300)):
        L, R = _special(n, 20 + k), _special(n, 30 + k)
        R[45 % n] = 0.5  # a NaN in one channel only: the other is the level
        oL, oR, g, gains = T.Engine.comp_ref(L, R, pts, a, r, 1.75, g)
        mL, mR, mg, mgains = M.row(L, R, pts, a, r, 1.75, mg)
        assert np.array_equal(bits(gains), bits(mgains)), (a, r, k)
        assert M.same(oL, mL) and M.same(oR, mR), (a, r, k)
        assert np.isnan(oL).sum() == np.isnan(L).sum()
        assert bits(g) == bits(mg) and np.isfinite(gains).all() and gains.min() >= 0.0 and gains.max() <= 1.0


def test_ref_with_a_key_equals_the_model_and_nan_rows_keep_g_finite():
    pts = P.comp_curve(-20.0, np.inf, 0.0)
    L, R = M.noise(1, 150), M.noise(2, 150)
    kl, kr = _special(150, 3), _special(150, 4)
    oL, oR, g, gains = T.Engine.comp_ref(L, R, pts, 0.3, 0.99, 1.0, 1.0, key=(kl, kr))
    mL, mR, mg, mgains = M.row(L, R, pts, 0.3, 0.99, 1.0, 1.0, key=(kl, kr))
    assert np.array_equal(bits(gains), bits(mgains)) and M.same(oL, mL) and M.same(oR, mR) and bits(g) == bits(mg)
    nan = np.full(64, np.nan, F32)
    oL, oR, g, gains = T.Engine.comp_ref(nan, nan, pts, 0.3, 0.99, 1.0, 0.25)
    assert np.isnan(oL).all() and np.isfinite(gains).all() and 0.25 < g <= 1.0  # the level of a NaN is 0: release


# ---------------------------------------------------------------- the lookup
def test_lookup_grid_levels_clamps_and_monotony():
    pts = P.comp_curve(-40.0, 3.0, 10.0)
    lv = M.levels().astype(F32)
    assert np.array_equal(lv.astype(np.float64), M.levels())  # the grid is exact in float32
    assert np.array_equal(bits(T.Engine.comp_lookup(pts, lv)), bits(pts))
    assert np.array_equal(lv.astype(np.float64), P.comp_levels())
    ramp = np.linspace(1.0, 0.25, M.POINTS).astype(F32)  # no two points equal: the clamps show
    below = np.array([0.0, 1e-45, 1e-38, np.nextafter(F32(2.0 ** -16), F32(0))], F32)
    above = np.array([256.0, np.nextafter(F32(256.0), F32(np.inf)), 1e30, np.inf], F32)
    assert (T.Engine.comp_lookup(ramp, below) == ramp[0]).all() and (T.Engine.comp_lookup(ramp, above) == ramp[-1]).all()
    assert ramp[-2] > T.Engine.comp_lookup(ramp, [254.0])[0] > ramp[-1]  # the last segment's middle: not clamped
    # monotone on a monotone curve: levels in order across segment and octave borders
    rng = np.random.default_rng(5)
    x = np.sort(np.exp2(rng.uniform(-17.0, 8.5, 20000)).astype(F32))
    t = T.Engine.comp_lookup(pts, x)
    assert (np.diff(pts.astype(np.float64)) <= 0).all() and (np.diff(t.astype(np.float64)) <= 0).all()
    tm = np.array([M.lookup(pts, v) for v in x[::97]], F32)
    assert np.array_equal(bits(t[::97]), bits(tm))


@pytest.mark.parametrize("ratio", [2.0, 4.0, np.inf])
def test_lookup_interpolation_bound_on_a_power_law(ratio):
    """Above the threshold c the gain is (p / c)^k with k = 1 / ratio - 1.  Linear interpolation over a
    segment of width w errs by at most max |f''| w^2 / 8 = |k (k - 1)| p^(k - 2) w^2 / 8, relative to
    f = p^k that is |k (k - 1)| (w / p)^2 / 8 <= |k (k - 1)| (1 / 32)^2 / 8, because a segment is 1 / 32
    of its octave's start and p is no smaller.  Float rounding on top: each point is rounded once (the
    interpolation is a convex mix of two, so at most 2^-24 of the larger, which exceeds the value by at
    most the factor (1 + 1 / 32)^|k| < 1.04), the subtraction errs by 2^-24 of a difference that is
    itself < 0.04 of the value, and the fmaf rounds once: 2^-24 (1.04 + 0.04 + 1) < 3 * 2^-24."""
    k = (0.0 if np.isinf(ratio) else 1.0 / ratio) - 1.0
    c = 2.0 ** -6
    pts = np.minimum(1.0, (M.levels() / c) ** k).astype(F32)
    rng = np.random.default_rng(int(min(ratio, 99)))
    p = np.exp2(rng.uniform(-6.0 + 2.0 / 32.0, 8.0, 50000)).astype(F32)  # a segment and more beyond the knee
    p = p[p < 256.0]
    t = T.Engine.comp_lookup(pts, p).astype(np.float64)
    want = (p.astype(np.float64) / c) ** k
    rel = np.abs(t - want) / want
    bound = (1.0 / 32.0) ** 2 / 8.0 * abs(k * (k - 1.0)) + 3.0 * 2.0 ** -24
    print(f"ratio {ratio}: largest relative error {rel.max():.4g}, bound {bound:.4g}")
    assert rel.max() <= bound
    assert rel.max() > 0.5 * (bound - 3.0 * 2.0 ** -24)  # the bound is about the error, not far above it


# ---------------------------------------------------------------- the designer
@pytest.mark.parametrize("T_db,ratio,knee", [(-20.0, 4.0, 0.0), (-20.0, 4.0, 6.0), (-90.0, 20.0, 40.0), (0.0, 2.0, 12.0),
                                             (-35.5, np.inf, 0.0), (-12.0, np.inf, 9.0), (-6.0, 1.5, 3.0)])
def test_designer_against_the_db_formula(T_db, ratio, knee):
    """The library computes 20 log10 (level), the piecewise y, and 10^((y - x) / 20) in double and rounds
    once to float.  Against the same formula in numpy's double: the two doubles differ by libm's error,
    a few 2^-53 on numbers below 200 (dB) turned into a relative error of the gain by ln (10) / 20 < 0.12
    per dB, so < 1e-13 relative; the one rounding to float is 2^-24 relative (the gains here are normal
    floats: the smallest, ratio +Inf at 48 dB over -90, is 1e-7).  Bound: want (2^-24 + 1e-12)."""
    pts = P.comp_curve(T_db, ratio, knee)
    want = M.design(T_db, ratio, knee)
    assert pts.dtype == np.float32 and pts.shape == (M.POINTS,)
    assert (np.abs(pts.astype(np.float64) - want) <= want * (2.0 ** -24 + 1e-12)).all()
    assert pts.max() <= 1.0 and pts.min() > 0.0 and (np.diff(pts.astype(np.float64)) <= 0).all()
    x = 20.0 * np.log10(M.levels())
    assert (pts[2.0 * (x - T_db) < -knee - 1e-9] == 1.0).all()
    # against `math`, point by point, on a few
    for i in (0, 100, 400, 555, 768):
        xi = 20.0 * math.log10(M.levels()[i])
        s = 0.0 if math.isinf(ratio) else 1.0 / ratio
        if 2.0 * (xi - T_db) < -knee:
            y = xi
        elif 2.0 * abs(xi - T_db) <= knee:
            y = xi + (s - 1.0) * (xi - T_db + knee / 2.0) ** 2 / (2.0 * knee) if knee else xi
        else:
            y = T_db + (xi - T_db) * s
        w = min(1.0, 10.0 ** ((y - xi) / 20.0))
        assert abs(float(pts[i]) - w) <= w * (2.0 ** -24 + 1e-12), i


def test_designer_soft_knee_is_continuous_ratio_one_is_flat_and_ranges_are_refused():
    # continuity: in dB the curve's slope lies in [1 / R - 1, 0], so neighbouring points, 6.02 / 32 dB
    # apart at most, differ by no more than that step in dB (and a rounding each)
    pts = P.comp_curve(-24.0, 8.0, 12.0).astype(np.float64)
    db = 20.0 * np.log10(pts)
    step = 20.0 * np.log10(M.levels()[1:] / M.levels()[:-1])
    assert (np.diff(db) <= 1e-5).all() and (np.diff(db) >= -step * (1.0 - 1.0 / 8.0) - 1e-5).all()
    # and the knee's ends meet the straight parts: the formula at x = T -+ W / 2
    x = 20.0 * np.log10(M.levels())
    hard = P.comp_curve(-24.0, 8.0, 0.0).astype(np.float64)
    outside = np.abs(x - (-24.0)) > 6.0
    assert np.array_equal(pts[outside], hard[outside])
    assert (pts[~outside] <= hard[~outside]).all()  # the knee only takes gain away
    assert np.array_equal(P.comp_curve(-20.0, 1.0, 0.0), FLAT) and np.array_equal(P.comp_curve(-90.0, 1.0, 40.0), FLAT)
    for args, word in (((-90.5, 4.0, 0.0), "threshold_db"), ((0.5, 4.0, 0.0), "threshold_db"), ((np.nan, 4.0, 0.0), "threshold_db"),
                       ((-20.0, 0.99, 0.0), "ratio"), ((-20.0, np.nan, 0.0), "ratio"), ((-20.0, -np.inf, 0.0), "ratio"),
                       ((-20.0, 4.0, -0.1), "knee_db"), ((-20.0, 4.0, 40.5), "knee_db"), ((-20.0, 4.0, np.nan), "knee_db")):
        with pytest.raises(T.TbfError, match="-22.*" + word):
            P.comp_curve(*args)
    assert T.load_library().tbf_comp_curve_design(-20.0, 4.0, 0.0, None) == -22 and "pts is NULL" in _err()


def test_comp_row_helper():
    r = P.comp_row(3, 5.0, 120.0, 6.0, rate=44100)
    assert r["curve"] == 3 and r["attack"] == F32(math.exp(-1.0 / (5e-3 * 44100))) and r["release"] == F32(math.exp(-1.0 / (0.12 * 44100)))
    assert r["makeup"] == F32(10.0 ** 0.3)
    d = P.comp_row()
    assert (d["curve"], d["attack"], d["release"], d["makeup"]) == (0, 0.0, 0.0, 1.0)
    assert P.COMP_ROW_DTYPE.itemsize == 16 and P.COMP_METER_DTYPE.itemsize == 8 and C.sizeof(E.CompConfig) == 4


# ---------------------------------------------------------------- the recurrence
@pytest.mark.parametrize("a,r", [(0.5, 0.9), (0.99, 0.999), (0.999, 0.5)])
def test_step_response(a, r):
    """A constant level above the threshold holds the target at t: in exact arithmetic g[n] - t =
    a^n (1 - t) from g = 1.  A frame rounds twice, d = g - t and the fmaf's result; both lie in [-1, 1],
    so each rounding errs by at most half an ulp of a number no larger than 1, 2^-25.  d's error is
    then multiplied by the coefficient, which is below 1, and so is the error that g carries from the
    frame before (it enters through d).  A frame therefore adds less than 2^-25 + 2^-25 = 2^-24 to an
    error that does not grow on its own: after n frames it is at most n roundings of 2^-24.  Then
    silence: t = 1, d < 0, g[n] = 1 - r^n (1 - g0), likewise."""
    a, r = float(F32(a)), float(F32(r))
    pts = P.comp_curve(-20.0, 4.0, 0.0)
    n = 400
    x = np.full(n, 0.5, F32)
    t = float(T.Engine.comp_lookup(pts, x[:1])[0])
    assert 0.0 < t < 1.0
    _, _, g0, gains = T.Engine.comp_ref(x, x, pts, a, r, 1.0)
    k = np.arange(1, n + 1)
    assert (np.abs(gains.astype(np.float64) - (t + a ** k * (1.0 - t))) <= k * 2.0 ** -24).all()
    assert (np.diff(gains.astype(np.float64)) <= 0).all()
    z = np.zeros(n, F32)
    _, _, g1, rel = T.Engine.comp_ref(z, z, pts, a, r, 1.0, g0)
    assert (np.abs(rel.astype(np.float64) - (1.0 - r ** k * (1.0 - float(g0)))) <= k * 2.0 ** -24).all()
    assert (np.diff(rel.astype(np.float64)) >= 0).all() and g1 <= 1.0


def test_flat_curve_with_makeup_one_is_the_identity_in_bits():
    L, R = _special(500, 7), _special(500, 8)
    for a, r in ((0.0, 0.0), (0.9, 0.999)):
        oL, oR, g, gains = T.Engine.comp_ref(L, R, FLAT, a, r, 1.0)
        ok = ~np.isnan(L)
        assert np.array_equal(bits(oL)[ok], bits(L)[ok]) and np.isnan(oL[~ok]).all() and (~ok).sum() == 1
        assert np.array_equal(bits(oR)[~np.isnan(R)], bits(R)[~np.isnan(R)])
        assert bits(g) == bits(F32(1.0)) and (bits(gains) == bits(F32(1.0))).all()


@pytest.mark.parametrize("cut", [1, 3, 127])
def test_cuts_of_the_restatement(cut):
    pts = P.comp_curve(-30.0, 6.0, 4.0)
    n = 700
    L, R = _special(n, 11), _special(n, 12)
    oL, oR, g, gains = T.Engine.comp_ref(L, R, pts, 0.7, 0.995, 2.5)
    cg, pl, pr, pg = F32(1.0), [], [], []
    for s in range(0, n, cut):
        a, b, cg, c = T.Engine.comp_ref(L[s:s + cut], R[s:s + cut], pts, 0.7, 0.995, 2.5, cg)
        pl.append(a), pr.append(b), pg.append(c)
    assert M.same(np.concatenate(pl), oL) and M.same(np.concatenate(pr), oR)
    assert np.array_equal(bits(np.concatenate(pg)), bits(gains)) and bits(cg) == bits(g)


def test_the_order_of_the_recurrence_is_observable():
    """g = 1, t = 0.2f, a = 0.9f: the definition's fmaf (a, g - t, t) against a * g + (1 - a) * t in
    float32, which is the same number in exact arithmetic and other bits"""
    a, t = F32(0.9), F32(0.2)
    pts = np.full(M.POINTS, t, F32)
    x = np.full(1, 0.5, F32)
    _, _, g, _ = T.Engine.comp_ref(x, x, pts, a, 0.0, 1.0)
    assert bits(g) == bits(M.step(F32(1.0), t, a, F32(0.0)))
    other = F32(F32(a * F32(1.0)) + F32(F32(F32(1.0) - a) * t))
    assert abs(float(other) - float(g)) < 1e-6 and bits(other) != bits(g)


# ---------------------------------------------------------------- refusals
def _ref_raw():
    f = T.load_library().tbf_debug_comp_ref
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                  C.c_void_p, C.c_void_p, C.c_void_p]
    return f


def test_ref_and_lookup_refusals():
    x = np.linspace(0.1, 0.9, 8).astype(F32)
    for kw, word in ((dict(attack=1.0), "row 0: attack"), (dict(attack=-0.1), "row 0: attack"), (dict(attack=np.nan), "row 0: attack"),
                     (dict(release=1.0), "row 0: release"), (dict(release=np.nan), "row 0: release"),
                     (dict(makeup=256.5), "row 0: makeup"), (dict(makeup=-1.0), "row 0: makeup"), (dict(makeup=np.inf), "row 0: makeup"),
                     (dict(makeup=np.nan), "row 0: makeup"), (dict(g=1.5), "g "), (dict(g=np.nan), "g ")):
        with pytest.raises(T.TbfError, match="-22.*" + word):
            T.Engine.comp_ref(x, x, FLAT, **kw)
    for i, v in ((0, 1.5), (400, -0.25), (768, np.nan), (5, np.inf), (9, -0.0)):
        bad = FLAT.copy()
        bad[i] = v
        with pytest.raises(T.TbfError, match=f"-22.*point {i}:"):
            T.Engine.comp_ref(x, x, bad)
        with pytest.raises(T.TbfError, match=f"-22.*point {i}:"):
            T.Engine.comp_lookup(bad, x)
    for v in (-1.0, np.nan):
        with pytest.raises(T.TbfError, match="-22.*level 2"):
            T.Engine.comp_lookup(FLAT, [0.0, 1.0, v])
    f, g, o = _ref_raw(), np.ones(1, F32), np.zeros(8, F32)
    xp, gp, op, pp = x.ctypes.data, g.ctypes.data, o.ctypes.data, FLAT.ctypes.data
    assert f(None, 0, 0, 1, xp, xp, None, None, 8, gp, op, op, None) == -22 and "pts is NULL" in _err()
    assert f(pp, 0, 0, 1, xp, xp, None, None, 8, None, op, op, None) == -22 and "g is NULL" in _err()
    assert f(pp, 0, 0, 1, None, xp, None, None, 8, gp, op, op, None) == -22 and "plane" in _err()
    assert f(pp, 0, 0, 1, xp, xp, xp, None, 8, gp, op, op, None) == -22 and "key" in _err()
    assert f(pp, 0, 0, 1, None, None, None, None, 0, gp, None, None, None) == 0
    assert g[0] == 1.0  # no refusal moved it


def test_host_only_engine_validates_then_refuses():
    lib = T.load_library()
    eng = T.Engine(sample_rate=48000.0, device=-1)
    h = C.c_void_p()

    def create(n, nc, e=eng._h, out=C.byref(h)):
        cfg = E.CompConfig(nc)
        return lib.tbf_comp_create(e, n, C.byref(cfg), out)

    assert create(4, 8) == -19 and "host-only" in _err()
    with pytest.raises(T.TbfError, match="-19"):
        eng.compressor(4)
    for args, word in (((0, 1), "n_rows"), ((4, 0), "n_curves"), ((4, 9), "n_curves")):
        assert create(*args) == -22 and word in _err(), args
    assert create(4, 1, e=None) == -22 and "engine is NULL" in _err()
    assert create(4, 1, out=None) == -22 and "out is NULL" in _err()
    assert lib.tbf_comp_create(eng._h, 4, None, C.byref(h)) == -22 and "cfg" in _err()
    assert h.value is None
    eng.close()


def test_null_compressor_refusals_and_grid():
    lib = T.load_library()
    assert lib.tbf_comp_destroy(None) == 0
    for call in (lambda: lib.tbf_comp_reset(None, 0, None, None), lambda: lib.tbf_comp_curve_set(None, 0, None, None),
                 lambda: lib.tbf_comp_rows_set(None, 0, None, None, None), lambda: lib.tbf_comp_curve_get(None, 0, None),
                 lambda: lib.tbf_comp_row_get(None, 0, None),
                 lambda: lib.tbf_comp_device(None, None, None, 0, 0, None, None, 0, None, None, 0, None, None, None),
                 lambda: lib.tbf_debug_comp_time(None, 0, None, None)):
        assert call() == -22 and "comp is NULL" in _err()
    header = (ROOT / "include" / "tbf.h").read_text()
    for name, v in (("MAX_CURVES", "8u"), ("SEG", "32u"), ("POINTS", "769u"), ("MAX_MAKEUP", "256.0f")):
        assert re.search(rf"#define\s+TBF_COMP_{name}\s+{re.escape(v)}", header)
    assert (P.COMP_MAX_CURVES, P.COMP_SEG, P.COMP_POINTS, P.COMP_MAX_MAKEUP) == (8, 32, 769, 256.0)
    seen = set()
    for n in (1, 2, 64, 4096, 8192, 8193, 100000):
        for nc in (1, 8):
            rpw, tile, lds = T.Engine.comp_grid(n, nc)
            seen.add(rpw)
            assert 1 <= rpw <= 64 and tile % 64 == 0 and tile >= 64 and 0 < lds <= 160 * 1024
            assert lds >= 4 * (3 * rpw * tile + nc * 769)
    assert len(seen) >= 1 and T.Engine.comp_grid(2)[0] == min(seen)
    for n, nc, word in ((0, 1, "n_rows"), (4, 0, "n_curves"), (4, 9, "n_curves")):
        with pytest.raises(T.TbfError, match="-22.*" + word):
            T.Engine.comp_grid(n, nc)
