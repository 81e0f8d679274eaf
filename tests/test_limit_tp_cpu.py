"""The bus limiter with a true-peak detector without a GPU: the host restatement
(tbf_debug_limit_tp_ref, built from the headers k_limit_tp is built from) against the numpy model
in bits, cuts into calls, transparency, the literal NaN / Inf cases, the quarter-rate sine that the
plain limiter passes and this one reduces, the steady-state bound on the output's true peak, and
the refusals of tbf_limiter_create_tp."""
import ctypes as C

import numpy as np
import pytest

import limit_model as LM
import limit_tp_model as M
import truepeak_model as TP

T = pytest.importorskip("tunebfree_amd")
E = T.engine

CEIL = M.CEILING
CONFIGS = [(2, 0, 4), (64, 1, 4), (64, 1, 2), (16, 5, 4)]
N = 700
bits = LM.bits


def _input():
    return LM.issue_input(5001, N), LM.issue_input(5002, N)


_one = {}


def _ref(A, H, F):
    """one tbf_debug_limit_tp_ref run of the issue's material under a configuration, computed once"""
    if (A, H, F) not in _one:
        L, R = _input()
        _one[A, H, F] = T.Engine.limit_ref(L, R, CEIL, A, H, oversample=F)
    return _one[A, H, F]


def _err():
    return T.load_library().tbf_last_error().decode()


# ---------------------------------------------------------------- 1. mirrors
def test_tp_structs_grid_and_abi():
    lib = T.load_library()
    assert lib.tbf_abi_version() == 1
    assert C.sizeof(E.LimiterDetect) == 8 and C.sizeof(E.LimiterConfig) == 12 and C.sizeof(E.LimitOut) == 32
    assert [f[0] for f in E.LimiterDetect._fields_] == ["oversample", "reserved"]
    for A, H in [(2, 0), (16, 5), (64, 0), (64, 1), (64, 200), (512, 4096)]:
        g0, tile0, hn0, lds0 = T.Engine.limit_grid(CEIL, A, H)
        for F in (2, 4):
            g, tile, hn, lds = T.Engine.limit_grid(CEIL, A, H, oversample=F)
            assert hn == M.history(A, H) == 2 * A + H + 9 == hn0 + M.REACH
            assert (g, tile) == (g0, tile0) and lds0 < lds <= 160 * 1024 // 2   # two workgroups a CU at the largest
            assert M.latency(A) == A + 5 <= hn                                    # the delayed input lies within the history
    for kw in (dict(oversample=3), dict(oversample=1), dict(oversample=0), dict(oversample=8)):
        with pytest.raises(T.TbfError, match="-22.*oversample"):
            T.Engine.limit_grid(CEIL, 64, 0, **kw)
    assert E.limiter_oversample(44100) == E.limiter_oversample(48000) == 4
    assert E.limiter_oversample(96000) == E.limiter_oversample(176400) == 2
    with pytest.raises(ValueError, match="plain limiter"):
        E.limiter_oversample(192000)


# ---------------------------------------------------------------- 2. identity with the model
@pytest.mark.parametrize("A,H,F", CONFIGS)
def test_tp_ref_equals_the_model_in_bits(A, H, F):
    L, R = _input()
    oL, oR, meter, hist = _ref(A, H, F)
    yL, yR, g, want, _ = M.limit_tp(L, R, CEIL, A, H, F)
    assert np.array_equal(bits(oL), bits(yL)) and np.array_equal(bits(oR), bits(yR))
    assert bits(meter["min_gain"]) == bits(want["min_gain"]) == bits(g.min())
    assert int(meter["reduced"]) == int(want["reduced"]) > 0 and int(meter["clamped"]) == int(want["clamped"])
    Hn = M.history(A, H)
    assert len(hist[0]) == len(hist[1]) == Hn
    assert np.array_equal(bits(hist[0]), bits(L[-Hn:])) and np.array_equal(bits(hist[1]), bits(R[-Hn:]))
    assert not (np.abs(oL) > CEIL).any() and not (np.abs(oR) > CEIL).any()


def test_tp_detector_differs_from_the_plain_one():
    """the same material through the plain limiter, delayed by E: other bits, so the identity above is
    no accident of a detector that sees the samples alone"""
    L, R = _input()
    oL, _, meter, _ = _ref(64, 1, 4)
    pL, _, pm, _ = T.Engine.limit_ref(L, R, CEIL, 64, 1)
    assert not np.array_equal(bits(oL[M.E:]), bits(pL[:N - M.E])) and int(meter["reduced"]) > 0 and int(pm["reduced"]) > 0


# ---------------------------------------------------------------- 3. cuts
@pytest.mark.parametrize("A,H,F", CONFIGS)
def test_tp_cuts_with_the_history_carried_equal_one_call(A, H, F):
    L, R = _input()
    oneL, oneR, one_m, one_h = _ref(A, H, F)
    D, Hn = A - 1, M.history(A, H)
    cuts = [1, 5, 6, 7, 11, 12, D + 6, Hn + 3]
    assert sum(cuts) < N
    cuts.append(N - sum(cuts))
    hist, at, gotL, gotR, reduced, clamped, ming = None, 0, [], [], 0, 0, np.float32(1.0)
    for k in cuts:
        a, b, m, hist = T.Engine.limit_ref(L[at:at + k], R[at:at + k], CEIL, A, H, hist=hist, oversample=F)
        gotL.append(a), gotR.append(b)
        reduced, clamped, ming = reduced + int(m["reduced"]), clamped + int(m["clamped"]), min(ming, m["min_gain"])
        at += k
    assert np.array_equal(bits(np.concatenate(gotL)), bits(oneL)) and np.array_equal(bits(np.concatenate(gotR)), bits(oneR))
    assert reduced == one_m["reduced"] and clamped == one_m["clamped"] and bits(ming) == bits(one_m["min_gain"])
    assert np.array_equal(bits(hist[0]), bits(one_h[0])) and np.array_equal(bits(hist[1]), bits(one_h[1]))
    _, _, m0, h0 = T.Engine.limit_ref(L[:0], R[:0], CEIL, A, H, hist=hist, oversample=F)
    assert np.array_equal(bits(h0[0]), bits(hist[0])) and m0["min_gain"] == 1.0 and m0["reduced"] == 0


# ---------------------------------------------------------------- 4. transparency
@pytest.mark.parametrize("A,H,F", CONFIGS)
def test_tp_a_row_whose_detector_stays_below_the_ceiling_comes_out_as_its_own_bits(A, H, F):
    rng = np.random.default_rng(33)
    n, lat = 1500, M.latency(A)
    rows = []
    for _ in range(2):
        u = rng.uniform(-1, 1, n)
        u[100], u[200] = -0.0, 0.0
        rows.append(u)
    # the largest magnitude the detector can see, in float64, and 1 % of room for float32's roundings
    top = max(max(np.abs(TP.y64(u, 4)).max(), np.abs(u).max()) for u in rows)
    L, R = [(u * (0.99 * float(CEIL) / top)).astype(np.float32) for u in rows]
    R[200] = np.float32(1e-41)                       # a subnormal; L[100] is a negative zero
    assert bits(L[100]) == 0x80000000 and max(np.abs(L).max(), np.abs(R).max()) > 0.4
    oL, oR, meter, _ = T.Engine.limit_ref(L, R, CEIL, A, H, oversample=F)
    assert np.array_equal(bits(oL[lat:]), bits(L[:n - lat])) and np.array_equal(bits(oR[lat:]), bits(R[:n - lat]))
    assert not bits(oL[:lat]).any() and not bits(oR[:lat]).any()   # +0.0f from before the row's start
    assert bits(oL[100 + lat]) == 0x80000000 and bits(oR[200 + lat]) == bits(np.float32(1e-41))
    assert meter["min_gain"] == 1.0 and meter["reduced"] == 0 and meter["clamped"] == 0


# ---------------------------------------------------------------- 5. the literal cases
def test_tp_nan_is_skipped_with_the_twelve_windows_it_touches():
    A, H, F, k = 16, 5, 4, 250
    L, R = _input()
    Ln = L.copy()
    Ln[k] = np.nan
    oL, oR, meter, _ = T.Engine.limit_ref(Ln, R, CEIL, A, H, oversample=F)
    own = k + M.latency(A)
    keep = np.arange(N) != own
    assert np.isnan(oL[own]) and np.isfinite(oL[keep]).all() and np.isfinite(oR).all()   # g is finite everywhere
    assert np.isfinite(meter["min_gain"]) and meter["min_gain"] > 0.0
    # the model with L's interpolated values of frames k .. k + 11 and its sample at k skipped: the
    # detector of those twelve frames is R's values and L's samples alone
    mL, mR, g, mm, _ = M.limit_tp(Ln, R, CEIL, A, H, F, nan_at=(k, None))
    assert np.isfinite(g).all() and np.isnan(mL[own])
    assert np.array_equal(bits(oL[keep]), bits(mL[keep])) and np.array_equal(bits(oR), bits(mR))
    assert bits(meter["min_gain"]) == bits(mm["min_gain"]) and meter["reduced"] == mm["reduced"]


def test_tp_only_the_twelve_frames_after_a_nan_fall_back_to_the_sample_peaks():
    """the quarter-rate sine, whose samples are under the ceiling and whose interpolated values are
    over it, with one NaN at k in L and nothing in R: t[k .. k + 11] is 1.0 (the sample peaks alone)
    and every other t of the steady part is below 1.  With A = 2, H = 0: m[j] = min (t[j-1], t[j]) is
    1.0 on k + 1 .. k + 11 and g[n] = (m[n-1] + m[n]) / 2 is 1.0 on exactly k + 2 .. k + 11."""
    A, H, F, k, n = 2, 0, 4, 300, 600
    lat = M.latency(A)
    x = _sine(n)
    xn = x.copy()
    xn[k] = np.nan
    zero = np.zeros(n, np.float32)
    cL, _, cm, _ = T.Engine.limit_ref(x, zero, CEIL, A, H, oversample=F)
    oL, oR, meter, _ = T.Engine.limit_ref(xn, zero, CEIL, A, H, oversample=F)
    d = np.concatenate([np.zeros(lat, np.float32), x[:n - lat]])
    steady = np.arange(n) >= 40
    assert (bits(cL) != bits(d))[steady].all()                       # without the NaN every steady frame is reduced
    # The sine's own t alternates: the stretch between two samples holds either a crest (p = 1.2) or a
    # zero crossing (p = the samples' 0.85, t = 1.0).  So take the frames with t = 1.0 from the model's
    # p of the clean row, add k .. k + 11, and g[n] == 1.0 where t[n-2], t[n-1], t[n] all are.
    p = M.limit_tp(x, zero, CEIL, A, H, F)[4]
    t_one = p <= CEIL
    assert 0.4 < t_one[steady].mean() < 0.6 and not (t_one[1:] & t_one[:-1])[steady[1:]].any()
    t_one[k:k + 12] = True
    idx = np.arange(n)
    unity = np.array([bool(steady[i]) and t_one[i - 2:i + 1].all() for i in idx])
    assert unity[k + 2:k + 12].all() and unity.sum() <= 12 and not unity[:k + 1].any() and not unity[k + 13:].any()
    changed = bits(oL) != bits(d)
    own = idx == k + lat                                             # the NaN's own sample
    assert np.isnan(oL[k + lat]) and not bits(oR).any()
    assert not changed[unity & ~own].any() and changed[steady & ~unity & ~own].all()
    assert int(meter["reduced"]) == int(cm["reduced"]) - int(unity.sum())


def test_tp_inf_gives_t_zero():
    A, H, F, n0, n = 16, 5, 4, 200, 500
    c = np.float32(0.5)
    x = np.full(n, 0.25, np.float32)
    L = x.copy()
    L[n0] = np.inf
    oL, oR, meter, _ = T.Engine.limit_ref(L, x, c, A, H, oversample=F)
    lat, W = M.latency(A), A + H
    assert meter["min_gain"] == 0.0 and np.isnan(oL[n0 + lat])          # 0 * Inf
    # the sample reaches p at n0 + 6, so g == 0 where all A minima see it: n in [n0 + 6 + A - 1, n0 + 6 + W - 1]
    zero = np.arange(n0 + M.E + A - 1, n0 + M.E + W)
    assert not bits(oR[zero]).any()
    assert (np.abs(oR) <= c).all() and (np.abs(oL[np.arange(n) != n0 + lat]) <= c).all()
    assert (oR[lat:n0 - 12] == 0.25).all() and (oR[n0 + 12 + W + A + lat:] == 0.25).all()


# ---------------------------------------------------------------- 6. the inter-sample peak
SINE_AMP = 1.2   # samples at 1.2 sin 45 = 0.85 < c, the waveform's peak at 1.2 > c


def _sine(n):
    x = TP.sine(n, 0.25, 45.0, SINE_AMP)
    assert float(np.abs(x).max()) < float(CEIL) < SINE_AMP
    return x


@pytest.mark.parametrize("A,H,F", [(64, 1, 4), (64, 1, 2), (16, 5, 4)])
def test_tp_quarter_rate_sine_is_reduced_where_the_plain_limiter_passes_it(A, H, F):
    x = _sine(N)
    pL, _, pm, _ = T.Engine.limit_ref(x, x, CEIL, A, H)
    assert pm["reduced"] == 0 and np.array_equal(bits(pL[A - 1:]), bits(x[:N - A + 1]))
    oL, _, meter, _ = T.Engine.limit_ref(x, x, CEIL, A, H, oversample=F)
    assert meter["reduced"] > 0 and meter["min_gain"] < 1.0
    print(f"A={A} H={H} F={F}: reduced {int(meter['reduced'])}, min_gain {float(meter['min_gain'])}")


def steady_bound(c):
    """The largest true-peak word of the output over frames of constant gain g, in float64.
    There y[i] = fl (g x[i]) = g x[i] (1 + d), |d| <= 2^-24, and an interpolated value of the output
    is a chain of 12 fmaf over such y.  With S = sum |h| < 2.03 and X = max |x| <= P, the input's
    largest detector value, and g = fl (c / P) <= (c / P) (1 + 2^-24):
      the output chain's 12 roundings, each at most 2^-24 of a partial sum <= S g X:  12 S 2^-24 c
      the 12 products' roundings, sum |h| |g x| 2^-24:                                   S 2^-24 c
      P itself is a rounded chain, off its exact value by at most 12 S 2^-24 X:        12 S 2^-24 c
      the division's rounding:                                                            2^-24 c
    together (25 S + 1) 2^-24 c < 52 x 2^-24 c, within the c (1 + 2^-18) = c (1 + 64 x 2^-24) that the
    definition states."""
    return float(c) * (1.0 + 2.0 ** -18)


def steady_words(out, start, F=4):
    """the true-peak words of out[start:] by the meter's restatement, its history the 11 frames before"""
    h = np.concatenate([out[start - 11:start], out[start - 11:start]])
    return T.Engine.true_peak_ref(out[start:], out[start:], oversample=F, hist=h)[0]


@pytest.mark.parametrize("A,H,F", [(64, 1, 4), (64, 1, 2), (16, 5, 4)])
def test_tp_steady_state_true_peak_is_within_the_bound(A, H, F):
    Hn = M.history(A, H)
    n = Hn + 12 + 11 + 400
    x = _sine(n)
    start = Hn + 12 + 11                       # g is constant from Hn_tp + 12 on; the meter's 11 frames of history too
    oL, _, meter, _ = T.Engine.limit_ref(x, x, CEIL, A, H, oversample=F)
    lat = M.latency(A)
    ratio = oL[start:].astype(np.float64) / x[start - lat:n - lat].astype(np.float64)
    assert np.ptp(ratio) < 2.0 ** -22 and meter["clamped"] == 0    # one gain, up to the product's rounding
    words = steady_words(oL, start, F)
    top = float(np.uint32(words.max()).view(np.float32))
    print(f"A={A} H={H} F={F}: steady true peak {top!r}, ceiling {float(CEIL)!r}, bound {steady_bound(CEIL)!r}")
    assert top <= steady_bound(CEIL)
    assert top > 0.99 * float(CEIL)            # and it is the ceiling that holds it, not a gain far below
    pL, _, _, _ = T.Engine.limit_ref(x, x, CEIL, A, H)
    plain = float(np.uint32(steady_words(pL, start, F).max()).view(np.float32))
    print(f"the plain limiter's output on the same frames: {plain!r}")
    assert plain > steady_bound(CEIL)          # the plain limiter's output reads over the ceiling


# ---------------------------------------------------------------- 7. host-only engines and refusals
def _create(eng, n_rows, ceiling, ahead, hold, oversample=4, reserved=0, cfg_null=False, det_null=False, out_null=False):
    lib = eng._lib
    cfg, det = E.LimiterConfig(float(ceiling), ahead, hold), E.LimiterDetect(oversample, reserved)
    h = C.c_void_p()
    return lib.tbf_limiter_create_tp(eng._h, n_rows, None if cfg_null else C.byref(cfg), None if det_null else C.byref(det),
                                     None if out_null else C.byref(h))


def test_tp_host_only_engine_validates_then_refuses():
    eng = T.Engine(sample_rate=48000.0, device=-1)
    assert _create(eng, 4, CEIL, 64, 0) == -19 and "host-only" in _err()
    assert _create(eng, 4, CEIL, 64, 0, oversample=2) == -19
    with pytest.raises(T.TbfError, match="-19"):
        eng.limiter(4, CEIL, oversample=4)
    bad = [
        (dict(n_rows=4, ceiling=CEIL, ahead=64, hold=0, oversample=3), "oversample"),
        (dict(n_rows=4, ceiling=CEIL, ahead=64, hold=0, oversample=1), "oversample"),
        (dict(n_rows=4, ceiling=CEIL, ahead=64, hold=0, oversample=0), "oversample"),
        (dict(n_rows=4, ceiling=CEIL, ahead=64, hold=0, oversample=8), "oversample"),
        (dict(n_rows=4, ceiling=CEIL, ahead=64, hold=0, reserved=1), "reserved"),
        (dict(n_rows=4, ceiling=CEIL, ahead=64, hold=0, det_null=True), "det"),
        (dict(n_rows=4, ceiling=0.0, ahead=64, hold=0), "ceiling"),
        (dict(n_rows=4, ceiling=np.nan, ahead=64, hold=0), "ceiling"),
        (dict(n_rows=4, ceiling=CEIL, ahead=48, hold=0), "ahead"),
        (dict(n_rows=4, ceiling=CEIL, ahead=1024, hold=0), "ahead"),
        (dict(n_rows=4, ceiling=CEIL, ahead=64, hold=4097), "hold"),
        (dict(n_rows=0, ceiling=CEIL, ahead=64, hold=0), "n_rows"),
        (dict(n_rows=4, ceiling=CEIL, ahead=64, hold=0, cfg_null=True), "cfg"),
        (dict(n_rows=4, ceiling=CEIL, ahead=64, hold=0, out_null=True), "out"),
    ]
    for kw, word in bad:   # validation comes before the -19
        assert _create(eng, **kw) == -22, kw
        assert word in _err(), (kw, _err())
    with pytest.raises(T.TbfError, match="-22.*oversample"):
        eng.limiter(4, CEIL, oversample=3)
    lib = eng._lib
    cfg, det, h = E.LimiterConfig(float(CEIL), 64, 0), E.LimiterDetect(4, 0), C.c_void_p()
    assert lib.tbf_limiter_create_tp(None, 4, C.byref(cfg), C.byref(det), C.byref(h)) == -22 and "engine" in _err()
    eng.close()


def test_tp_ref_refusals():
    x = np.zeros(8, np.float32)
    for kw, word in ((dict(ceiling=0.0), "ceiling"), (dict(ahead=3), "ahead"), (dict(hold=5000), "hold"),
                     (dict(oversample=3), "oversample"), (dict(oversample=1), "oversample")):
        with pytest.raises(T.TbfError, match=word):
            T.Engine.limit_ref(x, x, **{"ceiling": CEIL, "oversample": 4, **kw})
