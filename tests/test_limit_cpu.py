"""The bus limiter without a GPU: the host restatement of the definition (tbf_debug_limit_ref,
built from the header k_limit is built from) against the numpy float32 model in bits, the order
of the gain's sum made observable, the ceiling, transparency, the closed form of one peak, the
literal NaN / Inf cases, cuts into calls, and the refusals of the limiter calls."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import limit_model as M

T = pytest.importorskip("tunebfree_amd")
E = T.engine
ROOT = Path(__file__).resolve().parents[1]

CEIL = M.CEILING
CONFIGS = [(2, 0), (16, 5), (64, 0), (64, 200)]
bits = M.bits


def _case(A, H):
    n = 12000 if (A, H) == (512, 4096) else 4096
    return M.issue_input(1000 + A + H, n), M.issue_input(2000 + A + H, n)


_cache = {}


def _both(A, H):
    """(inputs, limit_ref's results, the model's) of a configuration, computed once"""
    if (A, H) not in _cache:
        L, R = _case(A, H)
        _cache[A, H] = (L, R, T.Engine.limit_ref(L, R, CEIL, A, H), M.limit(L, R, CEIL, A, H))
    return _cache[A, H]


def _err():
    return T.load_library().tbf_last_error().decode()


# ---------------------------------------------------------------- 1. mirrors
def test_constants_and_structs_mirror_the_header():
    h = (ROOT / "include" / "tbf.h").read_text()
    assert int(re.search(r"#define TBF_LIMIT_MAX_AHEAD (\d+)u", h).group(1)) == T.params.LIMIT_MAX_AHEAD == M.MAX_AHEAD == 512
    assert int(re.search(r"#define TBF_LIMIT_MAX_HOLD (\d+)u", h).group(1)) == T.params.LIMIT_MAX_HOLD == M.MAX_HOLD == 4096
    assert C.sizeof(E.LimiterConfig) == 12 and C.sizeof(E.LimitOut) == 32
    assert C.sizeof(E.LimitMeter) == T.params.LIMIT_METER_DTYPE.itemsize == M.METER_DTYPE.itemsize == 12
    assert T.params.LIMIT_METER_DTYPE == M.METER_DTYPE
    assert [f[0] for f in E.LimitMeter._fields_] == list(M.METER_DTYPE.names)
    for A, H in CONFIGS + [(512, 4096)]:
        g, tile, hn, lds = T.Engine.limit_grid(CEIL, A, H)
        assert hn == M.history(A, H) == 2 * A + H - 2
        assert g == 4 and tile % (64 * g) == 0 and lds <= 64 * 1024


# ---------------------------------------------------------------- 2. identity with the model
@pytest.mark.parametrize("A,H", CONFIGS + [(512, 4096)])
def test_ref_equals_the_model_in_bits(A, H):
    L, R, (oL, oR, meter, hist), (yL, yR, g, want, mhist) = _both(A, H)
    assert np.array_equal(bits(oL), bits(yL)) and np.array_equal(bits(oR), bits(yR))
    assert bits(meter["min_gain"]) == bits(want["min_gain"]) == bits(g.min())
    assert int(meter["reduced"]) == int(want["reduced"]) and int(meter["clamped"]) == int(want["clamped"])
    assert np.array_equal(bits(hist[0]), bits(mhist[0])) and np.array_equal(bits(hist[1]), bits(mhist[1]))
    assert np.array_equal(bits(hist[0]), bits(L[-M.history(A, H):]))


@pytest.mark.parametrize("A,H", [c for c in CONFIGS + [(512, 4096)] if c[0] >= 16])
def test_order_is_observable(A, H):
    """the gains of the descending sum differ from the ascending ones, and the outputs they give
    differ from limit_ref's, so a kernel that sums in another order cannot equal it by accident"""
    L, R, (oL, oR, _, _), (_, _, g, _, _) = _both(A, H)
    dL, dR, dg, _, _ = M.limit(L, R, CEIL, A, H, descending=True)
    ng = int((bits(g) != bits(dg)).sum())
    ny = int((bits(oL) != bits(dL)).sum() + (bits(oR) != bits(dR)).sum())
    print(f"A={A} H={H}: {ng} of {len(g)} gains and {ny} output samples differ between the two orders")
    assert ng >= 1 and ny >= 1


# ---------------------------------------------------------------- 3. the ceiling
def test_ceiling_holds_and_the_clamp_is_counted():
    any_clamped = 0
    for A, H in CONFIGS + [(512, 4096)]:
        _, _, (oL, oR, meter, _), (_, _, _, want, _) = _both(A, H)
        assert not (np.abs(oL) > CEIL).any() and not (np.abs(oR) > CEIL).any()
        assert int(meter["clamped"]) == int(want["clamped"])
        assert int(meter["reduced"]) > 0
        print(f"A={A} H={H}: clamped {int(meter['clamped'])}, reduced {int(meter['reduced'])}, min_gain {meter['min_gain']}")
        any_clamped += int(meter["clamped"])
    assert any_clamped > 0


# ---------------------------------------------------------------- 4. transparency
@pytest.mark.parametrize("A,H", CONFIGS)
def test_a_row_below_the_ceiling_comes_out_as_its_own_bits(A, H):
    rng = np.random.default_rng(31)
    n, D = 1500, A - 1
    L = (rng.uniform(-1, 1, n) * CEIL).astype(np.float32)
    R = (rng.uniform(-1, 1, n) * CEIL).astype(np.float32)
    L[100], R[200] = -0.0, np.float32(1e-41)   # a negative zero and a subnormal
    L[300], R[300] = CEIL, -CEIL               # the ceiling itself is not above it
    oL, oR, meter, _ = T.Engine.limit_ref(L, R, CEIL, A, H)
    assert np.array_equal(bits(oL[D:]), bits(L[:n - D])) and np.array_equal(bits(oR[D:]), bits(R[:n - D]))
    assert not bits(oL[:D]).any() and not bits(oR[:D]).any()   # +0.0f from before the row's start
    assert bits(oL[100 + D]) == 0x80000000 and bits(oR[200 + D]) == bits(np.float32(1e-41))
    assert meter["min_gain"] == 1.0 and meter["reduced"] == 0 and meter["clamped"] == 0


# ---------------------------------------------------------------- 5. the closed form
def test_one_peak_follows_the_closed_form():
    A, H, c, n0, n = 16, 5, np.float32(0.5), 300, 700
    W, D = A + H, A - 1
    x = np.full(n, 0.25, np.float32)
    x[n0] = 2.0
    oL, oR, meter, _ = T.Engine.limit_ref(x, x, c, A, H)
    idx = np.arange(n)
    cnt = np.clip(np.minimum(idx, n0 + W - 1) - np.maximum(idx - A + 1, n0) + 1, 0, None)
    g = (np.float32(1.0) - np.float32(0.75) * cnt.astype(np.float32) / np.float32(A)).astype(np.float32)
    d = np.concatenate([np.zeros(D, np.float32), x[:n - D]])
    want = (g * d).astype(np.float32)
    assert np.array_equal(bits(oL), bits(want)) and np.array_equal(bits(oR), bits(want))
    assert oL[n0 + D] == c and bits(oL[n0 + D]) == bits(c)
    assert bits(meter["min_gain"]) == bits(np.float32(0.25)) and meter["reduced"] == A + W - 1 and meter["clamped"] == 0
    # the model's gains are the closed form too
    assert np.array_equal(bits(M.limit(x, x, c, A, H)[2]), bits(g))


# ---------------------------------------------------------------- 6. the literal cases
def test_nan_passes_and_moves_no_gain():
    A, H = 16, 5
    L, R = _case(A, H)
    L, R = L[:600].copy(), R[:600].copy()
    clean = T.Engine.limit_ref(L, R, CEIL, A, H)
    Ln = L.copy()
    Ln[250] = np.nan
    oL, oR, meter, _ = T.Engine.limit_ref(Ln, R, CEIL, A, H)
    # its own sample comes out NaN; every other sample as if the NaN's peak were R's alone
    L0 = L.copy()
    L0[250] = 0.0
    ref0 = T.Engine.limit_ref(L0, R, CEIL, A, H)
    assert np.isnan(oL[250 + A - 1])
    keep = np.arange(600) != 250 + A - 1
    assert np.array_equal(bits(oL[keep]), bits(ref0[0][keep])) and np.array_equal(bits(oR), bits(ref0[1]))
    assert bits(meter["min_gain"]) == bits(ref0[2]["min_gain"]) and meter["reduced"] == ref0[2]["reduced"]
    mL, mR, _, mm, _ = M.limit(Ln, R, CEIL, A, H)
    assert np.array_equal(bits(oL), bits(mL)) and np.array_equal(bits(oR), bits(mR)) and mm["clamped"] == meter["clamped"]
    assert clean[2]["reduced"] > 0


def test_inf_drives_the_gain_to_zero_across_its_window():
    A, H, n0, n = 16, 5, 200, 500
    W, D = A + H, A - 1
    x = np.full(n, 0.25, np.float32)
    L = x.copy()
    L[n0] = np.inf
    oL, oR, meter, _ = T.Engine.limit_ref(L, x, np.float32(0.5), A, H)
    # g == 0 where all A minima of the sum see the Inf: n in [n0 + A - 1, n0 + W - 1]
    zero = np.arange(n0 + A - 1, n0 + W)
    assert not bits(oR[zero]).any() and meter["min_gain"] == 0.0
    assert np.isnan(oL[n0 + D]) and not bits(np.delete(oL[zero], 0)).any()   # 0 * Inf
    assert (oR[:n0] == 0.25 * (np.arange(n0) >= D)).all() and (oR[n0 + W + A:] == 0.25).all()
    mL, mR, _, _, _ = M.limit(L, x, np.float32(0.5), A, H)
    assert np.array_equal(bits(oL), bits(mL)) and np.array_equal(bits(oR), bits(mR))


# ---------------------------------------------------------------- 7. cuts
@pytest.mark.parametrize("A,H", [(16, 5), (64, 200)])
def test_cuts_with_the_history_carried_equal_one_call(A, H):
    n, D, Hn = 3000, A - 1, M.history(A, H)
    L, R = M.issue_input(77, n), M.issue_input(78, n)
    oneL, oneR, one_m, one_h = T.Engine.limit_ref(L, R, CEIL, A, H)
    cuts = [1, D, Hn - 1, Hn, Hn + 1]
    assert sum(cuts) < n
    cuts.append(n - sum(cuts))
    hist, at, gotL, gotR, reduced, clamped, ming = None, 0, [], [], 0, 0, np.float32(1.0)
    for k in cuts:
        a, b, m, hist = T.Engine.limit_ref(L[at:at + k], R[at:at + k], CEIL, A, H, hist=hist)
        gotL.append(a), gotR.append(b)
        reduced, clamped, ming = reduced + int(m["reduced"]), clamped + int(m["clamped"]), min(ming, m["min_gain"])
        at += k
    assert np.array_equal(bits(np.concatenate(gotL)), bits(oneL)) and np.array_equal(bits(np.concatenate(gotR)), bits(oneR))
    assert reduced == one_m["reduced"] and clamped == one_m["clamped"] and bits(ming) == bits(one_m["min_gain"])
    assert np.array_equal(bits(hist[0]), bits(one_h[0])) and np.array_equal(bits(hist[1]), bits(one_h[1]))
    # an empty call leaves the history as it is
    _, _, m0, h0 = T.Engine.limit_ref(L[:0], R[:0], CEIL, A, H, hist=hist)
    assert np.array_equal(bits(h0[0]), bits(hist[0])) and m0["min_gain"] == 1.0 and m0["reduced"] == 0


# ---------------------------------------------------------------- 8. host-only engines and refusals
def _create(eng, n_rows, ceiling, ahead, hold, cfg_null=False, out_null=False):
    lib = eng._lib
    cfg = E.LimiterConfig(float(ceiling), ahead, hold)
    h = C.c_void_p()
    return lib.tbf_limiter_create(eng._h, n_rows, None if cfg_null else C.byref(cfg), None if out_null else C.byref(h))


def test_host_only_engine_validates_then_refuses():
    eng = T.Engine(sample_rate=48000.0, device=-1)
    assert _create(eng, 4, CEIL, 64, 0) == -19 and "host-only" in _err()
    with pytest.raises(T.TbfError, match="-19"):
        eng.limiter(4, CEIL)
    bad = [
        (dict(n_rows=4, ceiling=0.0, ahead=64, hold=0), "ceiling"),
        (dict(n_rows=4, ceiling=-1.0, ahead=64, hold=0), "ceiling"),
        (dict(n_rows=4, ceiling=np.inf, ahead=64, hold=0), "ceiling"),
        (dict(n_rows=4, ceiling=np.nan, ahead=64, hold=0), "ceiling"),
        (dict(n_rows=4, ceiling=CEIL, ahead=48, hold=0), "ahead"),
        (dict(n_rows=4, ceiling=CEIL, ahead=1, hold=0), "ahead"),
        (dict(n_rows=4, ceiling=CEIL, ahead=0, hold=0), "ahead"),
        (dict(n_rows=4, ceiling=CEIL, ahead=1024, hold=0), "ahead"),
        (dict(n_rows=4, ceiling=CEIL, ahead=64, hold=4097), "hold"),
        (dict(n_rows=0, ceiling=CEIL, ahead=64, hold=0), "n_rows"),
        (dict(n_rows=4, ceiling=CEIL, ahead=64, hold=0, cfg_null=True), "cfg"),
        (dict(n_rows=4, ceiling=CEIL, ahead=64, hold=0, out_null=True), "out"),
    ]
    for kw, word in bad:   # validation comes before the -19
        assert _create(eng, **kw) == -22, kw
        assert word in _err(), (kw, _err())
    lib = eng._lib
    cfg, h = E.LimiterConfig(float(CEIL), 64, 0), C.c_void_p()
    assert lib.tbf_limiter_create(None, 4, C.byref(cfg), C.byref(h)) == -22 and "engine" in _err()
    eng.close()


def test_null_limiter_and_ref_refusals():
    lib = T.load_library()
    d = C.c_uint32()
    assert lib.tbf_limiter_latency(None, C.byref(d)) == -22 and "lim" in _err()
    assert lib.tbf_limiter_reset(None, 0, None, None) == -22 and "lim" in _err()
    lo = E.LimitOut(None, None, 0, None)
    assert lib.tbf_limit_device(None, None, None, 0, 0, None, C.byref(lo), None) == -22 and "lim" in _err()
    assert lib.tbf_limiter_destroy(None) == 0
    x = np.zeros(8, np.float32)
    for kw, word in ((dict(ceiling=0.0), "ceiling"), (dict(ahead=3), "ahead"), (dict(hold=5000), "hold")):
        with pytest.raises(T.TbfError, match=word):
            T.Engine.limit_ref(x, x, **{"ceiling": CEIL, **kw})
    with pytest.raises(T.TbfError, match="ahead"):
        T.Engine.limit_grid(CEIL, 6, 0)
