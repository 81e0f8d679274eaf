"""The bus limiter with a true-peak detector (include/tbf.h, "Bus limiter, addition") in numpy
float32, for a new row: the detector's interpolated values from truepeak_model.chain (exactly
rounded fmaf in rational arithmetic, which shares no code with the library), the gain law as
limit_model states it (window minimum by doubling, the ascending sum of A adds).  It is exact, so
the tests compare bits.  The chains are slow and depend on the input alone, so they are kept per
input and shared by every configuration that runs on it."""
import numpy as np

import limit_model as LM
import truepeak_model as TP

E = 6                       # the frames by which the samples trail the interpolated values they are paired with
REACH = TP.TAPS - 1         # t[n] reads x[n - 11]
CEILING = LM.CEILING


def history(ahead, hold):
    """Hn_tp: the frames of input a row keeps per channel"""
    return 2 * ahead + hold + 9


def latency(ahead):
    return ahead + 5


_chains = {}


def chains(x, F, nan_at=None):
    """y[n][p] of a new row x for the phases F uses, [n, phases] float32.  nan_at: a frame of x that
    holds a NaN: the chains are those of x with a zero there, and the twelve values per phase whose
    window holds the frame are NaN, as an fmaf chain through a NaN is."""
    x = np.ascontiguousarray(x, np.float32)
    if nan_at is not None:
        x = x.copy()
        x[nan_at] = 0.0
    out = np.empty((len(x), len(TP.phases(F))), np.float32)
    for k, p in enumerate(TP.phases(F)):
        key = (x.tobytes(), p)
        if key not in _chains:
            _chains[key] = TP.chain(x, p)
        out[:, k] = _chains[key]
    if nan_at is not None:
        out[nan_at:nan_at + TP.TAPS] = np.nan
    return out


def limit_tp(L, R, ceiling, ahead, hold, F, nan_at=(None, None)):
    """One new row: L, R [n] float32 (finite but for one NaN per channel at nan_at).  Returns
    (yL, yR, g, meter, p)."""
    c = np.float32(ceiling)
    A, W, DE = ahead, ahead + hold, ahead - 1 + E
    L, R = np.asarray(L, np.float32), np.asarray(R, np.float32)
    n = len(L)
    one, zero = np.float32(1.0), np.float32(0.0)
    with np.errstate(all="ignore"):
        cand = [np.abs(LM._shift(L, E, zero)), np.abs(LM._shift(R, E, zero))]
        for x, at in ((L, nan_at[0]), (R, nan_at[1])):
            y = chains(x, F, at)
            cand += [np.abs(y[:, k]) for k in range(y.shape[1])]
        p = np.zeros(n, np.float32)
        for v in cand:
            p = np.where(v > p, v, p)            # a NaN compares false and is skipped
        over = p > c
        t = np.where(over, c / np.where(over, p, one), one).astype(np.float32)
        m, w = t.copy(), 1
        while 2 * w <= W:
            m = np.minimum(m, LM._shift(m, w, one))
            w *= 2
        m = np.minimum(m, LM._shift(m, W - w, one))
        acc = np.zeros(n, np.float32)
        for k in range(A - 1, -1, -1):           # ascending in the frame: the oldest term first
            acc = (acc + LM._shift(m, k, one)).astype(np.float32)
        g = (acc * np.float32(1.0 / A)).astype(np.float32)
        dl, dr = LM._shift(L, DE, zero), LM._shift(R, DE, zero)
        yl, yr = (g * dl).astype(np.float32), (g * dr).astype(np.float32)
        clamped = int((yl > c).sum() + (yl < -c).sum() + (yr > c).sum() + (yr < -c).sum())
        yl = np.where(yl > c, c, np.where(yl < -c, -c, yl)).astype(np.float32)
        yr = np.where(yr > c, c, np.where(yr < -c, -c, yr)).astype(np.float32)
    meter = np.zeros(1, LM.METER_DTYPE)[0]
    meter["min_gain"] = g.min() if n else 1.0
    meter["reduced"] = int((g < one).sum())
    meter["clamped"] = clamped
    return yl, yr, g, meter, p
