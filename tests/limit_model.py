"""The bus limiter's definition (include/tbf.h) in numpy float32.

numpy's float32 add, multiply and divide are IEEE operations, so this model is exact: the tests
compare bits with it, not within a tolerance.  It is written for clarity, not speed: the window
minimum by doubling (min is exact in any order), the gain's sum as A vector adds in the order the
definition sets (ascending; descending on request, to show that the order is observable).
"""
import numpy as np

METER_DTYPE = np.dtype([("min_gain", "<f4"), ("reduced", "<u4"), ("clamped", "<u4")])
MAX_AHEAD, MAX_HOLD = 512, 4096
CEILING = np.float32(1.0 - 2.0 ** -15)


def history(ahead, hold):
    """Hn: the frames of input a row keeps per channel"""
    return 2 * ahead + hold - 2


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def issue_input(seed, frames, rows=None):
    """the inputs the issue sets for the identity tests: randn * 10^uniform (-2, 0.7) as float32"""
    rng = np.random.default_rng(seed)
    shape = (frames,) if rows is None else (rows, frames)
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-2, 0.7, shape)).astype(np.float32)


def _shift(a, k, fill):
    """a[n - k], `fill` before the start"""
    if k == 0:
        return a.copy()
    out = np.full_like(a, fill)
    out[k:] = a[:-k] if k < len(a) else a[:0]
    return out


def limit(L, R, ceiling, ahead, hold, hist=None, descending=False):
    """One row: L, R [n] float32 behind hist = (histL, histR) of Hn floats each (None: a new row).
    Returns (yL, yR, g, meter, (histL, histR))."""
    c = np.float32(ceiling)
    A, W, D, Hn = ahead, ahead + hold, ahead - 1, history(ahead, hold)
    L, R = np.asarray(L, np.float32), np.asarray(R, np.float32)
    n = len(L)
    hL, hR = (np.zeros(Hn, np.float32), np.zeros(Hn, np.float32)) if hist is None else hist
    xl, xr = np.concatenate([hL, L]).astype(np.float32), np.concatenate([hR, R]).astype(np.float32)
    with np.errstate(all="ignore"):
        p = np.zeros(len(xl), np.float32)
        al, ar = np.abs(xl), np.abs(xr)
        p = np.where(al > p, al, p)          # a NaN compares false and is skipped
        p = np.where(ar > p, ar, p)
        over = p > c
        t = np.where(over, c / np.where(over, p, np.float32(1.0)), np.float32(1.0)).astype(np.float32)
        # m[i] = min t[i - W + 1 .. i]; what lies before the array is taken as 1 and never used
        m, w = t.copy(), 1
        while 2 * w <= W:
            m = np.minimum(m, _shift(m, w, np.float32(1.0)))
            w *= 2
        m = np.minimum(m, _shift(m, W - w, np.float32(1.0)))
        acc = np.zeros(len(xl), np.float32)
        order = range(A - 1, -1, -1) if not descending else range(A)   # the shift of term j = n - k
        for k in order:
            acc = (acc + _shift(m, k, np.float32(1.0))).astype(np.float32)
        g = (acc * np.float32(1.0 / A)).astype(np.float32)[Hn:]
        dl, dr = xl[Hn - D:Hn - D + n], xr[Hn - D:Hn - D + n]
        yl, yr = (g * dl).astype(np.float32), (g * dr).astype(np.float32)
        clamped = int((yl > c).sum() + (yl < -c).sum() + (yr > c).sum() + (yr < -c).sum())
        yl = np.where(yl > c, c, np.where(yl < -c, -c, yl)).astype(np.float32)
        yr = np.where(yr > c, c, np.where(yr < -c, -c, yr)).astype(np.float32)
    meter = np.zeros(1, METER_DTYPE)[0]
    meter["min_gain"] = g.min() if n else 1.0
    meter["reduced"] = int((g < np.float32(1.0)).sum())
    meter["clamped"] = clamped
    return yl, yr, g, meter, (xl[n:].copy(), xr[n:].copy())
