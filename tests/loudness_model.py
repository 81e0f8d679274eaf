"""A model of the loudness meter (include/tbf.h, "Loudness meter") that shares no code with the
library: the coefficient formulas with Python's libm, the recurrence as plain Python floats (IEEE
doubles, one rounding per operator, no contraction), and the gating in numpy.  The tests compare
tbf_debug_loudness_ref with `recurrence` in bits and tbf_debug_loudness_result with `gating` to a
tolerance (both go through a log10)."""
import math

import numpy as np

RESULT_DTYPE = np.dtype([("integrated", "<f8"), ("momentary_max", "<f8"), ("short_term_max", "<f8"),
                         ("hops", "<u4"), ("blocks", "<u4"), ("gated", "<u4"), ("reserved", "<u4")])

# ITU-R BS.1770-4, table of the 48 kHz filters
TABLE_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             -1.99004745483398, 0.99007225036621)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ulps(a, b):
    """the distance of two arrays of finite doubles of equal sign, in units of the last place"""
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


def coeffs(rate):
    """b0, b1, b2, a1, a2 of the shelf and c1, c2 of the high-pass, as the header spells them"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / rate)
    Vh = math.pow(10.0, G / 20.0)
    Vb = math.pow(Vh, 0.4996667741545416)
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    return np.array(shelf + [2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], np.float64)


def recurrence(x, c, Hp, state=None, variant=None):
    """one channel: the frames x (float32) behind state [s1, s2, t1, t2, acc, k]; returns (the
    energies of the hops completed, the state).  variant "s1": s1 = (b1*x - a1*y) + s2, another
    association of the same terms; "half": the hop's sum taken as two half-hop sums that are then
    added (only for a channel that starts at k == 0)."""
    b0, b1, b2, a1, a2, c1, c2 = (float(v) for v in c)
    s1, s2, t1, t2, acc, k = (0.0,) * 6 if state is None else (float(v) for v in state)
    k = int(k)
    out, first = [], 0.0
    for v in np.asarray(x, np.float32).tolist():   # float32 -> Python float is exact
        y = b0 * v + s1
        if variant == "s1":
            s1 = (b1 * v - a1 * y) + s2
        else:
            s1 = (b1 * v + s2) - a1 * y
        s2 = b2 * v - a2 * y
        w = y + t1
        t1 = (-2.0 * y + t2) - c1 * w
        t2 = y - c2 * w
        acc = acc + w * w
        k += 1
        if variant == "half" and k == Hp // 2:
            first, acc = acc, 0.0
        if k == Hp:
            out.append(first + acc if variant == "half" else acc)
            acc, k, first = 0.0, 0, 0.0
    return np.array(out, np.float64), np.array([s1, s2, t1, t2, acc, float(k)], np.float64)


def row(L, R, rate, state=None, variant=None):
    """both channels of a row: (energies [hops, 2], state [12])"""
    c, Hp = _coeffs_of_library(rate), rate // 10
    st = np.zeros(12) if state is None else np.asarray(state, np.float64)
    eL, sL = recurrence(L, c, Hp, st[:6], variant)
    eR, sR = recurrence(R, c, Hp, st[6:], variant)
    return np.stack([eL, eR], axis=1).reshape(-1, 2), np.concatenate([sL, sR])


def _coeffs_of_library(rate):
    """the recurrence is compared in bits, so libm must not enter: the library's coefficients"""
    import tunebfree_amd as T
    return T.Engine.loudness_coeffs(rate)


def gating(rate, e):
    """the results of [hops, 2] energies as one RESULT_DTYPE record"""
    e = np.asarray(e, np.float64).reshape(-1, 2)
    Hp, n = rate // 10, len(e)
    out = np.zeros(1, RESULT_DTYPE)[0]
    out["integrated"] = out["momentary_max"] = out["short_term_max"] = -np.inf
    out["hops"] = n
    if n < 4:
        return out
    u = e[:, 0] + e[:, 1]
    z = (((u[:-3] + u[1:-2]) + u[2:-1]) + u[3:]) / (4.0 * Hp)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
    out["blocks"] = len(z)
    fin = l[~np.isnan(l)]
    out["momentary_max"] = fin.max() if len(fin) else -np.inf
    a = l > -70.0
    if a.any():
        gate = -0.691 + 10.0 * math.log10(math.fsum(z[a]) / a.sum()) - 10.0
        g = a & (l > gate)
        out["gated"] = g.sum()
        if g.any():
            out["integrated"] = -0.691 + 10.0 * math.log10(math.fsum(z[g]) / g.sum())
    if n >= 30:
        s = np.array([math.fsum(u[j:j + 30]) for j in range(n - 29)]) / (30.0 * Hp)
        with np.errstate(divide="ignore", invalid="ignore"):
            ls = -0.691 + 10.0 * np.log10(s)
        ls = ls[~np.isnan(ls)]
        out["short_term_max"] = ls.max() if len(ls) else -np.inf
    return out


def sine(rate, segments, freq=1000.0):
    """a sine of `freq` Hz as float32: segments [(dBFS peak, seconds), ...] one after the other,
    the phase running on"""
    n = [int(round(sec * rate)) for _db, sec in segments]
    t = np.arange(sum(n), dtype=np.float64)
    amp = np.concatenate([np.full(k, 10.0 ** (db / 20.0)) for (db, _s), k in zip(segments, n)])
    return (amp * np.sin(2.0 * np.pi * freq * t / rate)).astype(np.float32)


def noise(seed, n, rows=None, scale=0.25):
    """seeded float32 noise, [n] or [rows, n]"""
    shape = (n,) if rows is None else (rows, n)
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)
