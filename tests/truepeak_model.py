"""A model of the true-peak meter and of the loudness range (include/tbf.h, "True-peak meter" and
"Loudness range") that shares no code with the library: the table from its 48 integers, the chains
as exactly rounded float32 fmaf in rational arithmetic (slow: a few hundred frames), the same values
in float64 for longer rows, the aimed bursts, and the range in numpy."""
from fractions import Fraction

import numpy as np

K0 = (14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68)
K1 = (-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155)
K = np.array([K0, K1, K1[::-1], K0[::-1]], np.int64)
H = K.astype(np.float64) / 8192.0          # exact: 13-bit integers over 2^13
TAPS, HIST = 12, 11
RESULT_DTYPE = np.dtype([("sample_peak", "<f4", (2,)), ("inter_peak", "<f4", (2,)), ("frames", "<u8"), ("dbtp", "<f8")])


def phases(F):
    """the phases an oversampling factor uses"""
    return {4: (0, 1, 2, 3), 2: (0, 2), 1: ()}[F]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def mag(a):
    """the bit patterns of the magnitudes"""
    return bits(a) & np.uint32(0x7FFFFFFF)


def word(v):
    """the bit pattern of one float32's magnitude"""
    return int(np.float32(v).view(np.uint32)) & 0x7FFFFFFF


def is_nan_word(w):
    return int(w) > 0x7F800000


def windows(x, hist=None):
    """[n, 12] float64 with [n, j] = x[n - j], the frames before x from hist (None: zeros)"""
    h = np.zeros(HIST) if hist is None else np.asarray(hist, np.float64)
    ext = np.concatenate([h, np.asarray(x, np.float64)])
    return np.lib.stride_tricks.sliding_window_view(ext, TAPS)[:, ::-1]


def y64(x, F=4, hist=None):
    """every y[n][p] in float64, [n, phases]: 24-bit inputs times 13-bit coefficients, so each product
    is exact and the sum carries double's rounding only"""
    return windows(x, hist) @ H[list(phases(F))].T


def round32(v):
    """the float32 nearest the rational v, ties to even"""
    r = np.float32(float(v))
    if Fraction(float(r)) == v:
        return r
    best = None
    for c in (np.nextafter(r, np.float32(-np.inf)), r, np.nextafter(r, np.float32(np.inf))):
        d = abs(Fraction(float(c)) - v)
        even = (int(np.float32(c).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, c, even)
    return np.float32(best[1])


def chain(x, p, hist=None, descending=False):
    """y[n][p] of finite x as float32 [n]: one exactly rounded fmaf per tap, in tap order (or in the
    opposite order)"""
    w = windows(x, hist)
    order = range(TAPS - 1, -1, -1) if descending else range(TAPS)
    out = np.zeros(len(w), np.float32)
    for n in range(len(w)):
        acc = Fraction(0)
        for j in order:
            acc = Fraction(float(round32(Fraction(int(K[p][j]), 8192) * Fraction(float(w[n, j])) + acc)))
        out[n] = np.float32(float(acc))
    return out


def noise(seed, n, rows=None, scale=1.0):
    """seeded float32 noise, uniform in [-scale, scale], [n] or [rows, n]"""
    shape = (n,) if rows is None else (rows, n)
    return (np.random.default_rng(seed).uniform(-1.0, 1.0, shape) * scale).astype(np.float32)


def aimed(seed, n, n0, p):
    """noise of amplitude 0.01 with the burst matched to phase p at frame n0 in its place:
    x[n0 - j] = h[p][j] / max |h[p]|, which puts the one maximum of the y stream at (n0, p) and that
    above the burst's sample peak of 1.0; n0 >= 11"""
    x = noise(seed, n, scale=0.01)
    x[n0 - np.arange(TAPS)] = (H[p] / np.abs(H[p]).max()).astype(np.float32)
    return x


def argmax_y(y):
    """(frame, phase index, the largest |y| over the runner-up) of a [n, phases] stream"""
    a = np.abs(np.asarray(y, np.float64))
    n0, p = np.unravel_index(np.argmax(a), a.shape)
    top = a[n0, p]
    a = a.copy()
    a[n0, p] = 0.0
    return int(n0), int(p), float(top / a.max())


def dbtp(words):
    m = int(max(int(w) for w in words))
    if m == 0:
        return -np.inf
    v = np.uint32(m).view(np.float32)
    return np.nan if np.isnan(v) else 20.0 * np.log10(np.float64(v))


def sine(n, cycles_per_frame, phase_deg=0.0, amp=1.0):
    t = np.arange(n, dtype=np.float64)
    return (amp * np.sin(2.0 * np.pi * cycles_per_frame * t + np.deg2rad(phase_deg))).astype(np.float32)


def loudness_range(rate, e):
    """(LRA, windows) of [hops, 2] energies, EBU Tech 3342"""
    e = np.asarray(e, np.float64).reshape(-1, 2)
    Hp, n = rate // 10, len(e)
    if n < 30:
        return 0.0, 0
    u = e[:, 0] + e[:, 1]
    z = np.array([np.sum(u[j:j + 30]) for j in range(n - 29)]) / (30.0 * Hp)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
    a = l > -70.0
    if not a.any():
        return 0.0, 0
    gate = -0.691 + 10.0 * np.log10(np.sum(z[a]) / a.sum()) - 20.0
    s = np.sort(l[a & (l > gate)])
    if not len(s):
        return 0.0, 0
    m = len(s) - 1
    return float(s[int(np.floor(m * 0.95 + 0.5))] - s[int(np.floor(m * 0.10 + 0.5))]), len(s)
