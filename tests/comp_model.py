"""A plain-Python model of the bus compressor's definition (include/tbf.h, "Bus compressor"), for the
tests: the curve lookup, the recurrence and the output, one frame at a time.  Every float32
subtraction and multiply is numpy's (one IEEE operation); every fmaf is computed exactly in
rationals and rounded once, never as a double product rounded twice."""
from fractions import Fraction

import numpy as np

POINTS, SEG = 769, 32
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def levels():
    """the levels of the 769 points, exact in float64: point i at 2^(-16 + i // 32) (1 + (i % 32) / 32)"""
    i = np.arange(POINTS)
    return np.ldexp(1.0 + (i % SEG) / SEG, i // SEG - 16)


def round32(v):
    """the float32 nearest the rational v, ties to even; an exact zero is +0.0"""
    if v == 0:
        return F32(0.0)
    r = F32(float(v))
    if np.isfinite(r) and Fraction(float(r)) == v:
        return r
    best = None
    for c in (np.nextafter(r, F32(-np.inf)), r, np.nextafter(r, F32(np.inf))):
        if not np.isfinite(c):
            continue
        d = abs(Fraction(float(c)) - v)
        even = (int(F32(c).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, c, even)
    return F32(best[1])


def fmaf(a, b, c):
    """a * b + c of three finite float32, rounded once"""
    return round32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def peak(xl, xr):
    """limit_peak: the larger magnitude, NaN skipped"""
    p = F32(0.0)
    for x in (xl, xr):
        m = F32(abs(F32(x)))
        if m > p:  # False for a NaN
            p = m
    return p


def lookup(pt, p):
    """the curve pt at the level p (float32, >= 0, not NaN)"""
    p = F32(p)
    if p < F32(2.0 ** -16):
        return F32(pt[0])
    if p >= F32(256.0):
        return F32(pt[POINTS - 1])
    u = int(p.view(np.uint32))
    i = (u >> 18) - (111 << 5)
    assert 0 <= i < POINTS - 1
    fr = F32((u & 0x3FFFF) * 2.0 ** -18)  # 18 bits: exact
    lo, hi = F32(pt[i]), F32(pt[i + 1])
    return fmaf(fr, F32(hi - lo), lo)


def step(g, t, a, r):
    d = F32(F32(g) - F32(t))
    return fmaf(F32(a) if d > 0 else F32(r), d, t)


def row(L, R, pt, a, r, m, g=1.0, key=None):
    """one row: (outL, outR, g behind the last frame, gains [n])"""
    L, R = np.asarray(L, F32), np.asarray(R, F32)
    kl, kr = (L, R) if key is None else (np.asarray(key[0], F32), np.asarray(key[1], F32))
    pt = np.asarray(pt, F32)
    g, m = F32(g), F32(m)
    oL, oR, gains = np.zeros(len(L), F32), np.zeros(len(L), F32), np.zeros(len(L), F32)
    with np.errstate(all="ignore"):
        for n in range(len(L)):
            g = step(g, lookup(pt, peak(kl[n], kr[n])), a, r)
            gains[n] = g
            gm = F32(g * m)
            oL[n], oR[n] = F32(gm * L[n]), F32(gm * R[n])
    return oL, oR, g, gains


def noise(seed, n, scale=0.25):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(F32)


def design(T, R, W):
    """the designer's formula in float64 with math-grade functions: the 769 gains before rounding"""
    x = 20.0 * np.log10(levels())
    s = 0.0 if np.isinf(R) else 1.0 / R
    y = np.where(2.0 * (x - T) < -W, x, np.where(2.0 * np.abs(x - T) <= W,
                 x + (s - 1.0) * (x - T + W / 2.0) ** 2 / (2.0 * W) if W > 0 else x, T + (x - T) * s))
    return np.minimum(1.0, 10.0 ** ((y - x) / 20.0))


def same(a, b):
    """equal in bits, a NaN equal to any NaN"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))
