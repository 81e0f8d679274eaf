"""The output rate converter's definition (include/tbf.h) in numpy float64: the prototype
design, the count law, a float64 evaluation of one row with given taps, and the frequency
response of a table.  The tests compare the engine's hooks and kernel against these."""
from math import gcd

import numpy as np

ZC = 32
BETA = 10.0
EPS = 2.0 ** -24

# the rate pairs of the GPU tests and what each exercises (Fi, Fo, L, M, T)
PAIRS = [(48000, 16000, 1, 3, 192),     # uniform phase; history longer than a block
         (48000, 8000, 1, 6, 384),      # history spans three one-block calls; even stride
         (48000, 22050, 147, 320, 140),  # per-lane phases; counts vary by call and by instance
         (44100, 48000, 160, 147, 64)]   # more outputs than inputs


def ratio(fi, fo):
    """L, M, T of the definition"""
    g = gcd(fi, fo)
    L, M = fo // g, fi // g
    s = max(L, M)
    T = -(-2 * ZC * s // L)
    T += T & 1
    return L, M, T


def design(fi, fo):
    """g64[k], k = 0 .. L T - 1, in double"""
    L, M, T = ratio(fi, fo)
    N = L * T
    fc = 0.45 / max(L, M)
    k = np.arange(N, dtype=np.float64)
    return L * 2.0 * fc * np.sinc(2.0 * fc * (k - (N - 1) / 2.0)) * np.kaiser(N, BETA)


def count(P, L, M):
    """C (P) = ceil (P L / M), in Python integers"""
    return -(-P * L // M)


def ref64(g, L, M, T, x, hist=None, pos0=0):
    """the definition's sum in float64 with the taps g (k order, any dtype): x the samples
    pos0 .., hist the T - 1 before them (None: zeros).  Returns (y64, mag) for the outputs
    [C (pos0), C (pos0 + len (x))): mag[n] = sum_t |g_t x_t|, the scale of the fma bound."""
    g = np.asarray(g, np.float64).reshape(T, L)  # g[t, phi] = g[phi + t L]
    buf = np.zeros(T - 1 + len(x), np.float64)
    if hist is not None:
        buf[:T - 1] = hist
    buf[T - 1:] = x
    n0, n1 = count(pos0, L, M), count(pos0 + len(x), L, M)
    y, mag = np.zeros(n1 - n0), np.zeros(n1 - n0)
    for n in range(n0, n1):
        i, phi = divmod(n * M, L)
        top = T - 1 + (i - pos0)
        xs = buf[top - T + 1:top + 1][::-1]  # x[i], x[i - 1], ...
        pr = g[:, phi] * xs
        y[n - n0] = pr.sum()
        mag[n - n0] = np.abs(pr).sum()
    return y, mag


def response_db(g, L, over=8):
    """(f, dB): |H| of the prototype g, computed in float64, on a grid `over` times finer than its
    length resolves (zero-padded FFT), f in cycles per sample of the L-times upsampled rate
    (0 .. 0.5), normalised so that the passband gain L reads 0 dB"""
    g = np.asarray(g, np.float64)
    nfft = 1 << int(np.ceil(np.log2(over * len(g))))
    h = np.abs(np.fft.rfft(g, nfft)) / L
    return np.arange(len(h)) / nfft, 20.0 * np.log10(np.maximum(h, 1e-300))
