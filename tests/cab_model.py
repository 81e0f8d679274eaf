"""A numpy restatement of the cabinet convolver's scheme (tunebfree_amd/csrc/tbf_cabinet.hip),
not a test: uniformly partitioned overlap-save at the block size in float32 / complex64.

    partition P = 128, X_b = FFT-256 of blocks (b - 1, b), H_k = FFT-256 of taps
    [128 k, 128 k + 128) zero-padded (built in double, rounded to float, like the engine's table),
    Y_b = sum over k = 0 .. K - 1 of X_{b-k} H_k in ascending k (all K terms, zero spectra
    before the first block), block b of wet = the last 128 points of IFFT-256 (Y_b).

np.fft keeps single precision for complex64 input in the numpy this suite runs with; the kernel's
own FFT is a radix-2 with another butterfly order, so the two agree to rounding, not in bits.
The model carries its state (the spectra ring and the last block) between calls like the engine,
so it can be cut into calls.  direct64 / err: the float64 direct sum the convolver is measured
against, and the error norm of the accuracy tests."""
import numpy as np

P = 128
EPS = 2.0 ** -24


def decaying_noise(taps, seed, tau=None):
    """a seeded decaying-noise response of `taps` taps (float32)"""
    g = np.random.default_rng(seed)
    tau = tau or max(taps / 4.0, 1.0)
    return (g.standard_normal(taps) * np.exp(-np.arange(taps) / tau)).astype(np.float32)


def direct64(x, h):
    """x * h in float64, cut to len (x)"""
    return np.convolve(np.asarray(x, np.float64), np.asarray(h, np.float64))[:len(x)]


def err(y, x, h):
    """max |y - direct64| / (max |x| sum |h|)"""
    x = np.asarray(x, np.float64)
    scale = np.abs(x).max() * np.abs(np.asarray(h, np.float64)).sum()
    d = np.abs(np.asarray(y, np.float64) - direct64(x, h)).max()
    return 0.0 if d == 0.0 else d / scale


class Model:
    """one channel of one instance"""

    def __init__(self, h):
        h = np.asarray(h, np.float32)
        assert h.ndim == 1 and 1 <= len(h) <= 8192
        self.K = (len(h) + P - 1) // P
        pad = np.zeros(self.K * P, np.float64)
        pad[:len(h)] = h
        self.H = np.fft.rfft(pad.reshape(self.K, P), 2 * P, axis=1).astype(np.complex64)
        assert self.H.dtype == np.complex64
        self.X = np.zeros((self.K, P + 1), np.complex64)  # X[k] = X_{b-k} once block b is in
        self.tail = np.zeros(P, np.float32)

    def run(self, x):
        """the next len (x) / 128 blocks of wet"""
        x = np.asarray(x, np.float32)
        assert x.ndim == 1 and len(x) % P == 0
        out = np.empty_like(x)
        for b in range(len(x) // P):
            cur = x[b * P:(b + 1) * P]
            spec = np.fft.rfft(np.concatenate([self.tail, cur]).astype(np.float32))
            self.X = np.roll(self.X, 1, axis=0)
            self.X[0] = spec.astype(np.complex64)
            acc = np.zeros(P + 1, np.complex64)
            for k in range(self.K):
                acc = (acc + self.X[k] * self.H[k]).astype(np.complex64)
            y = np.fft.irfft(acc, 2 * P)
            assert acc.dtype == np.complex64
            out[b * P:(b + 1) * P] = y[P:].astype(np.float32)
            self.tail = cur.copy()
        return out


def convolve(x, h, cuts=None):
    """wet of x through h with the model, as one call or cut into calls of cuts[i] blocks"""
    m = Model(h)
    x = np.asarray(x, np.float32)
    cuts = cuts or [len(x) // P]
    assert sum(cuts) * P == len(x)
    parts, at = [], 0
    for c in cuts:
        parts.append(m.run(x[at * P:(at + c) * P]))
        at += c
    return np.concatenate(parts)
