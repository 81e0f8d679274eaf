"""The bus equaliser in plain Python: the cascade with scalar Python floats in the operation order
of include/tbf.h ("Bus equaliser"), and the RBJ designer with `math` in the order of eqCompute
(csrc/tbf_eq.h).  The tests compare the library's host restatement with `cascade` in bits, and its
coefficients with `coeffs` to a bound that allows libm's last place."""
import math

import numpy as np

LPF, HPF, BPF0, BPF1, NOTCH, APF, PEQ, LOW, HIGH = range(9)
TYPES = (LPF, HPF, BPF0, BPF1, NOTCH, APF, PEQ, LOW, HIGH)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def noise(seed, n, rows=None, scale=0.25):
    """seeded float32 noise, [n] or [rows, n]"""
    shape = (n,) if rows is None else (rows, n)
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def coeffs(kind, hz, q, gain_db, rate):
    """b0, b1, b2, a1, a2 of a band: every expression as eqCompute writes it"""
    A = math.pow(10.0, (gain_db / 40.0))
    omega = (2.0 * math.pi * hz) / float(rate)
    sin_, cos_ = math.sin(omega), math.cos(omega)
    alpha = sin_ / (2.0 * q)
    beta = math.sqrt(A) / q
    plain = (1.0 + alpha, -2.0 * cos_, 1.0 - alpha)
    if kind == LPF:
        b, a = ((1.0 - cos_) / 2.0, 1.0 - cos_, (1.0 - cos_) / 2.0), plain
    elif kind == HPF:
        b, a = ((1.0 + cos_) / 2.0, -(1.0 + cos_), (1.0 + cos_) / 2.0), plain
    elif kind == BPF0:
        b, a = (sin_ / 2.0, 0.0, -sin_ / 2.0), plain
    elif kind == BPF1:
        b, a = (alpha, 0.0, -alpha), plain
    elif kind == NOTCH:
        b, a = (1.0, -2.0 * cos_, 1.0), plain
    elif kind == APF:
        b, a = (1.0 - alpha, -2.0 * cos_, 1.0 + alpha), plain
    elif kind == PEQ:
        b = (1.0 + (alpha * A), -2.0 * cos_, 1.0 - (alpha * A))
        a = (1.0 + (alpha / A), -2.0 * cos_, 1.0 - (alpha / A))
    elif kind == LOW:
        b = (A * ((A + 1) - ((A - 1) * cos_) + (beta * sin_)), (2.0 * A) * ((A - 1) - ((A + 1) * cos_)),
             A * ((A + 1) - ((A - 1) * cos_) - (beta * sin_)))
        a = ((A + 1) + ((A - 1) * cos_) + (beta * sin_), -2.0 * ((A - 1) + ((A + 1) * cos_)),
             (A + 1) + ((A - 1) * cos_) - (beta * sin_))
    elif kind == HIGH:
        b = (A * ((A + 1) + ((A - 1) * cos_) + (beta * sin_)), -(2.0 * A) * ((A - 1) + ((A + 1) * cos_)),
             A * ((A + 1) + ((A - 1) * cos_) - (beta * sin_)))
        a = ((A + 1) - ((A - 1) * cos_) + (beta * sin_), 2.0 * ((A - 1) - ((A + 1) * cos_)),
             (A + 1) - ((A - 1) * cos_) - (beta * sin_))
    else:
        raise ValueError(kind)
    return np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]], np.float64)


def cascade(x, c, state=None):
    """one channel: the frames x (float32) through the bands c [nb, 5] behind state [nb, 2];
    returns (the output as float32, the state)"""
    c = [[float(v) for v in band] for band in np.asarray(c, np.float64).reshape(-1, 5)]
    st = [[0.0, 0.0] for _ in c] if state is None else [[float(v) for v in s] for s in np.asarray(state).reshape(-1, 2)]
    out = np.empty(len(x), np.float32)
    with np.errstate(all="ignore"):
        for i, sample in enumerate(np.asarray(x, np.float32)):
            v = float(sample)
            for (b0, b1, b2, a1, a2), s in zip(c, st):
                y = b0 * v + s[0]
                s[0] = (b1 * v + s[1]) - a1 * y
                s[1] = b2 * v - a2 * y
                v = y
            out[i] = np.float64(v).astype(np.float32)
    return out, np.array(st, np.float64).reshape(len(c), 2)


def row(L, R, c, state=None):
    """both channels of a row: (outL, outR, state [2, nb, 2])"""
    nb = len(np.asarray(c, np.float64).reshape(-1, 5))
    st = np.zeros((2, nb, 2)) if state is None else np.asarray(state, np.float64)
    oL, sL = cascade(L, c, st[0])
    oR, sR = cascade(R, c, st[1])
    return oL, oR, np.stack([sL, sR])


def gain_db(c, hz, rate):
    """20 log10 |H(e^{jw})| of one band's five doubles at hz, in float64"""
    b0, b1, b2, a1, a2 = (float(v) for v in c)
    w = 2.0 * math.pi * hz / float(rate)
    z1, z2 = complex(math.cos(w), -math.sin(w)), complex(math.cos(2.0 * w), -math.sin(2.0 * w))
    h = abs(b0 + b1 * z1 + b2 * z2) / abs(1.0 + a1 * z1 + a2 * z2)
    return 20.0 * math.log10(h) if h > 0.0 else -math.inf
