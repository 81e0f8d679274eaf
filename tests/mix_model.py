"""The mixdown stage's definition (include/tbf.h) in numpy float64: the value of every bus
sample, the magnitude of its terms and the number of rows that reach it, from which the bound of
a sequential fma sum follows.  Products of two float32 are exact in float64, so the only error of
the float64 value is its own summation, 2^-29 times smaller than float32's.  The tests compare the
engine's host restatement against these; the kernel is compared with the restatement in bits."""
import numpy as np

NONE = 0xFFFFFFFF
U = 2.0 ** -24  # float32 unit roundoff
ROW_DTYPE = np.dtype([("bus", "<u4"), ("ll", "<f4"), ("lr", "<f4"), ("rl", "<f4"), ("rr", "<f4")])


def rows_of(bus, ll, lr, rl, rr):
    """ROW_DTYPE records from five sequences"""
    r = np.zeros(len(bus), ROW_DTYPE)
    r["bus"] = np.asarray(bus, np.int64) & 0xFFFFFFFF
    for k, v in (("ll", ll), ("lr", lr), ("rl", rl), ("rr", rr)):
        r[k] = np.asarray(v, np.float32)
    return r


def mix64(L, R, rows, n_buses, counts=None):
    """(L64, R64, magL, magR, members): float64 [n_buses, frames] each: the sums of the definition
    over the rows in ascending order, mag = sum |c x| of their terms, members = the rows that
    reach each bus sample (j < count[r])"""
    L, R = np.asarray(L, np.float32).astype(np.float64), np.asarray(R, np.float32).astype(np.float64)
    n, frames = L.shape
    cnt = np.full(n, frames) if counts is None else np.asarray(counts, np.int64)
    out = [np.zeros((n_buses, frames)) for _ in range(5)]
    for r in range(n):
        b = int(rows["bus"][r])
        if b == NONE:
            continue
        c = int(cnt[r])
        l, x = L[r, :c], R[r, :c]
        ll, lr, rl, rr = (float(rows[k][r]) for k in ("ll", "lr", "rl", "rr"))
        out[0][b, :c] += ll * l
        out[0][b, :c] += lr * x
        out[1][b, :c] += rl * l
        out[1][b, :c] += rr * x
        out[2][b, :c] += np.abs(ll * l) + np.abs(lr * x)
        out[3][b, :c] += np.abs(rl * l) + np.abs(rr * x)
        out[4][b, :c] += 1
    return tuple(out)


def gamma(m):
    """gamma_m = m u / (1 - m u): the relative bound of a sequential sum of m terms by fma, each
    step one rounding (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1)"""
    m = np.asarray(m, np.float64)
    return m * U / (1.0 - m * U)
