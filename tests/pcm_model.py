"""The PCM output stage's definition (include/tbf.h) in numpy: float32
arithmetic with np.rint, the counter hash of the dither in wrapping 32-bit integers, the frame
packing as bytes and the meters.  Written from the definition's text, not from the C header the
kernel is built from; the tests compare the two in bytes.

    per float32 sample x, S = 32768 (S16) or 8388608 (S24):
        v = x * S;  t = v, or v + d with dither;  q = rint (t), ties to even
        NaN -> 0, q > max -> max, q < min -> min, each a clip
    F32 copies the bits and counts !(|x| <= 1).
    d of row r, channel c, frame f:  k = h (h (h (seed ^ (2 r + c)) ^ lo32 (f)) ^ hi32 (f)),
        d = (float (k & 0xffff) - float (k >> 16)) * 2^-16
    peak = max |x| without NaN, clip = the count."""
import numpy as np

S16, S24, F32 = 0, 1, 2
DITHER = 1
FRAME_BYTES = (4, 6, 8)
SCALE = {S16: 32768.0, S24: 8388608.0}
FORMATS = [(S16, 0), (S16, DITHER), (S24, 0), (F32, 0)]

_M32 = np.uint64(0xFFFFFFFF)


def h(a):
    """the 32-bit mixer, on uint64 arrays holding 32-bit values"""
    a = np.asarray(a, np.uint64) & _M32
    a = a ^ (a >> np.uint64(16))
    a = (a * np.uint64(0x7FEB352D)) & _M32
    a = a ^ (a >> np.uint64(15))
    a = (a * np.uint64(0x846CA68B)) & _M32
    return a ^ (a >> np.uint64(16))


def dither(seed, row, c, f):
    """d for the frames f (uint64 array) of row `row`, channel c: float32, in LSBs"""
    f = np.asarray(f, np.uint64)
    k = h(h(h(np.uint64((seed ^ (2 * row + c)) & 0xFFFFFFFF)) ^ (f & _M32)) ^ (f >> np.uint64(32)))
    lo = (k & np.uint64(0xFFFF)).astype(np.float32)
    hi = (k >> np.uint64(16)).astype(np.float32)
    return (lo - hi) * np.float32(2.0 ** -16)


def quantise(x, fmt, d=None):
    """one channel: (int32 values, clip count)"""
    x = np.asarray(x, np.float32)
    S = np.float32(SCALE[fmt])
    with np.errstate(all="ignore"):
        t = x * S
        if d is not None:
            t = t + np.asarray(d, np.float32)
        q = np.rint(t)
    assert t.dtype == np.float32 and q.dtype == np.float32
    top, bot = float(S) - 1.0, -float(S)
    nan = np.isnan(q)
    with np.errstate(invalid="ignore"):
        over, under = q > top, q < bot
    v = np.where(nan, 0.0, np.where(over, top, np.where(under, bot, q)))
    return v.astype(np.int64).astype(np.int32), int(nan.sum() + over.sum() + under.sum())


def peak(x):
    a = np.abs(np.asarray(x, np.float32))
    a = a[~np.isnan(a)]
    return np.float32(a.max()) if len(a) else np.float32(0.0)


def convert(fmt, L, R, flags=0, seed=0, row=0, frame0=0):
    """one row: (the packed frames as uint8 [n * frame bytes], (peakL, peakR, clipL, clipR))"""
    L, R = np.asarray(L, np.float32), np.asarray(R, np.float32)
    n = len(L)
    assert len(R) == n and (not flags or (flags == DITHER and fmt == S16))
    if fmt == F32:
        out = np.empty((n, 2), np.uint32)
        out[:, 0], out[:, 1] = L.view(np.uint32), R.view(np.uint32)
        with np.errstate(invalid="ignore"):
            clips = [int((~(np.abs(x) <= np.float32(1.0))).sum()) for x in (L, R)]
        return out.view(np.uint8).reshape(-1).copy(), (peak(L), peak(R), clips[0], clips[1])
    f = np.uint64(frame0) + np.arange(n, dtype=np.uint64)
    q, clips = [], []
    for c, x in enumerate((L, R)):
        v, k = quantise(x, fmt, dither(seed, row, c, f) if flags & DITHER else None)
        q.append(v)
        clips.append(k)
    nb = 2 if fmt == S16 else 3
    u = np.stack(q, axis=1).astype(np.int64) & ((1 << (8 * nb)) - 1)  # [n, 2] two's complement
    out = np.empty((n, 2, nb), np.uint8)
    for b in range(nb):
        out[:, :, b] = (u >> (8 * b)) & 0xFF
    return out.reshape(-1), (peak(L), peak(R), clips[0], clips[1])


def crafted(seed=5):
    """a row pair with the quantiser's edge cases for both scales and 1000 normals at 0.3: full
    scale and the largest code, the ties, a sample the reference chain reaches (1.22),
    infinities, NaNs with payloads, -0 and subnormals.  R is L in another order, so the channels'
    meters differ."""
    v = []
    for S in (32768.0, 8388608.0):
        v += [1.0, -1.0, 1.0 - 1.0 / S, -(1.0 - 1.0 / S), 0.5 / S, 1.5 / S, 2.5 / S, -0.5 / S, -1.5 / S, (S - 0.5) / S,
              -(S + 0.5) / S]
    v += [1.0 - 2.0 ** -15, -(1.0 - 2.0 ** -15), 1.22, -1.22, np.inf, -np.inf, 0.0]
    L = np.array(v, np.float32).view(np.uint32)
    special = np.array([0x7FC00000, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x80000100],
                       np.uint32)  # NaNs (quiet, payload, signalling), -0.f, subnormals of both signs
    noise = (np.random.default_rng(seed).standard_normal(1000) * 0.3).astype(np.float32).view(np.uint32)
    L = np.concatenate([L, special, noise]).view(np.float32)
    R = np.concatenate([L[37:], L[:37]])[::-1].copy()
    return L, R
