"""The true-peak meter on the GPU (tbf_true_peak_*, k_tpeak): identity in bits of every row's peaks
with the host restatement of the definition (tbf_debug_true_peak_ref) at every layout the kernel
takes, aimed bursts that put a row's maximum on the frames where the kernel could go wrong, rows
streaming at their own counts, reset and isolation, meters of different factors, the refusals, the
accounting, the mix -> measure -> gain -> measure chain, and Loudness.range on a device meter.

The stage is this project's own definition (include/tbf.h); the restatement
against exact arithmetic, the tap order, the sines and the range arithmetic are checked without a
GPU (tests/test_truepeak_cpu.py).  A NaN peak is compared as "is NaN", everything else in bits."""
import numpy as np
import pytest

import loudness_model as LM
import scenarios as S
import truepeak_model as M

pytestmark = pytest.mark.gpu

TONEGEN = 1
FILL = 777.0
bits = M.bits


def engine(n=0, chain=0):
    import tunebfree_amd as T
    eng = T.Engine(sample_rate=48000.0, device=0, chain=chain)
    if n:
        tid = eng.template(seed=7)
        eng.add_instances([tid] * n, [4100 + 37 * i for i in range(n)])
    return eng


def tile():
    import tunebfree_amd as T
    t, per_lane, _g, lds = T.Engine.true_peak_grid(1, 1)
    assert t >= 64 and t % per_lane == 0 and lds <= 160 * 1024
    return t


class Ref:
    """the rows of a meter on the host: true_peak_ref per row, the histories and peaks carried"""

    def __init__(self, n, F=4):
        self.n, self.F = n, F
        self.hist, self.peaks = [None] * n, [None] * n
        self.pos = np.zeros(n, np.int64)

    def reset(self, rows=None):
        for r in (range(self.n) if rows is None else rows):
            self.hist[r], self.peaks[r], self.pos[r] = None, None, 0

    def call(self, L, R, counts=None):
        import tunebfree_amd as T
        for r in range(self.n):
            c = L.shape[1] if counts is None else int(counts[r])
            self.peaks[r], self.hist[r] = T.Engine.true_peak_ref(L[r, :c], L[r, :c] if R is L else R[r, :c], self.F,
                                                                 hist=self.hist[r], peaks=self.peaks[r])
            self.pos[r] += c

    def words(self, r):
        return np.zeros(4, np.uint32) if self.peaks[r] is None else self.peaks[r]


def measure(tp, L, R, aligned=True, counts=None):
    """one tbf_true_peak_device call in torch memory: aligned -- every row 16-byte aligned, even
    strides; otherwise everything one float into its allocation with odd strides.  R is L: one
    plane passed twice.  Asserts that the call left the planes, pads included, as they were."""
    import torch
    n, frames = L.shape
    lead = 0 if aligned else 1
    stride = (frames + 3) // 4 * 4 + (0 if aligned else 1)
    host, dev = [], []
    for src in ((L,) if R is L else (L, R)):
        a = np.full(lead + n * stride + 4, FILL, np.float32)
        a[lead:lead + n * stride].reshape(n, stride)[:, :frames] = src
        host.append(a)
        dev.append(torch.from_numpy(a).cuda())
    torch.cuda.synchronize()
    assert all(t.data_ptr() % 16 == 0 for t in dev)
    ptr = [t.data_ptr() + 4 * lead for t in dev]
    tp.measure_device(ptr[0], ptr[-1], stride, frames, counts=counts)
    torch.cuda.synchronize()
    for a, t in zip(host, dev):
        assert a.tobytes() == t.cpu().numpy().tobytes(), "the meter wrote into its input"


def read_guarded(tp, rows=None):
    k = tp.n_rows if rows is None else len(rows)
    buf = np.zeros(k + 2, M.RESULT_DTYPE)
    raw = buf.view(np.uint8).reshape(k + 2, 32)
    raw[0], raw[-1] = 0xA5, 0xA5
    r = None if rows is None else np.ascontiguousarray(rows, np.uint32)
    rc = tp._lib.tbf_true_peak_read(tp._h, 0 if r is None else len(r), None if r is None else r.ctypes.data, buf[1:].ctypes.data)
    assert rc == 0, rc
    assert (raw[0] == 0xA5).all() and (raw[-1] == 0xA5).all(), "results written outside the rows asked for"
    return buf[1:-1].copy()


def words(rec):
    """a result record's four peaks as words: sample L, sample R, inter L, inter R"""
    return np.concatenate([bits(rec["sample_peak"]), bits(rec["inter_peak"])])


def check(tp, ref, what, rows=None):
    """every row's peaks, frames and dbtp against the reference: bits, a NaN as a NaN"""
    res = read_guarded(tp)
    for r in (range(ref.n) if rows is None else rows):
        got, want = words(res[r]), ref.words(r)
        for k in range(4):
            if M.is_nan_word(want[k]):
                assert M.is_nan_word(got[k]), (what, r, k, hex(int(got[k])))
            else:
                assert int(got[k]) == int(want[k]), f"{what}: row {r} word {k}: {int(got[k]):#x} against true_peak_ref's {int(want[k]):#x}"
        assert res["frames"][r] == ref.pos[r], (what, r)
        d = M.dbtp(want)
        assert (np.isnan(d) and np.isnan(res["dbtp"][r])) or res["dbtp"][r] == d or abs(res["dbtp"][r] - d) < 1e-9, (what, r)


def counts_for(n, frames, seed):
    """0, 1, 5, partial and full counts"""
    c = np.random.default_rng(seed).integers(0, frames + 1, n).astype(np.uint32)
    c[0::7] = frames
    c[1::7] = 0
    c[2::7] = min(1, frames)
    c[3::7] = frames // 2
    c[4::7] = min(5, frames)
    return c


def with_nan_beyond(x, counts):
    x = x.copy()
    for r, c in enumerate(counts):
        x[r, int(c):] = np.nan
    return x


@pytest.fixture(scope="module")
def eng():
    e = engine()
    yield e
    e.close()


# ---------------------------------------------------------------- 1. layouts
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd"])
@pytest.mark.parametrize("n", [1, 31, 33, 70])
def test_gpu_truepeak_layouts_against_ref(eng, n, aligned):
    """frame counts around the history (10, 11, 12), the wave and the tile, with and without counts
    (0, 1, 5, partial and full, NaN behind each), and one call with d_L == d_R; the calls follow each
    other on one meter, so every one but the first reads a history, and each is louder than the one
    before, so that its frames set the peaks"""
    t = tile()
    tp, ref = eng.true_peak(n, oversample=4), Ref(n)
    amp = 0.05
    for k, frames in enumerate([1, 10, 11, 12, 63, 65, t - 1, t, t + 1, 2 * t + 13]):
        what = f"rows={n} aligned={aligned} frames={frames}"
        amp *= 1.2
        L, R = M.noise(100 + k, frames, n, amp), M.noise(200 + k, frames, n, amp)
        measure(tp, L, R, aligned)
        ref.call(L, R)
        check(tp, ref, what)
        amp *= 1.2
        c = counts_for(n, frames, 300 + k)
        Ln, Rn = with_nan_beyond(M.noise(400 + k, frames, n, amp), c), with_nan_beyond(M.noise(500 + k, frames, n, amp), c)
        measure(tp, Ln, Rn, aligned, c)
        ref.call(Ln, Rn, c)
        check(tp, ref, what + " with counts")
        if frames == 65:
            amp *= 1.2
            L = M.noise(600, frames, n, amp)
            measure(tp, L, L, aligned)
            ref.call(L, L)
            check(tp, ref, what + " d_L == d_R")
    res = tp.read()
    assert np.isfinite(res["dbtp"]).all() and (res["inter_peak"] > 0).all()
    tp.close()


# ---------------------------------------------------------------- 2. aimed bursts
def test_gpu_truepeak_aimed_bursts(eng):
    """A maximum hides errors, so it is aimed: one call of 70 rows behind a call of 40 frames, row r
    with the burst matched to a phase at its own frame n0 of the call, in noise of amplitude 0.01.
    Together the rows stand on the call's first 12 frames (whose taps reach into the call before),
    its last frame, both sides of every lane, wave and tile edge, and every phase.  First the
    placement is asserted on true_peak_ref's y; then the device's peak must be that y in bits."""
    import tunebfree_amd as T
    t, n, before = tile(), 70, 40
    frames = 2 * t + 13
    targets = list(range(12)) + [frames - 1, 63, 64, 65, 255, 256, 257, t - 2, t - 1, t, t + 1, t + 11, t + 12,
                                 2 * t - 1, 2 * t, 2 * t + 1, 2 * t + 12, t // 2 + 3, t + t // 4, 12, 13, t + 256, 2 * t + 5]
    assert len(targets) == 35
    tp, ref = eng.true_peak(n, oversample=4), Ref(n)
    L, R = np.zeros((n, before + frames), np.float32), np.zeros((n, before + frames), np.float32)
    aim = []
    for r in range(n):
        n0, p = targets[r % 35], (r + 2 * (r // 35)) % 4      # 35 targets, each with two phases, R with the two others
        aim.append((n0, p, (p + 2) % 4))
        L[r] = M.aimed(1000 + r, before + frames, before + n0, p)
        R[r] = M.aimed(2000 + r, before + frames, before + n0, (p + 2) % 4)
    for r, (n0, p, q) in enumerate(aim):
        w, _h, y = T.Engine.true_peak_ref(L[r], R[r], 4, want_y=True)
        for ch, ph in ((0, p), (1, q)):
            at, where, ratio = M.argmax_y(y[ch])
            assert (at, where) == (before + n0, ph) and ratio > 1.05, (r, ch, at, where, ratio)
            assert int(w[2 + ch]) == M.word(y[ch][before + n0, ph]) > M.word(1.0) == int(w[ch])
    assert {p for _n0, p, _q in aim} == {0, 1, 2, 3}
    measure(tp, L[:, :before], R[:, :before])
    ref.call(L[:, :before], R[:, :before])
    measure(tp, L[:, before:], R[:, before:], aligned=False)
    ref.call(L[:, before:], R[:, before:])
    check(tp, ref, "aimed bursts")
    for r in range(n):       # the cut moved nothing in the reference either
        w, _h = T.Engine.true_peak_ref(L[r], R[r], 4)
        assert np.array_equal(w, ref.words(r)), r
    tp.close()


def test_gpu_truepeak_aimed_at_a_later_calls_head(eng):
    """the same on the heads of a third and fourth call, where the live side of the history has
    flipped twice: bursts that straddle the cuts at 1, 5, 10 and 11 frames into a call"""
    import tunebfree_amd as T
    n, cuts = 16, [0, 30, 37, 47, 500]
    tp, ref = eng.true_peak(n, oversample=4), Ref(n)
    x = np.zeros((n, cuts[-1]), np.float32)
    for r in range(n):
        n0 = (37, 47)[r % 2] + (0, 1, 5, 10, 11, 0, 2, 7)[r // 2]
        x[r] = M.aimed(3000 + r, cuts[-1], n0, r % 4)
        _w, _h, y = T.Engine.true_peak_ref(x[r], x[r], 4, want_y=True)
        assert M.argmax_y(y[0])[:2] == (n0, r % 4)
    for a, b in zip(cuts[:-1], cuts[1:]):
        measure(tp, x[:, a:b], x[:, a:b], aligned=bool(a % 2))
        ref.call(x[:, a:b], x[:, a:b])
    check(tp, ref, "bursts across later cuts")
    for r in range(n):
        w, _h = T.Engine.true_peak_ref(x[r], x[r], 4)
        assert np.array_equal(w, ref.words(r)), r
    tp.close()


# ---------------------------------------------------------------- 3. the other factors
@pytest.mark.parametrize("F", [2, 1])
def test_gpu_truepeak_other_factors(eng, F):
    """F = 2 takes phases 0 and 2 only and F = 1 none, so that inter_peak stays 0; bursts (the first
    row's across the cut between the two calls) in L, noise in R"""
    t, n = tile(), 9
    tp, ref = eng.true_peak(n, oversample=F), Ref(n, F)
    assert tp.oversample == F
    x = np.stack([M.aimed(4000 + r, t + 40, (15, 30, t - 1, t, t + 20)[r % 5], (0, 2, 1, 3)[r % 4]) for r in range(n)])
    y = M.noise(41, t + 40, n, 0.5)
    for k, (a, b) in enumerate([(0, 7), (7, t + 40)]):
        measure(tp, x[:, a:b], y[:, a:b], aligned=bool(k))
        ref.call(x[:, a:b], y[:, a:b])
        check(tp, ref, f"F={F} call {k}")
    res = tp.read()
    if F == 1:
        assert not res["inter_peak"].any() and (res["sample_peak"][:, 0] == 1.0).all()
        assert (res["dbtp"] == 0.0).all()
    else:      # a burst matched to phase 0 or 2 is seen, one matched to 1 or 3 only in part
        seen = np.array([(0, 2, 1, 3)[r % 4] in (0, 2) for r in range(n)])
        assert (res["inter_peak"][seen, 0] > 1.0).all()
    tp.close()
    assert [eng.true_peak(1, rate_hz=r).oversample for r in (44100, 96000, 192000)] == [4, 2, 1]
    assert eng.true_peak(1).oversample == 4          # the engine's 48 kHz


# ---------------------------------------------------------------- 4. streaming
def test_gpu_truepeak_rows_stream_at_their_own_counts(eng):
    """12 rows take random counts over 10 calls, small ones included, so that histories are shifted
    and rows stand on different sides: the peaks are those of one true_peak_ref run per row over its
    own frames"""
    import tunebfree_amd as T
    n, calls = 12, 10
    tp, ref = eng.true_peak(n, oversample=4), Ref(n)
    rng = np.random.default_rng(43)
    rowsL, rowsR = [[] for _ in range(n)], [[] for _ in range(n)]
    for k in range(calls):
        frames = int(rng.integers(20, 1500))
        counts = rng.integers(0, frames + 1, n).astype(np.uint32)
        counts[k % n], counts[(k + 1) % n], counts[(k + 2) % n], counts[(k + 3) % n] = frames, 0, 3, 10
        amp = 0.1 * 1.2 ** k
        L, R = with_nan_beyond(M.noise(500 + k, frames, n, amp), counts), with_nan_beyond(M.noise(600 + k, frames, n, amp), counts)
        measure(tp, L, R, aligned=bool(k % 2), counts=counts)
        ref.call(L, R, counts)
        check(tp, ref, f"streaming, call {k}")
        for r in range(n):
            rowsL[r].append(L[r, :counts[r]]), rowsR[r].append(R[r, :counts[r]])
    assert len(set(ref.pos.tolist())) > 6
    for r in range(n):   # the reference's own cuts moved nothing either
        one, _h = T.Engine.true_peak_ref(np.concatenate(rowsL[r]), np.concatenate(rowsR[r]), 4)
        assert np.array_equal(one, ref.words(r)), r
    tp.close()


# ---------------------------------------------------------------- 5. reset and isolation
def test_gpu_truepeak_reset_nan_and_two_meters(eng):
    """rows {1, 5} reset mid-stream start anew (history included) and the others go on; a NaN row
    stays NaN until it is reset and leaves its neighbours clean; a second meter of another factor
    goes its own way"""
    n, frames = 8, 300
    a, b = eng.true_peak(n, oversample=4), eng.true_peak(n, oversample=2)
    ra, rb = Ref(n), Ref(n, 2)
    for k in range(5):
        amp = 0.5 if k < 2 else 0.1          # quieter after the resets: a row that kept its peaks would show
        L, R = M.noise(60 + k, frames, n, amp), M.noise(70 + k, frames, n, amp)
        if k == 1:
            L[3, 17] = np.nan
        if k == 2:
            a.reset([1, 5])
            ra.reset([1, 5])
        if k == 3:
            a.reset([3])
            ra.reset([3])
        measure(a, L, R, aligned=bool(k % 2))
        ra.call(L, R)
        measure(b, L, R)
        rb.call(L, R)
        check(a, ra, f"meter a, call {k}")
        check(b, rb, f"meter b, call {k}")
        res = a.read()
        if k == 2:
            assert np.isnan(res["sample_peak"][3, 0]) and np.isnan(res["inter_peak"][3, 0]) and np.isnan(res["dbtp"][3])
            assert np.isfinite(res["sample_peak"][3, 1]) and np.isfinite(res["inter_peak"][3, 1])
            assert np.isfinite(res["dbtp"][[0, 1, 2, 4, 5, 6, 7]]).all()
            assert res["frames"].tolist() == [900, 300, 900, 900, 900, 300, 900, 900]
            assert (res["sample_peak"][[1, 5]] <= 0.1).all() and (res["sample_peak"][[0, 2]] > 0.4).all()
    assert np.isfinite(a.read()["dbtp"]).all() and a.read()["frames"][3] == 600
    with pytest.raises(Exception, match=r"-22.*rows\[1\]"):
        a.reset([0, n])
    a.reset()
    ra.reset()
    L, R = M.noise(91, frames, n, 0.01), M.noise(92, frames, n, 0.01)
    measure(a, L, R)
    ra.call(L, R)
    check(a, ra, "after a reset of all rows")
    assert (a.read()["sample_peak"] <= 0.01).all()
    a.close(), b.close()


def test_gpu_truepeak_meters_destroyed_and_left_to_the_engine():
    import torch
    e = engine()
    x = torch.from_numpy(M.noise(5, 801, 3)).cuda()
    torch.cuda.synchronize()
    kept, gone = e.true_peak(3), e.true_peak(3)
    for tp in (kept, gone):
        tp.measure_device(x.data_ptr(), x.data_ptr(), 801, 801)
    want = kept.read()
    assert gone.read().tobytes() == want.tobytes()
    gone.close()
    gone.close()                                # a second close is nothing
    kept.measure_device(x.data_ptr(), x.data_ptr(), 801, 5)
    again = kept.read()
    assert again["frames"].tolist() == [806] * 3 and again["inter_peak"].tobytes() == want["inter_peak"].tobytes()
    e.close()                                   # releases `kept`
    kept.close()


# ---------------------------------------------------------------- 6. refusals
def test_gpu_truepeak_refusals_move_no_state(eng):
    """every bad argument is -22 and names it, and a valid call behind them gives the bits of a
    stream that never saw them"""
    import torch
    import tunebfree_amd as T
    n, frames = 4, 500
    tp, ref = eng.true_peak(n), Ref(n)
    L, R = M.noise(81, frames, n, 0.3), M.noise(82, frames, n, 0.3)
    measure(tp, L, R)
    ref.call(L, R)
    stride = frames + 4
    loud = [np.ascontiguousarray(np.pad(a * 3.0, ((0, 0), (0, 4)))) for a in (L, R)]     # what a refused call must not take
    x = [torch.from_numpy(a).cuda() for a in loud]
    torch.cuda.synchronize()
    xl, xr = x[0].data_ptr(), x[1].data_ptr()
    good = dict(L_ptr=xl, R_ptr=xr, in_stride=stride, frames=frames, counts=None)
    over = np.full(n, frames, np.uint32)
    over[2] = frames + 1
    bad = [
        (dict(L_ptr=None), "d_L"),
        (dict(R_ptr=None), "d_R"),
        (dict(in_stride=frames - 1), "in_stride"),
        (dict(L_ptr=xl + 2), "aligned"),
        (dict(R_ptr=xr + 1), "aligned"),
        (dict(counts=over), r"counts\[2\]"),
    ]
    for kw, word in bad:
        with pytest.raises(T.TbfError, match="-22.*" + word):
            tp.measure_device(**{**good, **kw})
    with pytest.raises(T.TbfError, match=r"-22.*rows\[1\]"):
        tp.reset([0, n])
    with pytest.raises(T.TbfError, match=r"-22.*rows\[0\]"):
        tp.read([n])
    assert tp._lib.tbf_true_peak_read(tp._h, 0, None, None) == -22
    check(tp, ref, "behind the refusals")
    assert x[0].cpu().numpy().tobytes() == loud[0].tobytes()
    c2 = np.array([7, 0, 500, 11], np.uint32)
    L2, R2 = M.noise(83, frames, n, 0.5), M.noise(84, frames, n, 0.5)
    measure(tp, L2, R2, counts=c2)
    ref.call(L2, R2, c2)
    check(tp, ref, "a valid call behind the refusals")
    got = tp.read([2, 0])                      # rows in the order asked for
    assert got["frames"].tolist() == [1000, 507]
    tp.close()


# ---------------------------------------------------------------- 7. accounting
def test_gpu_truepeak_accounting():
    """a meter is no instance or stage memory of the engine, a call that takes frames is one launch
    and one that takes none is none, and the render kernels' launch counts do not move"""
    import torch
    e = engine(2)
    e.render(2)
    b0, l0 = e.device_bytes(), e.launches()
    tp = e.true_peak(64)
    e.true_peak(3, oversample=1)   # left to the engine
    assert e.device_bytes() == b0
    x = torch.zeros((64, 256), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tp.timing(True)
    for _ in range(3):
        tp.measure_device(x.data_ptr(), x.data_ptr(), 256, 256)
    tp.measure_device(x.data_ptr(), x.data_ptr(), 256, 256, counts=np.zeros(64, np.uint32))
    tp.measure_device(x.data_ptr(), x.data_ptr(), 256, 0)
    e.synchronize()
    ms, k = tp.timing()
    assert k == 3 and ms > 0.0
    tp.timing(False)
    tp.measure_device(x.data_ptr(), x.data_ptr(), 256, 256)
    assert tp.timing() == (0.0, 0)
    res = tp.read()
    assert res["frames"].tolist() == [1024] * 64 and (res["dbtp"] == -np.inf).all()      # silence
    assert tp.gains(-1.0).tolist() == [1.0] * 64
    assert e.device_bytes() == b0 and e.launches() == l0
    e.close()


# ---------------------------------------------------------------- 8. the chain
def test_gpu_truepeak_measure_gain_measure():
    """16 tone generators mixed to 2 buses over 64 blocks at 48 kHz: the meter on the bus planes is
    true_peak_ref of those planes, which are those of a twin engine without a meter.  The planes are
    then brought to about +2 dBTP through mix_device, metered, and the gains of gains(-1.0) applied
    through mix_device give planes that a further meter reads at no more than -1.0 dBTP + 0.01 dB.

    The margin: gains() rounds g <= 10**((-1 - dbtp) / 20) to float32 (relative error 2^-24) and
    k_mix rounds every product g * x once more (2^-24), so every input of the second measurement
    is g x (1 + d), |d| <= 2^-23; the chain of 12 fmaf adds at most 12 * 2^-24 * sum |h| * max |x|.
    With sum |h| <= 2.03 and max |x| <= the peak (the samples are part of it) the peak read is at
    most g * peak * (1 + 14 * 2.03 * 2^-24) = 1.7e-6 relative, 1.5e-5 dB: far inside 0.01 dB."""
    import torch
    import tunebfree_amd as T
    n, buses, nb = 16, 2, 64
    frames = nb * 128
    bus = np.arange(n) % buses

    def render(metered):
        e = engine(n, TONEGEN)
        for i in range(n):
            for (_b, kind, x, v) in S.bench_scenario(i):
                (e.note if kind == "note" else e.set_param)(i, x, v)
            for j in range(9):   # a registration of its own per instance
                e.set_param(i, S.P_DRAWBAR + j, (3 * i + 5 * j) % 9)
        mix = [torch.full((buses, frames), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        tp = e.true_peak(buses) if metered else None
        e.render_mix_device(nb, T.params.mix_rows(bus, 0.05), buses, mix[0].data_ptr(), mix[1].data_ptr(), frames)
        if metered:
            tp.measure_device(mix[0].data_ptr(), mix[1].data_ptr(), frames, frames)   # on the same stream
        e.synchronize()
        return e, tp, mix

    def plane_pair():
        p = [torch.full((buses, frames), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        return p

    def against_ref(tp, planes, what):
        res = tp.read()
        for b in range(buses):
            w, _h = T.Engine.true_peak_ref(planes[0][b], planes[1][b], 4)
            assert np.array_equal(words(res[b]), w), f"{what}: bus {b} against true_peak_ref of the planes"
            assert res["frames"][b] == frames and abs(res["dbtp"][b] - M.dbtp(w)) < 1e-9
        return res

    e, tp, mix = render(True)
    assert tp.oversample == 4
    planes = [t.cpu().numpy().copy() for t in mix]
    assert np.isfinite(planes[0]).all() and float(np.abs(planes[0]).max()) > 1e-3
    res = against_ref(tp, planes, "the mix")
    # to about +2 dBTP
    boost = (10.0 ** ((2.0 - res["dbtp"]) / 20.0)).astype(np.float32)
    hot = plane_pair()
    e.mix_device(buses, mix[0].data_ptr(), mix[1].data_ptr(), frames, frames, T.params.gain_rows(boost), buses,
                 hot[0].data_ptr(), hot[1].data_ptr(), frames)
    tph = e.true_peak(buses)
    tph.measure_device(hot[0].data_ptr(), hot[1].data_ptr(), frames, frames)
    rh = against_ref(tph, [t.cpu().numpy() for t in hot], "the boosted mix")
    assert (np.abs(rh["dbtp"] - 2.0) < 0.001).all()
    gains = tph.gains(-1.0)
    assert gains.dtype == np.float32 and (gains < 1.0).all()
    for b in range(buses):
        assert gains[b] == np.float32(10.0 ** ((-1.0 - rh["dbtp"][b]) / 20.0))
    out = plane_pair()
    e.mix_device(buses, hot[0].data_ptr(), hot[1].data_ptr(), frames, frames, T.params.gain_rows(gains), buses,
                 out[0].data_ptr(), out[1].data_ptr(), frames)
    tp2 = e.true_peak(buses)
    tp2.measure_device(out[0].data_ptr(), out[1].data_ptr(), frames, frames)
    after = against_ref(tp2, [t.cpu().numpy() for t in out], "the mix at the ceiling")
    for b in range(buses):
        print(f"bus {b}: {res['dbtp'][b]:+.4f} dBTP mixed, {rh['dbtp'][b]:+.4f} boosted, gain {gains[b]}, {after['dbtp'][b]:+.6f} after")
        assert -1.01 <= after["dbtp"][b] <= -1.0 + 0.01
    assert tp.gains(20.0).tolist() == [1.0, 1.0]       # capped at unity
    e.close()
    e2, _, twin = render(False)
    assert twin[0].cpu().numpy().tobytes() == planes[0].tobytes(), "mix planes with and without a meter, L"
    assert twin[1].cpu().numpy().tobytes() == planes[1].tobytes(), "mix planes with and without a meter, R"
    e2.close()


# ---------------------------------------------------------------- 9. the loudness range on a device meter
def test_gpu_loudness_range_of_a_device_meter(eng):
    """Loudness.range is loudness_range of the meter's own hops: rows at different level steps, one
    silent, one too short for a window"""
    import torch
    import tunebfree_amd as T
    rate, n = 8000, 5
    frames = 45 * 800
    x = np.zeros((n, frames), np.float32)
    x[0] = LM.sine(rate, [(-20.0, 2.25), (-30.0, 2.25)], 997.0)
    x[1] = LM.sine(rate, [(-40.0, 2.0), (-20.0, 2.5)], 440.0)
    x[2] = LM.noise(5, frames, scale=0.1) * np.linspace(0.05, 1.0, frames, dtype=np.float32)
    x[4] = LM.noise(6, frames, scale=0.1)
    counts = np.array([frames, frames, frames, frames, 29 * 800 + 799], np.uint32)
    lm = eng.loudness(n, rate, max_hops=64)
    d = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    lm.measure_device(d.data_ptr(), d.data_ptr(), frames, frames, counts=counts)
    lra, win = lm.range()
    for r in range(n):
        want = T.Engine.loudness_range(rate, lm.hops(r))
        assert (lra[r], win[r]) == want, (r, lra[r], win[r], want)
    print("LRA", lra.tolist(), "windows", win.tolist())
    assert (lra[:3] > 0.0).all()                 # three rows whose level moves
    assert (lra[3], win[3]) == (0.0, 0) and (lra[4], win[4]) == (0.0, 0) and win[0] == 16
    got, w2 = lm.range([2, 0])
    assert got.tolist() == [lra[2], lra[0]] and w2.tolist() == [win[2], win[0]]
    with pytest.raises(T.TbfError, match=r"-22.*rows\[0\]"):
        lm.range([n])
    lm.close()
